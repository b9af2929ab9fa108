"""The Gumbel host model (tests/gumbel_model.py) on the CPU, before tests/test_gumbel_gpu.py uses it to judge the engine: the
considered-visit table equals a literal transcription of the mctx recipe; per move the visits sum to S, at most k children are
visited, the played child is a most-visited one, the quantised target sums to 65535 within cnt / 2 and (m = 4) puts mass on
unvisited children somewhere in every game; with the option off the model is playout_cap_model.play_game on every recorded game."""
import math

import numpy as np
import pytest

import golden_io as G
import gumbel_model as GM
import playout_cap_model as PC

GUMBEL = (50.0, 1.0)


def mctx_sequence_of_considered_visits(max_num_considered_actions, num_simulations):
    """`get_sequence_of_considered_visits` of mctx (seq_halving.py), transcribed statement for statement."""
    if max_num_considered_actions <= 1:
        return tuple(range(num_simulations))
    log2max = int(math.ceil(math.log2(max_num_considered_actions)))
    sequence = []
    visits = [0] * max_num_considered_actions
    num_considered = max_num_considered_actions
    while len(sequence) < num_simulations:
        num_extra_visits = max(1, int(num_simulations / (log2max * num_considered)))
        for _ in range(num_extra_visits):
            sequence.extend(visits[:num_considered])
            for i in range(num_considered):
                visits[i] += 1
        # Halving the number of considered actions.
        num_considered = max(2, num_considered // 2)
    return tuple(sequence[:num_simulations])


@pytest.mark.parametrize("S", [1, 8, 24, 100, 200, 800])
def test_table_is_the_mctx_recipe(S):
    for k in range(1, 129):
        want = mctx_sequence_of_considered_visits(k, S)
        got = GM.considered_visits(k, S)
        assert len(got) == S and tuple(got) == want, k
        # within a phase (a run that ends where the count falls back for the halved set) the count never decreases, and a
        # phase starts where the previous one's candidates stand
        drops = [t for t in range(1, S) if got[t] < got[t - 1]]
        assert all(got[t] <= got[t - 1] and got[t] >= 0 for t in drops)
        lo = 0
        for hi in drops + [S]:
            run = got[lo:hi]
            assert all(b - a in (0, 1) for a, b in zip(run, run[1:])), (k, lo, hi)
            lo = hi
        assert got[0] == 0 and max(got) < S


def _trace(idx):
    t = G.game_traces()[idx]
    return t["cfg"], t["stub"] == "peaked", t["seed"]


@pytest.mark.parametrize("idx", range(4))
def test_gumbel_off_is_the_playout_cap_model(idx):
    cfg, peaked, seed = _trace(idx)
    want, w_winner, w_plies, w_stats = PC.play_game(cfg, peaked, seed)
    got, winner, plies, stats = GM.play_game(cfg, peaked, seed, gumbel=None)
    assert (winner, plies) == (w_winner, w_plies) and len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a["actions"]) == list(b["actions"]) and list(a["visits"]) == list(b["visits"])
        assert a["z"] == b["z"] and a["player"] == b["player"] and a["late"] == b["late"]
        assert bytes(a["board"]) == bytes(b["board"])
    assert stats["sims"] == w_stats["sims"]
    assert stats["gumbel_moves"] == stats["gumbel_considered"] == stats["gumbel_offprior"] == 0


@pytest.mark.parametrize("m", [4, 16])
@pytest.mark.parametrize("idx", range(4))
def test_per_move_invariants(idx, m):
    cfg, peaked, seed = _trace(idx)
    S = int(cfg["num_simulations"])
    got, winner, plies, st = GM.play_game(cfg, peaked, seed, gumbel=(m,) + GUMBEL)
    assert len(got) == st["gumbel_moves"] == len(st["moves"]) > 0 and st["sims"] == S * len(got)
    assert math.isfinite(st["min_gap"]) and st["min_gap"] >= 0.0
    considered = 0
    for smp, mv in zip(got, st["moves"]):
        cnt = len(smp["actions"])
        N = mv["visits"]
        k = min(m, cnt)
        assert mv["considered"] == k and int(N.sum()) == S == mv["sum_n"]
        assert mv["visited"] == int((N > 0).sum()) <= k
        assert int(N[mv["played"]]) == int(N.max()) == mv["max_n"]
        t = smp["visits"]
        assert len(t) == cnt and (t >= 0).all() and (t <= 65535).all()
        assert abs(int(t.sum()) - 65535) <= cnt / 2
        assert not smp["late"]
        assert abs(float(mv["pi"].sum()) - 1.0) < 1e-12 and -1.0 <= mv["v_mix"] <= 1.0
        considered += k
    assert considered == st["gumbel_considered"] <= m * st["gumbel_moves"]
    assert 0 <= st["gumbel_offprior"] <= st["gumbel_moves"]


@pytest.mark.parametrize("idx", range(4))
def test_unvisited_children_carry_target_mass_in_every_game(idx):
    """The target is not the visit counts: somewhere in each game an unvisited child has a non-zero quantised target.  m = 4: with
    the stub's widely spread values and S <= 24, sixteen considered moves leave the best q so far above v_mix that sigma
    (scale >= 50) drives every unvisited child's share below 2^-17 in three of the four games; four considered moves do not."""
    cfg, peaked, seed = _trace(idx)
    got, _, _, st = GM.play_game(cfg, peaked, seed, gumbel=(4,) + GUMBEL)
    assert sum(mv["unvisited_with_target"] for mv in st["moves"]) > 0
    for smp, mv in zip(got, st["moves"]):
        assert mv["unvisited_with_target"] == int(((mv["visits"] == 0) & (smp["visits"] > 0)).sum())


def test_first_simulations_take_the_top_k_of_g_plus_l():
    """The equal-visit rule is the Gumbel-top-k trick: after k simulations exactly the k largest g + l have one visit each."""
    from oracle import xq_oracle as O
    import leaf_batch_model as LB
    from draws import Draws
    g = O.Game()
    n = len(g.legal_actions())
    for m, S in ((4, 4), (8, 8), (16, 16)):
        gs = GM.injected_gumbels(Draws(11).s_dirichlet, n)
        s = GM.search(g, S, LB.stub_priors(True), gs, (m, 50.0, 1.0))
        f = int(s.first[0])
        top = set(np.argsort(-s.P64[f:f + n], kind="stable")[:m].tolist())
        assert set(np.nonzero(s.N[f:f + n])[0].tolist()) == top and int(s.N[f:f + n].max()) == 1


def test_parameters_are_rounded_to_float32_once():
    cfg, peaked, seed = _trace(1)
    a = GM.play_game(cfg, peaked, seed, gumbel=(8, 50.0 + 2.0 ** -30, 1.0 + 2.0 ** -40))
    b = GM.play_game(cfg, peaked, seed, gumbel=(8, 50.0, 1.0))
    assert a[1:3] == b[1:3] and all(list(x["visits"]) == list(y["visits"]) for x, y in zip(a[0], b[0]))
