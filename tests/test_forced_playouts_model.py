"""The forced-playouts host model (tests/forced_playouts_model.py) on the CPU, before tests/test_forced_playouts_gpu.py uses it to
judge the engine: with the option off it is playout_cap_model.play_game on every recorded game; with k = 2**-40 (k S < 1: no
child is ever forced, no visit subtracted) it replays that game sample for sample; with k = 2 the pruned counts obey the rules'
invariants and every tested game exercises forcing, pruning and outright removal (a game that did not would prove nothing)."""
import numpy as np
import pytest

import forced_playouts_model as FP
import golden_io as G
import playout_cap_model as PC

TINY = 2.0 ** -40
STAT_KEYS = ("sims", "reused_visits", "reroots", "fast_moves", "fast_sims", "full_moves")


def _same_samples(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a["actions"]) == list(b["actions"]) and list(a["visits"]) == list(b["visits"])
        assert a["z"] == b["z"] and a["player"] == b["player"] and a["late"] == b["late"]
        assert bytes(a["board"]) == bytes(b["board"])


def _trace(idx):
    t = G.game_traces()[idx]
    return t["cfg"], t["stub"] == "peaked", t["seed"]


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("idx", range(4))
def test_forced_off_is_the_playout_cap_model(idx, reuse):
    cfg, peaked, seed = _trace(idx)
    want, w_winner, w_plies, w_stats = PC.play_game(cfg, peaked, seed, tree_reuse=reuse)
    got, winner, plies, stats = FP.play_game(cfg, peaked, seed, tree_reuse=reuse, cap=None, forced=None)
    assert (winner, plies) == (w_winner, w_plies)
    _same_samples(got, want)
    assert all(stats[k] == w_stats[k] for k in STAT_KEYS)
    assert stats["forced_sims"] == stats["pruned_visits"] == stats["pruned_children"] == 0


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("idx", range(4))
def test_tiny_k_replays_the_forced_off_game(idx, reuse):
    cfg, peaked, seed = _trace(idx)
    assert TINY * int(cfg["num_simulations"]) < 1
    want, w_winner, w_plies, w_stats = PC.play_game(cfg, peaked, seed, tree_reuse=reuse)
    got, winner, plies, stats = FP.play_game(cfg, peaked, seed, tree_reuse=reuse, forced=TINY)
    assert (winner, plies) == (w_winner, w_plies)
    _same_samples(got, want)
    assert all(stats[k] == w_stats[k] for k in STAT_KEYS)
    assert stats["forced_sims"] == stats["pruned_visits"] == stats["pruned_children"] == 0
    assert len(stats["pruned"]) == stats["full_moves"] and all((p["v"] == p["N"]).all() for p in stats["pruned"])


@pytest.mark.parametrize("cap_p", [None, 0.5])
@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("idx", range(4))
def test_k_two_invariants(idx, reuse, cap_p):
    cfg, peaked, seed = _trace(idx)
    S = int(cfg["num_simulations"])
    cap = None if cap_p is None else (cap_p, max(1, S // 4))
    got, winner, plies, st = FP.play_game(cfg, peaked, seed, tree_reuse=reuse, cap=cap, forced=2.0)
    # the condition: this game exercises all three effects
    assert st["forced_sims"] > 0 and st["pruned_visits"] > 0 and st["pruned_children"] > 0
    assert len(got) == st["full_moves"] == len(st["pruned"])
    pv = pc = 0
    for smp, p in zip(got, st["pruned"]):
        N, v, d, cs = p["N"], p["v"], p["d"], p["cstar"]
        assert int(N.sum()) == S                                        # the tree keeps its real counts: a full move holds S visits
        assert (v <= N).all() and (v >= 0).all()
        assert cs == int(np.argmax(N)) and v[cs] == N[cs] and d[cs] == 0          # c* untouched
        assert not ((d > 0) & (v == 1)).any()                           # reduced to a single playout: removed
        assert ((d == 0) == (v == N)).all()
        assert (((d > 0) & (v > 0)) <= (v == N - d)).all() and (((d > 0) & (v == 0)) <= (N - d == 1)).all()
        assert (d.astype(np.float64) ** 2 < 2.0 * S).all()              # d <= sqrt(k S): the loop's bound
        assert list(smp["visits"]) == list(v) and 0 < int(v.sum()) <= S
        pv += int((N - v).sum())
        pc += int(((N > 0) & (v == 0)).sum())
    assert (pv, pc) == (st["pruned_visits"], st["pruned_children"])
    assert sum(int(s["visits"].sum()) for s in got) == S * st["full_moves"] - st["pruned_visits"]
    assert st["forced_sims"] <= st["sims"] - st["fast_sims"]
    if cap is None:
        assert st["fast_moves"] == 0
    else:
        assert st["fast_moves"] > 0 and st["fast_moves"] + st["full_moves"] == len(st["moves"])


def test_k_is_rounded_to_float32_once():
    cfg, peaked, seed = _trace(1)
    k = 2.0 + 2.0 ** -30                               # rounds to 2.0f
    a = FP.play_game(cfg, peaked, seed, forced=k)
    b = FP.play_game(cfg, peaked, seed, forced=2.0)
    _same_samples(a[0], b[0])
    assert a[3]["forced_sims"] == b[3]["forced_sims"]
