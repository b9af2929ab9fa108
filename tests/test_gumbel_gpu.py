"""The Gumbel root search with sequential halving on the GPU (k_select<false, false, false, true> / k_expand<false, false, true>,
xq_engine_init_gz).

* whole games with injected draws equal the host model (tests/gumbel_model.py): boards, actions, z, winner, plies and all counters
  exactly, the quantised improved policy within +-1 count per entry -- the four recorded configurations and a longer peaked game,
  m = 4 and m = 16, c_visit = 50, c_scale = 1.  The condition on the inputs is asserted: the model's smallest gap between winner
  and runner-up over every root arg-max of the game is above 1e-9.  Two float64 log implementations differ by a few ulp of
  |l| <= 88, about 4e-14, so no decision can flip, and a last-bit difference in exp can move a rounding by one count at most;
* search only (manual_moves = 1) with handed Gumbel values on the opening and 16 corpus positions: visits and W equal the model,
  the prior kind is 3 and the prior is g + l;
* the device's Gumbel draws over 1024 slots have the distribution's mean and variance and differ between slots;
* eager and graph-replayed steps give byte-identical records; Gumbel with the evaluation cache equals Gumbel alone;
* run_games on peaked weights with the device RNG: the counters add up and every sample is marked as an improved policy;
* the plain engine through xq_engine_init_gz(..., NULL) is byte-identical to xq_engine_init_fp and xq_engine_init.
"""
import ctypes as C
import math
import types

import numpy as np
import pytest

import golden_io as G
import gumbel_model as GM
import leaf_batch_model as LB
from draws import Stream
from oracle import xq_oracle as O
from test_hip_engine import _replay, _run_steps, _set_from_game
from test_playout_cap_gpu import _engine_cfg, _inject_array, _play_stub, _records_sha, _run
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator, _stub_step

pytestmark = pytest.mark.gpu

GAP = 1e-9
_LONG = dict(num_simulations=100, c_puct=1.5, temperature_threshold=10, max_game_length=70, random_opening_moves=4,
             enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
CONFIGS = [(t["cfg"], t["stub"] == "peaked", t["seed"], t["name"]) for t in G.game_traces()] + [(_LONG, True, 31, "long_peaked")]
# the seeds are the recorded games' own where the model's smallest arg-max gap on that game is above GAP (checked on the CPU);
# "natural" with m = 4 has an exact tie under its recorded seed 13 and plays seed 1
SEEDS = {("natural", 4): 1}
COUNTERS = ("sims", "gumbel_moves", "gumbel_considered", "gumbel_offprior")
OFF = ("fast_moves", "fast_sims", "reused_visits", "reroots", "forced_sims", "pruned_visits", "pruned_children", "collisions")


@pytest.mark.parametrize("m", [4, 16])
@pytest.mark.parametrize("game", CONFIGS, ids=[g[3] for g in CONFIGS])
def test_games_equal_host_model(game, m):
    from xiangqi_alphazero_amd import engine
    c, peaked, seed, name = game
    seed = SEEDS.get((name, m), seed)
    gumbel = (m, 50.0, 1.0)
    want, winner, plies, mst = GM.play_game(c, peaked, seed, gumbel=gumbel)
    print(name, "m", m, "seed", seed, "moves", len(want), "smallest arg-max gap", mst["min_gap"])
    assert mst["min_gap"] > GAP                        # the condition on the inputs: no decision can flip on a last-bit difference
    assert mst["gumbel_offprior"] > 0 and len(want) > 0
    n_slots, inj_len = 2, 16384
    eng = engine.SelfPlayEngine(_engine_cfg(engine, c, n_slots, inj_len, n_slots), inject=_inject_array([seed] * n_slots, inj_len),
                                gumbel=gumbel)
    assert eng.gumbel == gumbel
    st = _play_stub(eng, peaked, n_slots)
    samples, results = eng.drain()
    assert len(results) == n_slots
    for r in results:
        assert (int(r["winner"]), int(r["steps"]), int(r["n_samples"])) == (winner, plies, len(want))
    worst = 0
    for slot in range(n_slots):
        mine = samples[samples["slot"] == slot]
        mine = mine[np.argsort(mine["ply"], kind="stable")]
        assert len(mine) == len(want)
        for k, (s, w) in enumerate(zip(mine, want)):
            n = int(s["n_moves"])
            assert list(s["actions"][:n]) == list(w["actions"]), k
            assert int(s["z"]) == w["z"] and bytes(s["board"].view(np.int8)) == bytes(w["board"]), k
            assert int(s["side"]) == w["player"] and int(s["late_temp"]) == 0 and int(s["reserved0"]) == 1, k
            dv = np.abs(s["visits"][:n].astype(np.int64) - w["visits"])
            worst = max(worst, int(dv.max()))
            assert int(dv.max()) <= 1, (k, s["visits"][:n], w["visits"])
            assert not s["visits"][n:].any()
    print("largest |visits - model|", worst, {k: st[k] for k in COUNTERS})
    assert tuple(st[k] for k in COUNTERS) == tuple(n_slots * mst[k] for k in COUNTERS)
    assert st["samples_written"] == st["moves_played"] == n_slots * len(want)
    assert all(st[k] == 0 for k in OFF)


def test_search_only_with_handed_gumbels_equals_model():
    from xiangqi_alphazero_amd import engine
    d = G.corpus()
    picks = [i for i in range(5, len(d["board"]), 70) if not d["done"][i]][:16]
    games = [O.Game()] + [_replay([int(a) for a in d["taken"][i - d["ply"][i]:i]]) for i in picks]
    S, gumbel = 32, (8, 50.0, 1.0)
    eng = engine.SelfPlayEngine(engine.make_config(len(games), S, add_noise=True, manual_moves=True), gumbel=gumbel)
    priors = LB.stub_priors(True)
    handed = []
    for slot, g in enumerate(games):
        gs = GM.injected_gumbels(Stream(700 + slot, 3), len(g.legal_actions()))
        handed.append(gs)
        _set_from_game(eng, slot, g, gs)
    _run_steps(eng, S + 1, [True] * len(games))
    st = eng.stats()
    assert st["overflow"] == 0 and st["sims"] == S * len(games) and eng.held()
    assert st["gumbel_moves"] == 0 and st["moves_played"] == 0            # a search-only engine never plays the move
    v_hat = eng.gumbel_root_values().cpu().numpy()
    for slot, g in enumerate(games):
        s = GM.search(g, S, priors, handed[slot], gumbel)
        assert float(v_hat[slot]) == s.v_hat             # the root's network value, kept for the end of a move
        assert s.min_gap > GAP, slot
        want, r = s.root(), eng.read_root(slot)
        assert r["sims_done"] == S == r["root_visits"]
        assert list(r["actions"]) == list(want["actions"])
        assert list(r["visits"]) == list(want["visits"]), slot
        np.testing.assert_array_equal(r["total_value"], want["total_value"])
        assert r["prior_kind"] == 3 == want["prior_kind"] and r["prior_is_f64"]
        np.testing.assert_allclose(r["prior"], handed[slot] + s.l, rtol=0, atol=1e-12)      # g + l, l within a few ulp of 88
        assert int((r["visits"] > 0).sum()) <= 8


def test_device_gumbel_draws_have_the_distribution():
    import torch
    from xiangqi_alphazero_amd import engine
    n_slots = 1024
    eng = engine.SelfPlayEngine(engine.make_config(n_slots, 8, seed=21, manual_moves=True), gumbel=(16, 50.0, 1.0))
    g0 = O.Game()
    cnt = len(g0.legal_actions())
    assert cnt == 44
    for slot in range(n_slots):
        _set_from_game(eng, slot, g0)
    _stub_step(eng, True, {})                         # one step: the root request and its expansion
    assert eng.stats()["overflow"] == 0
    rootp_off = int(eng.h.p[12]) - int(eng.ws.data_ptr())
    rootp = eng.ws[rootp_off:rootp_off + n_slots * 128 * 8].view(torch.float64).view(n_slots, 128)[:, :cnt].cpu().numpy()
    tp = eng.arena_views()["P"][:, 1:1 + cnt].cpu().numpy()
    r = eng.read_root(5)
    assert r["prior_kind"] == 3 and len(r["prior"]) == cnt
    np.testing.assert_array_equal(r["prior"], rootp[5])
    assert (tp == tp[0]).all() and (tp > 0).all()      # one position: one set of float32 priors
    g = rootp - np.log(tp.astype(np.float64))
    n = g.size
    mean, var = float(g.mean()), float(g.var())
    print("n", n, "mean", mean, "variance", var, "want", 0.5772156649, math.pi ** 2 / 6)
    assert abs(mean - 0.5772156649) <= 0.03            # five standard errors of 1.2825 / sqrt(n) at n = 1024 x 44
    assert 5 * 1.2825 / math.sqrt(n) <= 0.0303
    assert abs(var / (math.pi ** 2 / 6) - 1.0) <= 0.08
    assert len({row.tobytes() for row in g}) == n_slots                    # slots differ
    assert int(eng.slot_ints[:, 14 + 2].min().item()) == cnt == int(eng.slot_ints[:, 14 + 2].max().item())   # the stream's counter


def _selfplay_gumbel(ev, graph, cache_entries=0, n_games=12, sims=24, seed=3, gumbel=(16, 50.0, 1.0)):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(n_games, sims, seed=seed, games_target=n_games, max_game_length=40)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, eval_cache_entries=cache_entries, gumbel=gumbel)
    st = _run(eng, n_games, graph, sims)
    sha, smp, res = _records_sha(eng)
    assert len(res) == n_games and st["samples_written"] == len(smp) == st["moves_played"] == st["gumbel_moves"] > 0
    assert (smp["reserved0"] == 1).all() and (smp["late_temp"] == 0).all()
    return st, sha


def test_eager_and_graph_replayed_steps_are_byte_identical():
    ev = _TorchStub()
    st_e, sha_e = _selfplay_gumbel(ev, False)
    st_g, sha_g = _selfplay_gumbel(ev, True)
    assert sha_e == sha_g
    assert all(st_e[k] == st_g[k] for k in COUNTERS + ("moves_played", "samples_written", "games_finished"))


def test_gumbel_with_eval_cache_equals_gumbel_alone():
    _, ev = _hip_evaluator()
    st, sha = _selfplay_gumbel(ev, True, 0, n_games=16)
    st_c, sha_c = _selfplay_gumbel(ev, True, 64, n_games=16)
    assert sha_c == sha and st_c["eval_cache_hits"] > 0
    assert all(st_c[k] == st[k] for k in COUNTERS + ("moves_played", "samples_written"))
    assert st_c["rows_evaluated"] < st["rows_evaluated"]


def test_run_games_counts_add_up():
    from xiangqi_alphazero_amd import selfplay
    S, m, games = 32, 16, 64
    net, _ = _hip_evaluator(policy_gain=8.0)           # peaked weights
    config = types.SimpleNamespace(num_simulations=S, c_puct=1.5, temperature_threshold=10, max_game_length=60,
                                   random_opening_moves=4, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
                                   gumbel_considered=m)        # through the config key, as AlphaZeroLoop's self-play passes it
    samples, results, st, _ = selfplay.run_games(net, config, games, seed=7)
    assert st["overflow"] == 0 and len(results) == games == st["games_finished"]
    assert st["gumbel"] == (m, 50.0, 1.0)
    assert st["gumbel_moves"] == st["moves_played"] == st["samples_written"] == len(samples) == int(results["n_samples"].sum())
    assert st["sims"] == S * st["gumbel_moves"]
    assert 0 < st["gumbel_considered"] <= m * st["gumbel_moves"]
    assert st["gumbel_offprior"] > 0
    assert (samples["reserved0"] == 1).all() and (samples["late_temp"] == 0).all()
    unvisited_mass = 0.0
    for s in samples[:256]:
        n = int(s["n_moves"])
        assert abs(int(s["visits"][:n].astype(np.int64).sum()) - 65535) <= n / 2
        np.testing.assert_array_equal(s["actions"][:n], O.legal_actions(s["board"], int(s["side"])))
        unvisited_mass += float(np.sort(s["visits"][:n].astype(np.float64))[:max(0, n - m)].sum()) / 65535.0
    print("moves", st["gumbel_moves"], "considered per move", st["gumbel_considered"] / st["gumbel_moves"], "off-prior share",
          st["gumbel_offprior"] / st["gumbel_moves"], "target mass outside the m largest entries (first 256 samples)",
          unvisited_mass / min(256, len(samples)))


def test_plain_engine_through_init_gz_null_is_byte_identical():
    import torch
    from xiangqi_alphazero_amd import engine, hip
    ev = _TorchStub()
    n_games, sims, inj_len = 12, 24, 8192
    cfg = engine.make_config(n_games, sims, games_target=n_games, max_game_length=40, inject_len=inj_len)
    inject = _inject_array([100 + s for s in range(n_games)], inj_len)

    def run(how):
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, inject=inject)     # xq_engine_init
        base = (eng.ws.data_ptr() + 255) & ~255
        args = (base, eng.workspace_bytes, eng._inject.data_ptr(), hip.stream_ptr(eng.device))
        if how == "init_fp":
            hip.check(eng.lib.xq_engine_init_fp(C.byref(eng.h), C.byref(cfg), 1, 0, None, None, *args), "xq_engine_init_fp")
        elif how == "init_gz":
            assert eng.lib.xq_engine_workspace_bytes_gz(C.byref(cfg), 1, 0, None, None, None) == eng.workspace_bytes
            hip.check(eng.lib.xq_engine_init_gz(C.byref(eng.h), C.byref(cfg), 1, 0, None, None, None, *args), "xq_engine_init_gz")
        torch.cuda.synchronize()
        st = _run(eng, n_games, False, sims)
        assert st["gumbel_moves"] == st["gumbel_considered"] == st["gumbel_offprior"] == 0
        sha, smp, res = _records_sha(eng)
        assert len(smp) > 0 and len(res) == n_games and (smp["reserved0"] == 0).all()
        return sha

    want = run("init")
    assert run("init_fp") == want and run("init_gz") == want
