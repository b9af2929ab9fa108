"""Forced playouts and policy target pruning on the GPU (k_select<.., .., true>, xq_engine_init_fp).

* whole games with injected draws equal the host model (tests/forced_playouts_model.py) record for record: board, actions, PRUNED
  visits, z, winner, plies and the counters sims, fast_moves, fast_sims, reused_visits, reroots, forced_sims, pruned_visits,
  pruned_children -- the four recorded configurations and a longer peaked game, k = 2, tree reuse off and on, the playout cap
  off and on (p = 0.5, S_fast = S / 4);
* k = 2**-40 (k S < 1: nothing is ever forced or subtracted): drained samples and results byte-identical to engines built by
  xq_engine_init_cap, and by xq_engine_init where neither cap nor reuse is set, eager and replayed from a graph;
* forced playouts with the evaluation cache equal forced playouts alone;
* run_games with the hand-written evaluator on peaked weights, device RNG, run to completion: no overflow, forced simulations
  happened, the samples' visits sum to S * (full moves) - pruned_visits, and with the cap samples = moves - fast_moves.
"""
import ctypes as C
import types

import numpy as np
import pytest

import forced_playouts_model as FP
import golden_io as G
from oracle import xq_oracle as O
from test_playout_cap_gpu import _assert_game, _engine_cfg, _inject_array, _play_stub, _records_sha, _run
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -40
_LONG = dict(num_simulations=100, c_puct=1.5, temperature_threshold=10, max_game_length=70, random_opening_moves=4,
             enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
GAMES = [(t["cfg"], t["stub"] == "peaked", t["seed"], t["name"]) for t in G.game_traces()] + [(_LONG, True, 31, "long_peaked")]
COUNTERS = ("sims", "fast_moves", "fast_sims", "reused_visits", "reroots", "forced_sims", "pruned_visits", "pruned_children")


@pytest.mark.parametrize("capped", [False, True], ids=["nocap", "cap"])
@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
@pytest.mark.parametrize("game", GAMES, ids=[g[3] for g in GAMES])
def test_games_equal_host_model(game, reuse, capped):
    from xiangqi_alphazero_amd import engine
    c, peaked, seed, _ = game
    S = int(c["num_simulations"])
    cap = (0.5, max(1, S // 4)) if capped else None
    want, winner, plies, mst = FP.play_game(c, peaked, seed, tree_reuse=reuse, cap=cap, forced=2.0)
    # the condition: the game exercises forcing, pruning and outright removal, or the comparison proves nothing
    assert mst["forced_sims"] > 0 and mst["pruned_visits"] > 0 and mst["pruned_children"] > 0
    assert sum(int(w["visits"].sum()) for w in want) == S * mst["full_moves"] - mst["pruned_visits"]
    if capped:
        assert mst["fast_moves"] > 0
    n_slots, inj_len = 2, 16384
    eng = engine.SelfPlayEngine(_engine_cfg(engine, c, n_slots, inj_len, n_slots), inject=_inject_array([seed] * n_slots, inj_len),
                                tree_reuse=reuse, playout_cap=cap, forced_playouts=2.0)
    assert eng.forced_playouts == 2.0 and eng.playout_cap == cap
    st = _play_stub(eng, peaked, n_slots)
    samples, results = eng.drain()
    assert len(results) == n_slots
    for r in results:
        assert (int(r["winner"]), int(r["steps"]), int(r["n_samples"])) == (winner, plies, len(want))
    for slot in range(n_slots):
        _assert_game(samples[samples["slot"] == slot], want)
    print({k: st[k] for k in COUNTERS})
    assert tuple(st[k] for k in COUNTERS) == tuple(n_slots * mst[k] for k in COUNTERS)
    assert st["samples_written"] == n_slots * len(want) and st["moves_played"] == n_slots * len(mst["moves"])


def test_tiny_k_is_byte_identical_to_engines_without_the_option():
    import torch
    from xiangqi_alphazero_amd import engine, hip
    ev = _TorchStub()
    n_games, sims, inj_len = 12, 24, 8192
    assert TINY * sims < 1
    cfg = engine.make_config(n_games, sims, games_target=n_games, max_game_length=40, inject_len=inj_len)
    inject = _inject_array([100 + s for s in range(n_games)], inj_len)

    def off(reuse, cap, how):
        """how = 'init': the engine as SelfPlayEngine builds it (xq_engine_init when neither cap nor reuse is set);
        'init_cap': the same engine initialised again through xq_engine_init_cap."""
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, inject=inject, tree_reuse=reuse, playout_cap=cap)
        if how == "init_cap":
            base = (eng.ws.data_ptr() + 255) & ~255
            cs = None if cap is None else hip.PlayoutCap(cap[1], 0, cap[0])
            hip.check(eng.lib.xq_engine_init_cap(C.byref(eng.h), C.byref(cfg), 1, hip.ENGINE_TREE_REUSE if reuse else 0,
                                                 None if cs is None else C.byref(cs), base, eng.workspace_bytes,
                                                 eng._inject.data_ptr(), hip.stream_ptr(eng.device)), "xq_engine_init_cap")
            torch.cuda.synchronize()
        st = _run(eng, n_games, False, sims)
        return st, _records_sha(eng)

    def on(reuse, cap, graph):
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, inject=inject, tree_reuse=reuse, playout_cap=cap, forced_playouts=TINY)
        st = _run(eng, n_games, graph, sims)
        assert st["forced_sims"] == st["pruned_visits"] == st["pruned_children"] == 0
        return st, _records_sha(eng)

    keys = ("sims", "moves_played", "samples_written", "reused_visits", "reroots", "fast_moves", "fast_sims", "games_finished")
    for reuse in (False, True):
        for cap in (None, (0.5, 6)):
            st_off, (sha_off, smp, res) = off(reuse, cap, "init_cap")
            assert len(smp) > 0 and len(res) == n_games
            if not reuse and cap is None:
                assert off(False, None, "init")[1][0] == sha_off
            if reuse:
                assert st_off["reroots"] > 0
            if cap is not None:
                assert st_off["fast_moves"] > 0
            for graph in (False, True):
                st, (sha, _, _) = on(reuse, cap, graph)
                assert sha == sha_off, (reuse, cap, graph)
                assert all(st[k] == st_off[k] for k in keys), (reuse, cap, graph)


def _selfplay_forced(ev, reuse, cache_entries, cap=None, n_games=16, sims=24, seed=3):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(n_games, sims, seed=seed, games_target=n_games, max_game_length=40)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, tree_reuse=reuse, eval_cache_entries=cache_entries, playout_cap=cap,
                                forced_playouts=2.0)
    st = _run(eng, n_games, True, sims)
    sha, smp, res = _records_sha(eng)
    assert all(0 < int(s["visits"][:s["n_moves"]].sum()) <= sims for s in smp)
    assert st["samples_written"] == len(smp) == int(res["n_samples"].sum()) == st["moves_played"] - st["fast_moves"]
    assert int(sum(int(s["visits"][:s["n_moves"]].sum()) for s in smp)) == sims * len(smp) - st["pruned_visits"]
    return st, sha


@pytest.mark.parametrize("capped", [False, True], ids=["nocap", "cap"])
@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
def test_forced_with_eval_cache_equals_forced_alone(reuse, capped):
    _, ev = _hip_evaluator()
    cap = (0.5, 6) if capped else None
    st, sha = _selfplay_forced(ev, reuse, 0, cap)
    st_c, sha_c = _selfplay_forced(ev, reuse, 64, cap)
    assert sha_c == sha and st_c["eval_cache_hits"] > 0 and st["forced_sims"] > 0
    assert all(st_c[k] == st[k] for k in COUNTERS + ("moves_played", "samples_written"))


@pytest.mark.parametrize("capped", [False, True], ids=["nocap", "cap"])
@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
def test_run_games_counts_add_up(reuse, capped):
    from xiangqi_alphazero_amd import selfplay
    S, S_fast, p, games = 32, 8, 0.5, 64
    net, _ = _hip_evaluator(policy_gain=8.0)           # peaked weights
    config = types.SimpleNamespace(num_simulations=S, c_puct=1.5, temperature_threshold=10, max_game_length=60,
                                   random_opening_moves=4, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
                                   forced_playouts_k=2.0)      # through the config key, as AlphaZeroLoop's self-play passes it
    if capped:
        config.playout_cap_full_prob, config.playout_cap_fast_simulations = p, S_fast
    samples, results, st, _ = selfplay.run_games(net, config, games, seed=7, tree_reuse=reuse)
    assert st["overflow"] == 0 and len(results) == games == st["games_finished"]
    assert st["forced_playouts"] == 2.0 and st["forced_sims"] > 0
    full = st["moves_played"] - st["fast_moves"]
    assert st["samples_written"] == len(samples) == int(results["n_samples"].sum()) == full
    if not capped:
        assert st["fast_moves"] == 0
    total = kept = 0
    for s in samples:
        n = int(s["n_moves"])
        v = s["visits"][:n].astype(np.int64)
        assert 0 < int(v.sum()) <= S
        total += int(v.sum())
        kept += int((v > 0).sum())
        np.testing.assert_array_equal(s["actions"][:n], O.legal_actions(s["board"], int(s["side"])))
    assert total == S * full - st["pruned_visits"]
    if not reuse:
        assert st["sims"] == S * full + S_fast * st["fast_moves"] and st["reused_visits"] == 0
    print("full moves", full, "forced_sims", st["forced_sims"], "pruned visit share", st["pruned_visits"] / (S * full),
          "pruned share of visited children", st["pruned_children"] / max(1, kept + st["pruned_children"]))
