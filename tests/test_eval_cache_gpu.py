"""The evaluation cache on the GPU (engine.SelfPlayEngine(eval_cache_entries=K), xq_evcache_*): a cached row is the row the
network would have computed, so cache-on games are byte-identical to cache-off games -- eager and graph-replayed, through
run_games and parallel_self_play -- while the network runs on fewer rows; evictions and weight updates change nothing."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, SIMS, PLIES, K = 128, 64, 60, 128       # K = recommended_cache_entries(64)


def _config(**kw):
    c = types.SimpleNamespace(num_simulations=SIMS, c_puct=1.5, temperature_threshold=15, max_game_length=PLIES,
                              random_opening_moves=4, enable_resign=True, resign_threshold=-0.85, resign_check_steps=3,
                              num_games_per_iter=G)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _net(gain, seed=0):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(64, 2)
    net.load_state_dict(weights.make_state_dict(64, 2, seed=seed, policy_gain=gain))
    return net


CACHE_KEYS = ("eval_cache_probes", "eval_cache_hits", "eval_cache_inserts", "eval_cache_evictions", "eval_cache_mismatches",
              "eval_cache_entries", "eval_cache_bytes")


def _records(smp, res):
    """The rings fill in the order slots finish within a step, which is not fixed: compare the records sorted."""
    return np.sort(smp, order=["slot", "game_seq", "ply"]).tobytes(), np.sort(res, order=["slot", "game_seq"]).tobytes()


def _engine_stats(st):
    """The engine's counters; what the step ran on (path, launch mode, the polled step count) is left out."""
    return {k: v for k, v in st.items() if k not in CACHE_KEYS and k not in ("rows_evaluated", "path", "launch", "steps")}


def _run(net, entries, graph):
    from xiangqi_alphazero_amd import selfplay
    smp, res, st, _ = selfplay.run_games(net, _config(), G, "cuda", seed=3, use_graph=graph, eval_cache_entries=entries)
    assert st["launch"] == ("graph" if graph else "eager")
    assert st["path"] == ("cached" if entries else "packed")
    return smp, res, st


@pytest.mark.parametrize("gain,min_hit", [(1.0, 0.05), (8.0, 0.15)], ids=["random", "peaked"])
def test_cached_games_identical_through_run_games(gain, min_hit):
    net = _net(gain)
    s0, r0, st0 = _run(net, 0, True)
    assert "eval_cache_mismatches" not in st0 and st0["eval_cache_hits"] == 0
    runs = [_run(net, K, graph) for graph in (False, True)]
    for smp, res, st in runs:
        assert _records(smp, res) == _records(s0, r0)
        assert _engine_stats(st) == _engine_stats(st0)
        assert st["eval_cache_mismatches"] == 0
        assert st["eval_cache_probes"] == st0["rows_evaluated"]                       # every waiting slot is probed
        assert st0["rows_evaluated"] == st["rows_evaluated"] + st["eval_cache_hits"]  # hits are rows the network skipped
        assert st["eval_cache_inserts"] == st["rows_evaluated"]
        rate = st["eval_cache_hits"] / st["eval_cache_probes"]
        assert rate > min_hit, f"hit rate {rate:.3f}"
    # determinism: the eager and the replayed cache-on run count the same
    assert {k: runs[0][2][k] for k in CACHE_KEYS} == {k: runs[1][2][k] for k in CACHE_KEYS}
    print(f"gain {gain}: hit rate {runs[0][2]['eval_cache_hits'] / runs[0][2]['eval_cache_probes']:.3f}, rows "
          f"{st0['rows_evaluated']} -> {runs[0][2]['rows_evaluated']}")


def test_parallel_self_play_takes_the_config_key():
    from xiangqi_alphazero_amd import selfplay
    net = _net(8.0, seed=1)
    d0, st0 = selfplay.parallel_self_play(net, _config(), seed=2, return_compact=True)
    d1, st1 = selfplay.parallel_self_play(net, _config(eval_cache_entries=K), seed=2, return_compact=True)
    assert st0["path"] == "packed" and st1["path"] == "cached"
    assert _records(st0["compact_samples"], st0["compact_results"]) == _records(st1["compact_samples"], st1["compact_results"])
    flat = lambda d: sorted(a.tobytes() + p.tobytes() + np.float64(z).tobytes() for a, p, z in d)
    assert len(d0) == len(d1) > 0 and flat(d0) == flat(d1)
    assert st0["eval_cache_hits"] == 0 and st1["eval_cache_hits"] > 0
    assert st0["rows_evaluated"] == st1["rows_evaluated"] + st1["eval_cache_hits"]
    skip = ("total_time", "rows_evaluated", "eval_cache_hits", "eval_cache_probes", "path", "compact_samples", "compact_results")
    assert {k: v for k, v in st0.items() if k not in skip} == {k: v for k, v in st1.items() if k not in skip}


def test_small_table_evicts_and_still_plays_the_same_games():
    net = _net(8.0)
    s0, r0, st0 = _run(net, 0, True)
    s1, r1, st1 = _run(net, 4, True)
    assert st1["eval_cache_evictions"] > 0 and st1["eval_cache_mismatches"] == 0
    assert _records(s1, r1) == _records(s0, r0)
    assert _engine_stats(st1) == _engine_stats(st0)
    assert st0["rows_evaluated"] == st1["rows_evaluated"] + st1["eval_cache_hits"]


def _engine(ev, entries, plies=PLIES):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(G, SIMS, max_game_length=plies, seed=11)
    return engine.SelfPlayEngine(cfg, "cuda", evaluator=ev, eval_cache_entries=entries)


def _state(eng):
    import torch
    torch.cuda.synchronize()
    v = eng.arena_views()
    mark = eng.slot_ints[:, 7].cpu().numpy()                     # allocation mark: nodes past it are not the engine's state
    out = {"ints": eng.slot_ints.cpu().numpy().tobytes(), "board": v["board"].cpu().numpy().tobytes()}
    for name in ("N", "W", "P", "action", "first", "meta"):
        a = v[name].cpu().numpy()
        out[name] = b"".join(a[s, :max(int(mark[s]), 1)].tobytes() for s in range(G))
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_weight_update_invalidates(graph):
    """Net A for a while, update() to net B, step on: every engine state, sample and result equals a cache-off engine on
    the same schedule, and the first step after the update is answered by the network alone."""
    from xiangqi_alphazero_amd import evaluator
    net_a, net_b = _net(8.0, seed=0), _net(8.0, seed=5)
    ev_on, _ = evaluator.make_evaluator(net_a, "cuda", "hip")
    ev_off, _ = evaluator.make_evaluator(net_a, "cuda", "hip")
    on, off = _engine(ev_on, K, 16), _engine(ev_off, 0, 16)          # 16 plies: games finish within the schedule
    assert on.path == "cached" and off.path == "packed"
    if graph:
        assert on.capture_step() and off.capture_step()
    for _ in range(300):
        on.step()
        off.step()
    hits_before = on.stats()["eval_cache_hits"]
    assert hits_before > 0
    version = ev_on.weights_version
    ev_on.update(net_b)
    ev_off.update(net_b)
    assert ev_on.weights_version == version + 1
    on.step()
    off.step()
    assert on.stats()["eval_cache_hits"] == hits_before, "a stale entry answered after the weight update"
    for _ in range(1200):
        on.step()
        off.step()
    assert on.launch_mode == off.launch_mode == ("graph" if graph else "eager")
    assert _state(on) == _state(off)
    so, sf = on.stats(), off.stats()
    assert so["eval_cache_hits"] > hits_before and so["eval_cache_mismatches"] == 0
    assert _engine_stats(so) == _engine_stats(sf)
    assert sf["rows_evaluated"] == so["rows_evaluated"] + so["eval_cache_hits"]
    (s1, r1), (s0, r0) = on.drain(), off.drain()
    assert len(s0) > 0 and _records(s1, r1) == _records(s0, r0)


def test_cache_needs_a_live_rows_evaluator_and_a_power_of_two():
    from xiangqi_alphazero_amd import evaluator, hip
    ev, _ = evaluator.make_evaluator(_net(1.0), "cuda", "hip")

    class NoLiveRows:
        def __init__(self, inner):
            self.inner = inner

        def evaluate_legal(self, x, moves, counts):
            return self.inner.evaluate_legal(x, moves, counts)

    with pytest.raises(hip.XqError):
        _engine(NoLiveRows(ev), K)
    with pytest.raises(hip.XqError):
        _engine(ev, 6)
    eng = _engine(ev, 0)
    assert eng.path == "packed" and not any(k.startswith("eval_cache") for k in eng.stats())
