"""CPU checks of the leaf-batching ABI (include/xq_hip.h, xq_engine_init_leaves): exports, unchanged struct sizes, and the
argument errors that are returned before any launch."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in ("xq_engine_workspace_bytes_leaves", "xq_engine_init_leaves"):
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)


def test_struct_sizes_unchanged():
    hip, _ = _lib()
    assert C.sizeof(hip.EngineConfig) == 112           # the header's layouts before leaf batching
    assert C.sizeof(hip.Engine) == 112 + 16 + 32 * 8
    assert C.sizeof(hip.EngineStats) == 32 * 8
    names = [f[0] for f in hip.EngineStats._fields_]
    assert names.index("collisions") == 19 and names.index("leaves_per_step_sum") == 20


def test_workspace_bytes_leaves():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(64, 100, manual_moves=1)
    base = lib.xq_engine_workspace_bytes(C.byref(cfg))
    assert lib.xq_engine_workspace_bytes_leaves(C.byref(cfg), 1) == base
    k8 = lib.xq_engine_workspace_bytes_leaves(C.byref(cfg), 8)
    nodes = 64 * (1 + 101 * 128)
    assert k8 > base + nodes * 4                       # virtual-loss counters and 8x the request rows
    for bad in (0, -1, 65):
        assert lib.xq_engine_workspace_bytes_leaves(C.byref(cfg), bad) == 0
    arena = engine.make_config(8, 100, manual_moves=2)
    assert lib.xq_engine_workspace_bytes_leaves(C.byref(arena), 2) == 0
    assert lib.xq_engine_workspace_bytes_leaves(C.byref(arena), 1) > 0


def test_init_leaves_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    cfg = engine.make_config(8, 50, manual_moves=1)
    for bad in (0, 65, -3):
        assert lib.xq_engine_init_leaves(C.byref(h), C.byref(cfg), bad, fake_ws, 1 << 40, None, None) == -1
    arena = engine.make_config(8, 50, manual_moves=2)
    assert lib.xq_engine_init_leaves(C.byref(h), C.byref(arena), 4, fake_ws, 1 << 40, None, None) == -1


def test_eval_cache_entry_points_reject_leaf_batching_engines():
    hip, lib = _lib()
    h = hip.Engine()
    h.cfg.n_games = 4
    h.pad0 = 4                                         # K = 4, as xq_engine_init_leaves records it
    cache = hip.EvCache()
    cache.n_slots, cache.entries, cache.ways, cache.sets = 4, 8, 4, 2
    for i in range(16):
        cache.p[i] = 4096 * (i + 1)                    # never dereferenced
    x = C.c_void_p(1 << 20)
    assert lib.xq_evcache_probe(C.byref(cache), C.byref(h), x, None) == -1
    assert lib.xq_engine_compact_misses(C.byref(h), x, x, None) == -1
    assert lib.xq_evcache_commit(C.byref(cache), C.byref(h), x, x, None) == -1


def test_python_rejects_unsupported_combinations():
    from xiangqi_alphazero_amd import engine, hip, mcts
    cfg = engine.make_config(4, 16)
    with pytest.raises(hip.XqError, match="evaluation cache"):
        engine.SelfPlayEngine(cfg, "cpu", leaves_per_step=2, eval_cache_entries=64)
    with pytest.raises(hip.XqError, match="arena"):
        engine.SelfPlayEngine(engine.make_config(4, 16, manual_moves=2), "cpu", leaves_per_step=2)
    for bad in (0, 65):
        with pytest.raises(hip.XqError, match="leaves_per_step"):
            engine.SelfPlayEngine(cfg, "cpu", leaves_per_step=bad)
        with pytest.raises(hip.XqError, match="leaves_per_step"):
            mcts.MCTS(lambda x: x, leaves_per_step=bad)
