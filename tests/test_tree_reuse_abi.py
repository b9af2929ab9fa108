"""CPU checks of the tree-reuse ABI (include/xq_hip.h, xq_engine_init_ex with XQ_ENGINE_TREE_REUSE): exports, the workspace of
every flag combination, and the argument errors returned before any launch, in C and in Python."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_ex", "xq_engine_init_ex", "xq_engine_drop_reroots")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    for d in ("XQ_ENGINE_TREE_REUSE 1u", "XQ_REUSE_MAX_SIMS 1600", "XQ_STAT_REUSED_VISITS 3", "XQ_STAT_REROOTS 4"):
        assert "#define " + d in header
    assert hip.ENGINE_TREE_REUSE == 1 and hip.REUSE_MAX_SIMS == 1600
    names = [f[0] for f in hip.EngineStats._fields_]
    assert names.index("reused_visits") == 19 + 3 and names.index("reroots") == 19 + 4
    assert C.sizeof(hip.EngineStats) == 32 * 8


def test_workspace_bytes_ex():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    R = hip.ENGINE_TREE_REUSE
    cfg = engine.make_config(64, 100)
    base = lib.xq_engine_workspace_bytes(C.byref(cfg))
    assert lib.xq_engine_workspace_bytes_ex(C.byref(cfg), 1, 0) == base
    assert lib.xq_engine_workspace_bytes_ex(C.byref(cfg), 1, R) == base          # tree reuse needs no workspace of its own
    assert lib.xq_engine_workspace_bytes_ex(C.byref(cfg), 4, 0) == lib.xq_engine_workspace_bytes_leaves(C.byref(cfg), 4)
    assert lib.xq_engine_workspace_bytes_ex(C.byref(cfg), 4, R) == 0             # leaf batching
    assert lib.xq_engine_workspace_bytes_ex(C.byref(cfg), 1, 2) == 0             # unknown flag
    for manual in (1, 2):
        assert lib.xq_engine_workspace_bytes_ex(C.byref(engine.make_config(8, 100, manual_moves=manual)), 1, R) == 0
    assert lib.xq_engine_workspace_bytes_ex(C.byref(engine.make_config(8, 1600)), 1, R) > 0
    assert lib.xq_engine_workspace_bytes_ex(C.byref(engine.make_config(8, 1601)), 1, R) == 0
    assert lib.xq_engine_workspace_bytes_ex(C.byref(engine.make_config(8, 1601)), 1, 0) > 0


def test_init_ex_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    R = hip.ENGINE_TREE_REUSE
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    bad = [(engine.make_config(8, 50, manual_moves=1), 1, R), (engine.make_config(8, 50, manual_moves=2), 1, R),
           (engine.make_config(8, 50), 2, R), (engine.make_config(8, 50), 1, 6), (engine.make_config(8, 1601), 1, R)]
    for cfg, K, flags in bad:
        assert lib.xq_engine_init_ex(C.byref(h), C.byref(cfg), K, flags, fake_ws, 1 << 40, None, None) == -1
    h.cfg.n_games = 4
    for pad0 in (0, 4):                                # K = 1 / K = 4 handles without the flag
        h.pad0 = pad0
        assert lib.xq_engine_drop_reroots(C.byref(h), None) == -1
    assert lib.xq_engine_drop_reroots(None, None) == -1


def test_python_rejects_unsupported_combinations():
    from xiangqi_alphazero_amd import engine, hip
    for manual in (1, 2):
        with pytest.raises(hip.XqError, match="tree_reuse"):
            engine.SelfPlayEngine(engine.make_config(4, 16, manual_moves=manual), "cpu", tree_reuse=True)
    with pytest.raises(hip.XqError, match="tree_reuse"):
        engine.SelfPlayEngine(engine.make_config(4, 16), "cpu", tree_reuse=True, leaves_per_step=2)
    with pytest.raises(hip.XqError, match="tree_reuse"):
        engine.SelfPlayEngine(engine.make_config(4, 1601), "cpu", tree_reuse=True)
