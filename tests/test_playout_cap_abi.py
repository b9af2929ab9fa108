"""CPU checks of the playout-cap ABI (include/xq_hip.h, xq_engine_init_cap): exports, unchanged struct sizes, the workspace, and
the argument errors returned before any launch, in C and in Python."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_cap", "xq_engine_init_cap")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    for d in ("XQ_STAT_FAST_MOVES 5", "XQ_STAT_FAST_SIMS 6"):
        assert "#define " + d in header
    assert "typedef struct xq_playout_cap { int32_t fast_simulations; int32_t reserved; double full_search_prob; }" in header
    assert "uint64_t reserved[13];" in header


def test_struct_sizes():
    hip, _ = _lib()
    assert C.sizeof(hip.PlayoutCap) == 16 and hip.PlayoutCap.full_search_prob.offset == 8
    assert C.sizeof(hip.EngineConfig) == 112
    assert C.sizeof(hip.Engine) == 384
    assert C.sizeof(hip.EngineStats) == 32 * 8
    names = [f[0] for f in hip.EngineStats._fields_]
    assert names.index("fast_moves") == 19 + 5 and names.index("fast_sims") == 19 + 6
    assert names.index("reused_visits") == 19 + 3 and names.index("reroots") == 19 + 4
    assert {"fast_moves", "fast_sims"} <= set(hip.EngineStats().as_dict())


def test_workspace_bytes_cap():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(64, 100)
    cap = hip.PlayoutCap(25, 0, 0.25)
    for flags in (0, 1):
        for K in (1, 4):
            want = lib.xq_engine_workspace_bytes_ex(C.byref(cfg), K, flags)
            assert lib.xq_engine_workspace_bytes_cap(C.byref(cfg), K, flags, None) == want
    for flags in (0, 1):                               # a valid cap adds no workspace
        want = lib.xq_engine_workspace_bytes_ex(C.byref(cfg), 1, flags)
        assert want > 0 and lib.xq_engine_workspace_bytes_cap(C.byref(cfg), 1, flags, C.byref(cap)) == want
    assert lib.xq_engine_workspace_bytes_cap(C.byref(cfg), 1, 0, C.byref(hip.PlayoutCap(99, 0, 1.0))) > 0


def _bad_cases(hip, engine):
    ok = engine.make_config(8, 50)
    good = hip.PlayoutCap(10, 0, 0.25)
    return [("S_fast = 0", ok, 1, 0, hip.PlayoutCap(0, 0, 0.25)),
            ("S_fast = S", ok, 1, 0, hip.PlayoutCap(50, 0, 0.25)),
            ("S_fast < 0", ok, 1, 0, hip.PlayoutCap(-3, 0, 0.25)),
            ("p = 0", ok, 1, 0, hip.PlayoutCap(10, 0, 0.0)),
            ("p > 1", ok, 1, 0, hip.PlayoutCap(10, 0, float(np.nextafter(1.0, 2.0)))),
            ("p NaN", ok, 1, 0, hip.PlayoutCap(10, 0, float("nan"))),
            ("p < 0", ok, 1, 0, hip.PlayoutCap(10, 0, -0.5)),
            ("reserved = 1", ok, 1, 0, hip.PlayoutCap(10, 1, 0.25)),
            ("manual_moves 1", engine.make_config(8, 50, manual_moves=1), 1, 0, good),
            ("manual_moves 2", engine.make_config(8, 50, manual_moves=2), 1, 0, good),
            ("K = 2", ok, 2, 0, good),
            ("unknown flags 2", ok, 1, 2, good),
            ("unknown flags 6", ok, 1, 6, good),
            ("K = 2 with reuse", ok, 2, 1, good)]


def test_cap_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    for what, cfg, K, flags, cap in _bad_cases(hip, engine):
        assert lib.xq_engine_workspace_bytes_cap(C.byref(cfg), K, flags, C.byref(cap)) == 0, what
        assert lib.xq_engine_init_cap(C.byref(h), C.byref(cfg), K, flags, C.byref(cap), fake_ws, 1 << 40, None, None) == -1, what
    # cap == NULL is xq_engine_init_ex: the same refusals
    for cfg, K, flags in ((engine.make_config(8, 50), 1, 2), (engine.make_config(8, 50), 2, 1), (engine.make_config(8, 50), 0, 0)):
        assert lib.xq_engine_init_cap(C.byref(h), C.byref(cfg), K, flags, None, fake_ws, 1 << 40, None, None) == -1


def test_python_rejects_unsupported_combinations():
    from xiangqi_alphazero_amd import engine, hip
    for manual in (1, 2):
        with pytest.raises(hip.XqError, match="playout_cap"):
            engine.SelfPlayEngine(engine.make_config(4, 16, manual_moves=manual), "cpu", playout_cap=(0.25, 4))
    cfg = engine.make_config(4, 16)
    with pytest.raises(hip.XqError, match="playout_cap"):
        engine.SelfPlayEngine(cfg, "cpu", playout_cap=(0.25, 4), leaves_per_step=2)
    for bad in ((0.25, 0), (0.25, 16), (0.0, 4), (1.5, 4), (float("nan"), 4), (0.25,), "x"):
        with pytest.raises(hip.XqError, match="playout_cap"):
            engine.SelfPlayEngine(cfg, "cpu", playout_cap=bad)


def test_consumers_accept_a_game_without_samples():
    """A capped game may record no sample: the dense adapter and the replay buffer take an empty sample array."""
    from xiangqi_alphazero_amd import sample_format as F, training
    samples = np.zeros(0, dtype=F.SAMPLE_DTYPE)
    results = np.zeros(1, dtype=F.RESULT_DTYPE)
    results[0]["winner"], results[0]["steps"] = 1, 37
    all_data, per_game = F.to_reference_tuples(samples, results)
    assert all_data == [] and per_game == [(1, 37, 0)]
    buf = training.ReplayBuffer(64, "cpu")
    buf.extend(samples)
    assert len(buf) == 0
