"""CPU checks of the Gumbel root search's ABI (include/xq_hip.h, xq_engine_init_gz): exports, header text, unchanged struct sizes,
the new statistics indices, gumbel == NULL being xq_engine_init_fp, the considered-visit table of the library against the host
model's, the workspace (only Gumbel engines grow), and every refusal, returned before any launch, in C and in Python."""
import ctypes as C
import os

import numpy as np
import pytest

import gumbel_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_gz", "xq_engine_init_gz", "xq_gumbel_considered_visits_host")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    for d in ("XQ_STAT_GUMBEL_MOVES 10", "XQ_STAT_GUMBEL_CONSIDERED 11", "XQ_STAT_GUMBEL_OFFPRIOR 12"):
        assert "#define " + d in header
    assert ("typedef struct xq_gumbel { int32_t considered; int32_t reserved; double c_visit; double c_scale; } xq_gumbel;"
            in header)
    # what earlier options pinned stays
    assert "uint64_t reserved[13];" in header
    assert "typedef struct xq_forced_playouts { double k; uint32_t reserved[2]; } xq_forced_playouts;" in header
    for d in ("XQ_STAT_FORCED_SIMS 7", "XQ_STAT_PRUNED_VISITS 8", "XQ_STAT_PRUNED_CHILDREN 9"):
        assert "#define " + d in header
    # the rules are written down where the host model is written from
    for phrase in ("l_i = log((double)max(tP[i], FLT_MIN))", "g = -log(-log(u)), u = ((x >> 11) + 0.5) * 2^-53",
                   "((double)((x >> 40) % 4096) - 1024.0) / 512.0", "rootP[i] = g_i + l_i", "prior kind is 3",
                   "get_sequence_of_considered_visits", "children with N_i == cv",
                   "sigma(q) = ((c_visit + maxN) * c_scale) * ((q + 1) * 0.5)",
                   "v_mix = (v_hat + sumN * (sum_{N_b>0} tP[b] q_b / sum_{N_b>0} tP[b])) / (1 + sumN)",
                   "visits[i] = (uint16_t)floor(pi'_i * 65535 + 0.5)", "reserved0 = 1", "NO draw of the uniform stream"):
        assert phrase in header, phrase


def test_struct_sizes_and_stat_indices():
    hip, _ = _lib()
    assert C.sizeof(hip.Gumbel) == 24 and hip.Gumbel.considered.offset == 0 and hip.Gumbel.c_visit.offset == 8
    assert C.sizeof(hip.ForcedPlayouts) == 16 and C.sizeof(hip.PlayoutCap) == 16
    assert C.sizeof(hip.EngineConfig) == 112
    assert C.sizeof(hip.Engine) == 384
    assert C.sizeof(hip.EngineStats) == 32 * 8
    names = [f[0] for f in hip.EngineStats._fields_]
    assert names[-1] == "reserved" and hip.EngineStats.reserved.offset == 29 * 8 == (19 + 10) * 8
    assert names.index("pruned_children") == 28 and names.index("rows_evaluated") == 18
    s = hip.EngineStats()
    s.reserved[0], s.reserved[1], s.reserved[2] = 5, 60, 3
    d = s.as_dict()
    assert (d["gumbel_moves"], d["gumbel_considered"], d["gumbel_offprior"]) == (5, 60, 3) and "reserved" not in d


def test_gumbel_null_is_init_fp():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(64, 100)
    cap = hip.PlayoutCap(25, 0, 0.25)
    fp = hip.ForcedPlayouts(2.0)
    for flags in (0, 1):
        for K in (1, 4):
            want = lib.xq_engine_workspace_bytes_fp(C.byref(cfg), K, flags, None, None)
            assert (want > 0) == (not (flags and K > 1))   # tree reuse with K > 1 stays refused
            assert lib.xq_engine_workspace_bytes_gz(C.byref(cfg), K, flags, None, None, None) == want
        for cp, f in ((cap, None), (None, fp), (cap, fp)):
            cr, fr = (None if cp is None else C.byref(cp)), (None if f is None else C.byref(f))
            want = lib.xq_engine_workspace_bytes_fp(C.byref(cfg), 1, flags, cr, fr)
            assert want > 0 and lib.xq_engine_workspace_bytes_gz(C.byref(cfg), 1, flags, cr, fr, None) == want
    # the same refusals as xq_engine_init_fp, none lifted
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    ok = engine.make_config(8, 50)
    for cfg2, K, flags, cp, f in ((ok, 1, 2, None, None), (ok, 2, 1, None, None), (ok, 0, 0, None, None),
                                  (ok, 1, 0, hip.PlayoutCap(50, 0, 0.25), None), (ok, 1, 0, None, hip.ForcedPlayouts(17.0)),
                                  (engine.make_config(8, 50, manual_moves=2), 1, 0, cap, None)):
        cr, fr = (None if cp is None else C.byref(cp)), (None if f is None else C.byref(f))
        assert lib.xq_engine_workspace_bytes_gz(C.byref(cfg2), K, flags, cr, fr, None) == 0
        assert lib.xq_engine_init_fp(C.byref(h), C.byref(cfg2), K, flags, cr, fr, fake_ws, 1 << 40, None, None) == -1
        assert lib.xq_engine_init_gz(C.byref(h), C.byref(cfg2), K, flags, cr, fr, None, fake_ws, 1 << 40, None, None) == -1


@pytest.mark.parametrize("S", [1, 8, 24, 100, 200, 800])
def test_library_table_equals_the_model(S):
    _, lib = _lib()
    out = np.zeros(S, dtype=np.uint16)
    for k in range(1, 129):
        assert lib.xq_gumbel_considered_visits_host(k, S, out.ctypes.data) == 0
        assert out.tolist() == GM.considered_visits(k, S), k
    for k, s in ((0, S), (129, S), (4, 0), (4, 65536)):
        assert lib.xq_gumbel_considered_visits_host(k, s, out.ctypes.data) == -1
    assert lib.xq_gumbel_considered_visits_host(4, S, None) == -1


def test_only_gumbel_engines_grow():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    for G_, S in ((64, 100), (1024, 32), (3, 7)):
        for manual in (0, 1):
            cfg = engine.make_config(G_, S, manual_moves=manual)
            plain = lib.xq_engine_workspace_bytes(C.byref(cfg))
            assert plain > 0 and lib.xq_engine_workspace_bytes_gz(C.byref(cfg), 1, 0, None, None, None) == plain
            for m in (1, 16, 128):
                gz = hip.Gumbel(m, 0, 50.0, 1.0)
                got = lib.xq_engine_workspace_bytes_gz(C.byref(cfg), 1, 0, None, None, C.byref(gz))
                extra = 16 + 8 * G_ + 2 * m * S        # the parameters, one double per slot, m tables of S uint16
                assert got >= plain and abs(got - (plain + extra)) < 256, (G_, S, m)     # regions are 256-byte aligned


def _bad_cases(hip, engine):
    ok = engine.make_config(8, 50)
    good = hip.Gumbel(16, 0, 50.0, 1.0)
    inf, nan = float("inf"), float("nan")
    return [("manual_moves 2", engine.make_config(8, 50, manual_moves=2), 1, 0, None, None, good),
            ("tree reuse", ok, 1, 1, None, None, good),
            ("playout cap", ok, 1, 0, hip.PlayoutCap(10, 0, 0.25), None, good),
            ("forced playouts", ok, 1, 0, None, hip.ForcedPlayouts(2.0), good),
            ("K = 2", ok, 2, 0, None, None, good),
            ("m = 0", ok, 1, 0, None, None, hip.Gumbel(0, 0, 50.0, 1.0)),
            ("m < 0", ok, 1, 0, None, None, hip.Gumbel(-4, 0, 50.0, 1.0)),
            ("m = 129", ok, 1, 0, None, None, hip.Gumbel(129, 0, 50.0, 1.0)),
            ("c_visit < 0", ok, 1, 0, None, None, hip.Gumbel(16, 0, -1.0, 1.0)),
            ("c_visit NaN", ok, 1, 0, None, None, hip.Gumbel(16, 0, nan, 1.0)),
            ("c_visit inf", ok, 1, 0, None, None, hip.Gumbel(16, 0, inf, 1.0)),
            ("c_visit beyond float32", ok, 1, 0, None, None, hip.Gumbel(16, 0, 1e39, 1.0)),
            ("c_scale 0", ok, 1, 0, None, None, hip.Gumbel(16, 0, 50.0, 0.0)),
            ("c_scale < 0", ok, 1, 0, None, None, hip.Gumbel(16, 0, 50.0, -1.0)),
            ("c_scale NaN", ok, 1, 0, None, None, hip.Gumbel(16, 0, 50.0, nan)),
            ("c_scale inf", ok, 1, 0, None, None, hip.Gumbel(16, 0, 50.0, inf)),
            ("reserved", ok, 1, 0, None, None, hip.Gumbel(16, 1, 50.0, 1.0)),
            ("unknown flags 2", ok, 1, 2, None, None, good)]


def test_gz_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    for what, cfg, K, flags, cap, fp, gz in _bad_cases(hip, engine):
        cr, fr = (None if cap is None else C.byref(cap)), (None if fp is None else C.byref(fp))
        assert lib.xq_engine_workspace_bytes_gz(C.byref(cfg), K, flags, cr, fr, C.byref(gz)) == 0, what
        assert lib.xq_engine_init_gz(C.byref(h), C.byref(cfg), K, flags, cr, fr, C.byref(gz), fake_ws, 1 << 40, None, None) == -1, what
    # allowed: search only, no root noise, the boundaries of m, c_visit = 0
    for cfg in (engine.make_config(8, 50), engine.make_config(8, 50, manual_moves=1), engine.make_config(8, 50, add_noise=False)):
        for gz in (hip.Gumbel(1, 0, 0.0, 1.0), hip.Gumbel(128, 0, 50.0, 0.1)):
            assert lib.xq_engine_workspace_bytes_gz(C.byref(cfg), 1, 0, None, None, C.byref(gz)) > 0


def test_python_rejects_unsupported_combinations():
    from xiangqi_alphazero_amd import engine, hip
    good = (16, 50.0, 1.0)
    with pytest.raises(hip.XqError, match="gumbel"):
        engine.SelfPlayEngine(engine.make_config(4, 16, manual_moves=2), "cpu", gumbel=good)
    cfg = engine.make_config(4, 16)
    for kw in (dict(tree_reuse=True), dict(playout_cap=(0.5, 4)), dict(forced_playouts=2.0), dict(leaves_per_step=2)):
        with pytest.raises(hip.XqError, match="gumbel"):
            engine.SelfPlayEngine(cfg, "cpu", gumbel=good, **kw)
    nan, inf = float("nan"), float("inf")
    for bad in ((0, 50.0, 1.0), (129, 50.0, 1.0), (-1, 50.0, 1.0), (16, -1.0, 1.0), (16, nan, 1.0), (16, inf, 1.0), (16, 1e39, 1.0),
                (16, 50.0, 0.0), (16, 50.0, -2.0), (16, 50.0, nan), (16, 50.0, inf), (16, 50.0), 16, "x", (2.5, 50.0, 1.0)):
        with pytest.raises(hip.XqError, match="gumbel"):
            engine.SelfPlayEngine(cfg, "cpu", gumbel=bad)
    # a valid option on a machine without a GPU gets as far as the product path's own refusal
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(hip.XqError, match="GPU"):
            engine.SelfPlayEngine(engine.make_config(4, 16, manual_moves=1), "cpu", gumbel=good)


def test_run_games_reads_the_config_keys():
    """Absent or 0 means off, so a reference TrainingConfig works; the arena never passes the option."""
    import inspect
    from xiangqi_alphazero_amd import arena, selfplay, train_loop
    src = inspect.getsource(selfplay.run_games)
    for key in ("gumbel_considered", "gumbel_c_visit", "gumbel_c_scale"):
        assert key in src
    assert "gumbel" in inspect.signature(selfplay.run_games).parameters
    assert "gumbel" in inspect.signature(selfplay.parallel_self_play).parameters
    assert "gumbel" in inspect.signature(engine_init()).parameters
    assert "gumbel" in inspect.getsource(train_loop.AlphaZeroLoop._play_shard)
    assert "gumbel" not in inspect.getsource(arena)


def engine_init():
    from xiangqi_alphazero_amd import engine
    return engine.SelfPlayEngine.__init__
