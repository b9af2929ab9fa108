"""CPU-side checks of the per-side resign rule (xq_engine_resign, xq_resign_scan_batch, xq_resign_exempt_host,
xq_resign_state_bytes; include/xq_hip.h): the exports, the refusals before any launch in C, the same
refusals as XqError from parse_resign / SelfPlayEngine, and the way of the option from the config keys to run_games and into the
iteration's "resign" entry (one rank: the gather over ranks cannot run here).  No GPU is needed by any of it."""
import ctypes as C
import inspect
import json
import math
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
NINF = float("-inf")


@pytest.fixture(scope="module")
def lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


def _fake_engine(manual_moves=0, n_games=8, enable_resign=1, threshold=NINF):
    from xiangqi_alphazero_amd import hip
    e = hip.Engine()
    e.cfg.n_games, e.cfg.num_simulations, e.cfg.manual_moves = n_games, 32, manual_moves
    e.cfg.enable_resign, e.cfg.resign_threshold, e.cfg.resign_check_steps = enable_resign, threshold, 5
    for i in range(32):
        e.p[i] = 0x200000 + 0x1000 * i                  # never dereferenced: every call below fails first
    return e


def _opts(threshold=-0.9, holdout_prob=0.1, check_steps=5, reserved=0):
    from xiangqi_alphazero_amd import hip
    return hip.ResignOpts(threshold, holdout_prob, check_steps, reserved)


def test_the_symbols_are_declared_exported_and_typed(lib):
    from xiangqi_alphazero_amd import hip, sample_format
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "int xq_engine_resign(const xq_engine *eng, const xq_resign_opts *opts, void *dev_state, xq_resign_row *dev_rows, int max_rows," in header
    assert "int xq_resign_scan_batch(const float *dev_values" in header
    assert "int xq_resign_exempt_host(uint64_t seed, int rank, int slot, uint32_t game_seq, double holdout_prob);" in header
    assert "size_t xq_resign_state_bytes(int n_games);" in header
    assert "#define XQ_RNG_KIND_RESIGN_HOLDOUT 12" in header and hip.RNG_KIND_RESIGN_HOLDOUT == 12
    assert "#define XQ_RESIGN_MAX_STEPS 8" in header and hip.RESIGN_MAX_STEPS == 8
    assert "typedef struct xq_resign_opts {" in header and "typedef struct xq_resign_row {" in header
    assert [f[0] for f in hip.ResignOpts._fields_] == ["threshold", "holdout_prob", "check_steps", "reserved"]
    assert C.sizeof(hip.ResignOpts) == 24 and C.sizeof(hip.ResignRow) == 32 == hip.RESIGN_ROW_BYTES
    assert [f[0] for f in hip.ResignRow._fields_] == list(sample_format.RESIGN_ROW_DTYPE.names)
    for name, field in zip(sample_format.RESIGN_ROW_DTYPE.names, hip.ResignRow._fields_):
        assert sample_format.RESIGN_ROW_DTYPE.fields[name][1] == getattr(hip.ResignRow, field[0]).offset, name
    vp, i32 = C.c_void_p, C.c_int32
    for name in ("xq_resign_state_bytes", "xq_resign_exempt_host", "xq_resign_scan_batch", "xq_engine_resign"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert lib.xq_engine_resign.argtypes == [C.POINTER(hip.Engine), C.POINTER(hip.ResignOpts), vp, vp, i32, vp, vp, vp]
    assert lib.xq_resign_scan_batch.argtypes == [vp, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp]
    assert lib.xq_resign_state_bytes(0) == 0 == lib.xq_resign_state_bytes(-3)
    assert lib.xq_resign_state_bytes(1) == hip.RESIGN_STATE_BYTES and lib.xq_resign_state_bytes(1024) == 1024 * 32
    # the kernel file is built by the wildcard of csrc/Makefile
    assert os.path.exists(os.path.join(ROOT, "xiangqi-alphazero_amd", "csrc", "xq_resign.hip"))


def test_engine_refusals_in_c_before_any_launch(lib):
    B, st, rows, cnt, ctr = C.byref, 0x400000, 0x500000, 0x600000, 0x700000
    call = lib.xq_engine_resign
    eng, ok = _fake_engine(), _opts()
    assert call(None, B(ok), st, rows, 16, cnt, ctr, None) == ARG
    assert call(B(eng), None, st, rows, 16, cnt, ctr, None) == ARG
    assert call(B(eng), B(ok), None, rows, 16, cnt, ctr, None) == ARG
    assert call(B(eng), B(ok), st, None, 16, cnt, ctr, None) == ARG
    assert call(B(eng), B(ok), st, rows, 16, None, ctr, None) == ARG
    assert call(B(eng), B(ok), st, rows, 16, cnt, None, None) == ARG
    assert call(B(eng), B(ok), st, rows, -1, cnt, ctr, None) == ARG
    bad = (dict(reserved=1), dict(check_steps=0), dict(check_steps=9), dict(check_steps=-1), dict(holdout_prob=-0.01),
           dict(holdout_prob=1.01), dict(holdout_prob=float("nan")), dict(threshold=float("nan")))
    for kw in bad:
        assert call(B(eng), B(_opts(**kw)), st, rows, 16, cnt, ctr, None) == ARG, kw
    for m in (1, 2, 3, -1):                                                   # search-only, arena, and no mode at all
        assert call(B(_fake_engine(m)), B(ok), st, rows, 16, cnt, ctr, None) == ARG, m
    # the engine's own rule must be the recorder: on, with a threshold no value is below
    assert call(B(_fake_engine(enable_resign=0)), B(ok), st, rows, 16, cnt, ctr, None) == ARG
    for t in (-0.9, 0.0, -1e308, float("inf"), float("nan")):
        assert call(B(_fake_engine(threshold=t)), B(ok), st, rows, 16, cnt, ctr, None) == ARG, t
    assert call(B(_fake_engine(n_games=0)), B(ok), st, rows, 16, cnt, ctr, None) == ARG


def test_scan_and_draw_refusals_in_c_before_any_launch(lib):
    p = 0x400000
    call = lib.xq_resign_scan_batch
    assert call(p, p, p, 0, 40, 2, -0.9, p, p, p, p, None) == 0                                    # an empty batch is a no-op
    assert call(None, None, None, 0, 0, 1, NINF, None, None, None, None, None) == 0
    assert call(p, p, p, -1, 40, 2, -0.9, p, p, p, p, None) == ARG
    assert call(p, p, p, 4, -1, 2, -0.9, p, p, p, p, None) == ARG
    for K in (0, 9, -2):
        assert call(p, p, p, 4, 40, K, -0.9, p, p, p, p, None) == ARG, K
    assert call(p, p, p, 4, 40, 2, float("nan"), p, p, p, p, None) == ARG
    for hole in range(7):
        ptrs = [p] * 7
        ptrs[hole] = None
        assert call(ptrs[0], ptrs[1], ptrs[2], 4, 40, 2, -0.9, ptrs[3], ptrs[4], ptrs[5], ptrs[6], None) == ARG, hole
    draw = lib.xq_resign_exempt_host
    assert draw(1, 0, 0, 1, 0.0) == 0 and draw(1, 0, 0, 1, 1.0) == 1
    for args in ((1, -1, 0, 1, 0.5), (1, 0, -1, 1, 0.5), (1, 0, 0, 1, -0.1), (1, 0, 0, 1, 1.1), (1, 0, 0, 1, float("nan"))):
        assert draw(*args) == ARG, args


def test_parse_resign_refuses_by_name():
    from xiangqi_alphazero_amd import engine, hip
    cfg = engine.make_config(8, 16)
    assert engine.parse_resign(cfg, None) is None
    opts, max_rows = engine.parse_resign(cfg, dict(threshold=-0.8))
    assert (opts.threshold, opts.check_steps, opts.holdout_prob, opts.reserved, max_rows) == (-0.8, 5, 0.1, 0, 1024)
    opts, max_rows = engine.parse_resign(engine.make_config(4096, 16), dict(threshold=NINF, check_steps=8, holdout_prob=1, max_rows=0))
    assert (opts.threshold, opts.check_steps, opts.holdout_prob, max_rows) == (NINF, 8, 1.0, 0)
    assert engine.parse_resign(engine.make_config(4096, 16), dict(threshold=0.0))[1] == 8 * 4096
    refused = [(cfg, dict(check_steps=2), "threshold"), (cfg, -0.9, "dict"), (cfg, dict(threshold=-0.9, steps=2), "keys"),
               (cfg, dict(threshold=float("nan")), "threshold"), (cfg, dict(threshold="low"), "threshold"),
               (cfg, dict(threshold=-0.9, check_steps=0), "check_steps"), (cfg, dict(threshold=-0.9, check_steps=9), "check_steps"),
               (cfg, dict(threshold=-0.9, check_steps=2.5), "check_steps"), (cfg, dict(threshold=-0.9, check_steps=True), "check_steps"),
               (cfg, dict(threshold=-0.9, holdout_prob=1.5), "holdout_prob"), (cfg, dict(threshold=-0.9, holdout_prob=-0.1), "holdout_prob"),
               (cfg, dict(threshold=-0.9, holdout_prob=float("nan")), "holdout_prob"),
               (cfg, dict(threshold=-0.9, max_rows=-1), "max_rows"), (cfg, dict(threshold=-0.9, max_rows=1.5), "max_rows"),
               (engine.make_config(8, 16, manual_moves=1), dict(threshold=-0.9), "self-play"),
               (engine.make_config(8, 16, manual_moves=2, add_noise=False), dict(threshold=-0.9), "self-play")]
    for c, arg, word in refused:
        with pytest.raises(hip.XqError, match="resign") as ei:
            engine.parse_resign(c, arg)
        assert word in str(ei.value), (arg, str(ei.value))


def test_the_engine_refuses_without_a_gpu_and_off_is_the_call_without_it(monkeypatch):
    from xiangqi_alphazero_amd import engine, hip, selfplay
    with pytest.raises(hip.XqError, match="resign.*check_steps"):
        engine.SelfPlayEngine(engine.make_config(8, 16), "cuda", resign=dict(threshold=-0.9, check_steps=12))
    with pytest.raises(hip.XqError, match="resign.*self-play"):
        engine.SelfPlayEngine(engine.make_config(8, 16, manual_moves=1), "cuda", resign=dict(threshold=-0.9))
    for fn in (engine.SelfPlayEngine.__init__, selfplay.run_games):
        assert inspect.signature(fn).parameters["resign"].default is None, fn
    for fn in (hip.resign_scan, hip.resign_exempt, engine.SelfPlayEngine.drain_resign_rows, engine.SelfPlayEngine.resign_stats,
               engine.SelfPlayEngine.resign_stage):
        assert callable(fn)
    with pytest.raises(hip.XqError, match="holdout_prob"):
        hip.resign_exempt(1, 0, 0, 1, 1.5)
    with pytest.raises(hip.XqError, match="negative"):
        hip.resign_exempt(1, 0, -1, 1, 0.5)
    # run_games: off, the engine is built by the call it made before; on, the argument arrives with one row per game
    made = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        made.append(kw)
        raise Stop

    monkeypatch.setattr(engine, "SelfPlayEngine", fake)
    monkeypatch.setattr(selfplay.evaluator, "make_evaluator", lambda *a, **kw: (None, "none"))
    config = types.SimpleNamespace(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30,
                                   random_opening_moves=2, enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    with pytest.raises(Stop):
        selfplay.run_games(None, config, 12, "cuda")
    assert "resign" not in made[-1]
    with pytest.raises(Stop):
        selfplay.run_games(None, config, 12, "cuda", resign=dict(threshold=-0.7, check_steps=3))
    assert made[-1]["resign"] == dict(threshold=-0.7, check_steps=3, max_rows=20)
    with pytest.raises(Stop):
        selfplay.run_games(None, config, 12, "cuda", resign=dict(threshold=-0.7, max_rows=5))
    assert made[-1]["resign"]["max_rows"] == 5


def _loop_config(tmp_path, **extra):
    base = dict(
        num_channels=16, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=4,
        max_game_length=30, random_opening_moves=2, enable_resign=True, resign_threshold=-0.9, resign_check_steps=5,
        learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40, min_buffer_size=4,
        num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55, save_interval=2, num_iterations=1,
        checkpoint_dir=str(tmp_path))
    return types.SimpleNamespace(**{**base, **extra})


def test_the_loop_checks_its_keys_at_construction(tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop
    bad = ((dict(resign_per_side=1), "resign_per_side"), (dict(resign_calibrate="yes"), "resign_calibrate"),
           (dict(resign_holdout_prob=1.5), "resign_holdout_prob"), (dict(resign_holdout_prob=float("nan")), "resign_holdout_prob"),
           (dict(resign_fp_target=-0.1), "resign_fp_target"), (dict(resign_min_pairs=0), "resign_min_pairs"),
           (dict(resign_min_pairs=2.5), "resign_min_pairs"), (dict(resign_threshold_max="x"), "resign_threshold_max"),
           (dict(resign_per_side=True, enable_resign=False), "enable_resign"),
           (dict(resign_per_side=True, resign_check_steps=9), "check_steps"))
    for extra, key in bad:
        cfg = _loop_config(tmp_path, **extra)
        with pytest.raises(hip.XqError, match=key):
            train_loop.AlphaZeroLoop(cfg, device="cpu", seed=1)
    assert train_loop.AlphaZeroLoop(_loop_config(tmp_path), device="cpu", seed=1).resign is None
    assert train_loop.AlphaZeroLoop(_loop_config(tmp_path, resign_per_side=False, resign_holdout_prob=0.3), device="cpu", seed=1).resign is None
    loop = train_loop.AlphaZeroLoop(_loop_config(tmp_path, resign_per_side=True), device="cpu", seed=1)
    assert loop.resign == dict(threshold=-0.9, check_steps=5, holdout_prob=0.1, calibrate=False, fp_target=0.05, min_pairs=20,
                               threshold_max=-0.5)
    assert loop.resign_threshold == -0.9
    loop = train_loop.AlphaZeroLoop(_loop_config(tmp_path, resign_per_side=True, resign_threshold=-0.3, resign_threshold_max=-0.2,
                                                 resign_holdout_prob=0.25, resign_calibrate=True, resign_fp_target=0.1,
                                                 resign_min_pairs=3), device="cpu", seed=1)
    assert loop.resign == dict(threshold=-0.3, check_steps=5, holdout_prob=0.25, calibrate=True, fp_target=0.1, min_pairs=3,
                               threshold_max=-0.2)
    assert train_loop.AlphaZeroLoop(_loop_config(tmp_path, resign_per_side=True, resign_threshold=-0.3), device="cpu",
                                    seed=1).resign["threshold_max"] == -0.3


def _holdout_rows():
    """Six holdout games: the pairs by level are -0.98 (lost), -0.97 (lost), -0.95 (lost), -0.92 (drew: a false positive),
    -0.85 (lost), -0.6 (won: a false positive); the other sides never had a window."""
    from xiangqi_alphazero_amd.sample_format import RESIGN_ROW_DTYPE
    rows = np.zeros(6, dtype=RESIGN_ROW_DTYPE)
    rows["slot"], rows["game_seq"] = np.arange(6), 1
    rows["level"] = [(-0.98, math.inf), (math.inf, -0.97), (-0.95, math.inf), (-0.92, math.inf), (math.inf, -0.85), (-0.6, math.inf)]
    rows["winner"] = [-1, 1, -1, 0, 1, 1]
    return rows


@pytest.mark.parametrize("mode", ["absent", "logged", "calibrated"])
def test_the_config_keys_reach_run_games_and_the_log(monkeypatch, tmp_path, mode):
    """One rank.  Absent, run_games is called as before and nothing is logged.  On, self-play gets the threshold, the steps and
    the holdout share, and the iteration's "resign" entry holds the threshold used, the games resigned, the holdout games, the
    pairs below the threshold with their false-positive rate and the calibrated threshold; with resign_calibrate the next
    iteration plays under that threshold."""
    import torch
    from xiangqi_alphazero_amd import selfplay, train_loop
    extra = {} if mode == "absent" else dict(resign_per_side=True, resign_holdout_prob=0.5, resign_fp_target=0.25, resign_min_pairs=2,
                                             resign_calibrate=mode == "calibrated")
    loop = train_loop.AlphaZeroLoop(_loop_config(tmp_path, **extra), device="cpu", seed=1)
    loop.config.resign_holdout_prob = 0.9                                     # read once
    seen = []

    def fake_run_games(model, config, n, device, **kw):
        seen.append(kw)
        st = dict(resign_rows=_holdout_rows(), resign_resigned=3, resign_holdout_games=6, resign_rows_dropped=0)
        return torch.empty((0, 640), dtype=torch.uint8), torch.empty((0, 16), dtype=torch.uint8), st, 0.0

    monkeypatch.setattr(selfplay, "run_games", fake_run_games)
    monkeypatch.setattr(loop, "train_network", lambda: {})
    monkeypatch.setattr(loop, "_save", lambda iteration: None)
    stats = loop.train(2)
    if mode == "absent":
        assert all("resign" not in kw for kw in seen) and all("resign" not in e for e in stats)
        return
    from xiangqi_alphazero_amd import resign
    s = float(np.nextafter(np.float32(-0.85), np.float32(np.inf)))            # 1 false positive of 5 pairs; at -0.6 it is 2 of 6
    assert resign.calibrate(_holdout_rows(), 0.25, 2, -0.5) == s
    assert seen[0]["resign"] == dict(threshold=-0.9, check_steps=5, holdout_prob=0.5)
    first = stats[0]["resign"]
    assert first == dict(threshold=-0.9, resigned=3, holdout_games=6, rows_dropped=0, pairs_below=4, fp_rate=0.25,
                         calibrated_threshold=s, calibrate=mode == "calibrated")
    used = s if mode == "calibrated" else -0.9
    assert seen[1]["resign"]["threshold"] == used and stats[1]["resign"]["threshold"] == used
    if mode == "calibrated":
        assert stats[1]["resign"]["pairs_below"] == 5 and stats[1]["resign"]["fp_rate"] == 0.2
    logged = json.load(open(os.path.join(str(tmp_path), "training_stats.json")))
    assert logged[0]["resign"] == first and [e["iteration"] for e in logged] == [1, 2]
