"""CPU checks of the root statistics per sample and the q-mixed value target (include/xq_hip.h: xq_root_stats_opts,
xq_sample_root_stats, xq_batch_opts): exports, struct sizes and header text; root_stats == NULL and enabled = 0 being
xq_engine_init_sv; every refusal on the C side before any launch and in parse_engine_options with a message that names the option;
xq_samples_to_batch_ex's argument errors; the numpy reference (sample_format.mixed_z / root_stats / to_reference_tuples) on
hand-made records; the config keys of run_games, AlphaZeroLoop and train_network; mcts.root_value."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_rs", "xq_engine_init_rs", "xq_samples_to_batch_ex")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _ref(x):
    return None if x is None else C.byref(x)


def _bad_root_stats(hip):
    out = [("enabled 2", hip.RootStatsOpts(2)), ("enabled -1", hip.RootStatsOpts(-1))]
    for e in (0, 1):
        for i in range(3):
            s = hip.RootStatsOpts(e)
            s.reserved[i] = 1
            out.append((f"enabled {e} reserved[{i}]", s))
    return out


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    assert "typedef struct xq_root_stats_opts { int32_t enabled; int32_t reserved[3]; } xq_root_stats_opts;" in header
    assert "typedef struct xq_batch_opts { double q_mix; int32_t reserved[2]; } xq_batch_opts;" in header
    assert "typedef struct xq_sample_root_stats {" in header and "#define XQ_SAMPLE_ROOT_STATS_OFFSET 108" in header
    assert C.sizeof(hip.RootStatsOpts) == 16 and hip.RootStatsOpts.reserved.offset == 4
    assert C.sizeof(hip.BatchOpts) == 16 and hip.BatchOpts.reserved.offset == 8
    assert C.sizeof(hip.Engine) == 384 and C.sizeof(hip.EngineConfig) == 112 and C.sizeof(hip.EngineStats) == 256
    for phrase in ("root_stats == NULL or enabled = 0 is xq_engine_init_sv exactly", "before forced-playout pruning",
                   "root_q = proven >= 0 ? 1.0f : (sumN > 0 ? (float)(sumW / (double)sumN) : 0.0f)",
                   "dev_z[j] = (float)((1.0 - q_mix) * (double)z + q_mix * (double)root_q)", "opts == NULL or q_mix = 0.0"):
        assert phrase in header, phrase
    from xiangqi_alphazero_amd import sample_format as F
    assert F.ROOT_STATS_DTYPE.itemsize == 20 and F.SAMPLE_DTYPE.fields["pad"][1] == 108
    assert [F.ROOT_STATS_DTYPE.fields[n][1] for n in ("root_q", "root_visits", "has_root_stats")] == [0, 4, 8]
    assert F.SAMPLE_DTYPE.itemsize == 640 and F.SAMPLE_DTYPE.names[-3:] == ("pad", "actions", "visits")


def _sv_cases(hip, engine):
    """The case list of tests/test_solver_abi.py, with the solver struct appended (None, off, and on where it is allowed)."""
    gz, ar, cap, fp = hip.Gumbel(16, 0, 50.0, 1.0), hip.ArenaOpts(4, 0), hip.PlayoutCap(10, 0, 0.25), hip.ForcedPlayouts(2.0)
    ru, on = hip.RulesOpts(1), hip.SolverOpts(1)
    return [(engine.make_config(64, 100), 1, 0, None, None, None, None, None, None),
            (engine.make_config(64, 100), 4, 0, None, None, None, None, ru, None),
            (engine.make_config(64, 100), 1, 1, cap, fp, None, None, None, hip.SolverOpts(0)),
            (engine.make_config(8, 24, manual_moves=1), 1, 0, None, None, gz, None, None, None),
            (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, ar, ru, on),
            (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, None, None, None),
            (engine.make_config(64, 100), 1, 1, cap, None, None, None, ru, on)]


def test_root_stats_null_and_zero_are_init_sv():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    for cfg, K, flags, *structs in _sv_cases(hip, engine):
        args = (C.byref(cfg), K, flags, *[_ref(s) for s in structs])
        want = lib.xq_engine_workspace_bytes_sv(*args)
        assert want > 0
        assert lib.xq_engine_workspace_bytes_rs(*args, None) == want
        assert lib.xq_engine_workspace_bytes_rs(*args, C.byref(hip.RootStatsOpts(0))) == want
        for what, bad in _bad_root_stats(hip):
            assert lib.xq_engine_workspace_bytes_rs(*args, C.byref(bad)) == 0, what
        # no workspace of its own: on, where it is allowed (self-play without Gumbel), the bytes are the same
        allowed = int(cfg.manual_moves) == 0 and structs[2] is None
        assert lib.xq_engine_workspace_bytes_rs(*args, C.byref(hip.RootStatsOpts(1))) == (want if allowed else 0)


# what root_stats refuses: (name, config keywords, the Gumbel struct or None, Python keywords, message part)
REFUSED = [("search_only", dict(manual_moves=1), False, {}, "manual_moves"), ("arena", dict(manual_moves=2), False, {}, "manual_moves"),
           ("gumbel", {}, True, dict(gumbel=(16, 50.0, 1.0)), "gumbel")]


@pytest.mark.parametrize("name,cfg_kw,gumbel,kw,part", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_combinations_on_both_sides(name, cfg_kw, gumbel, kw, part):
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(**{**dict(n_games=4, num_simulations=32), **cfg_kw})
    gz = hip.Gumbel(16, 0, 50.0, 1.0) if gumbel else None
    on, h, fake_ws = hip.RootStatsOpts(1), hip.Engine(), C.c_void_p(1 << 20)
    args = (C.byref(cfg), 1, 0, None, None, _ref(gz), None, None, None)
    assert lib.xq_engine_workspace_bytes_rs(*args, None) > 0                       # fine without the option
    assert lib.xq_engine_workspace_bytes_rs(*args, C.byref(on)) == 0
    assert lib.xq_engine_init_rs(C.byref(h), *args, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    engine.parse_engine_options(cfg, **kw)
    with pytest.raises(hip.XqError, match="root_stats") as e:
        engine.parse_engine_options(cfg, root_stats=True, **kw)
    assert part in str(e.value)


ALLOWED = [("plain", dict()), ("leaves", dict(leaves_per_step=4)), ("tree_reuse", dict(tree_reuse=True)),
           ("playout_cap", dict(playout_cap=(0.25, 8))), ("forced", dict(forced_playouts=2.0)),
           ("solver_reuse_cap_cache_rule", dict(solver=True, tree_reuse=True, playout_cap=(0.25, 8), eval_cache_entries=64,
                                                perpetual_check=True))]


@pytest.mark.parametrize("name,kw", ALLOWED, ids=[a[0] for a in ALLOWED])
def test_allowed_combinations_on_both_sides(name, kw):
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(4, 32)
    off, on = engine.parse_engine_options(cfg, **kw), engine.parse_engine_options(cfg, root_stats=True, **kw)
    assert off.root_stats is None and engine.parse_engine_options(cfg, root_stats=False, **kw).root_stats is None
    assert isinstance(on.root_stats, hip.RootStatsOpts) and bytes(on.root_stats) == bytes(hip.RootStatsOpts(1))
    assert tuple(on)[:2] == tuple(off)[:2] and len(tuple(on)) == 6
    refs = [_ref(o) for o in tuple(on)[2:]] + [_ref(on.rules), _ref(on.solver)]
    assert lib.xq_engine_workspace_bytes_rs(C.byref(cfg), on.K, on.flags, *refs, C.byref(on.root_stats)) == \
        lib.xq_engine_workspace_bytes_sv(C.byref(cfg), on.K, on.flags, *refs) > 0
    for bad in (2, "yes", None):
        with pytest.raises(hip.XqError, match="root_stats"):
            engine.parse_engine_options(cfg, root_stats=bad, **kw)


def test_init_rs_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h, cfg, on = hip.Engine(), engine.make_config(8, 50), hip.RootStatsOpts(1)
    none = (None,) * 6
    for what, bad in _bad_root_stats(hip):
        assert lib.xq_engine_init_rs(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(bad), fake_ws, 1 << 40, None, None) == -1, what
    assert lib.xq_engine_init_rs(None, C.byref(cfg), 1, 0, *none, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_rs(C.byref(h), None, 1, 0, *none, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_workspace_bytes_rs(None, 1, 0, *none, C.byref(on)) == 0
    assert lib.xq_engine_init_rs(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(on), None, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_rs(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(on), C.c_void_p((1 << 20) + 8), 1 << 40, None,
                                 None) == -1                                   # workspace not 256-byte aligned
    inj = engine.make_config(8, 50, inject_len=4)
    assert lib.xq_engine_init_rs(C.byref(h), C.byref(inj), 1, 0, *none, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_rs(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(on), fake_ws, 16, None, None) == -3   # XQ_ERR_WORKSPACE
    # what xq_engine_init_sv refuses stays refused with the option on: flags 2 and 6, K = 0, and the solver with forced playouts
    for K, flags in ((1, 2), (1, 6), (0, 0)):
        assert lib.xq_engine_workspace_bytes_rs(C.byref(cfg), K, flags, *none, C.byref(on)) == 0
    fp, sv = hip.ForcedPlayouts(2.0), hip.SolverOpts(1)
    assert lib.xq_engine_workspace_bytes_rs(C.byref(cfg), 1, 0, None, C.byref(fp), None, None, None, C.byref(sv), C.byref(on)) == 0


def test_samples_to_batch_ex_argument_errors():
    """q_mix outside [0, 1] or NaN, a reserved word, and xq_samples_to_batch's own rules: all before any launch (the device
    pointers are null or fake and n > 0)."""
    hip, lib = _lib()
    fake = C.c_void_p(1 << 20)
    ptrs = (fake,) * 3

    def call(opts, n=4, t=0.3, outs=ptrs, ins=ptrs):
        return lib.xq_samples_to_batch_ex(*ins, n, t, _ref(opts), *outs, None)

    for q in (-0.25, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(hip.BatchOpts(q)) == -1, q
    for i in range(2):
        for q in (0.0, 0.5):
            o = hip.BatchOpts(q)
            o.reserved[i] = 1
            assert call(o) == -1, (i, q)
    for opts in (None, hip.BatchOpts(0.0), hip.BatchOpts(0.5), hip.BatchOpts(1.0)):
        assert call(opts, outs=(None, fake, fake)) == -1 and call(opts, outs=(fake, None, fake)) == -1
        assert call(opts, outs=(fake, fake, None)) == -1 and call(opts, ins=(None, fake, fake)) == -1
        assert call(opts, ins=(fake, None, fake)) == -1 and call(opts, ins=(fake, fake, None)) == -1
        assert call(opts, n=-1) == -1 and call(opts, t=0.0) == -1
        assert call(opts, outs=(fake, C.c_void_p((1 << 20) + 4), fake)) == -1     # pi not 16-byte aligned
        assert call(opts, n=0, outs=(None, None, None), ins=(None, None, None)) == 0   # n = 0 is a no-op
    assert call(hip.BatchOpts(2.0), n=0) == -1                                      # the option check comes first


def _records():
    """Hand-made records: every (z, root_q, mark) of z in {-1, 0, 1}, root_q in {-1, -0.0, 0.3, 1}, mark in {0, 1}."""
    from xiangqi_alphazero_amd import sample_format as F
    combos = [(z, q, m) for z in (-1, 0, 1) for q in (-1.0, -0.0, 0.3, 1.0) for m in (0, 1)]
    smp = np.zeros(len(combos), dtype=F.SAMPLE_DTYPE)
    pad = np.zeros(len(combos), dtype=F.ROOT_STATS_DTYPE)
    for k, (z, q, m) in enumerate(combos):
        smp[k]["board"][4], smp[k]["board"][85] = 1, -1
        smp[k]["side"], smp[k]["z"], smp[k]["n_moves"], smp[k]["ply"], smp[k]["slot"], smp[k]["game_seq"] = 1, z, 1, k, 0, 1
        smp[k]["actions"][0], smp[k]["visits"][0] = 4 * 90 + 13, 7
        pad[k]["root_q"], pad[k]["root_visits"], pad[k]["has_root_stats"] = q, 16, m
    smp["pad"] = pad.view(np.uint8).reshape(len(combos), 20)
    return smp, combos


def test_numpy_reference_on_hand_made_records():
    from xiangqi_alphazero_amd import sample_format as F
    smp, combos = _records()
    rs = F.root_stats(smp)
    assert rs.dtype == F.ROOT_STATS_DTYPE and rs.shape == (len(combos),)
    assert [(float(r["root_q"]), int(r["has_root_stats"]), int(r["root_visits"])) for r in rs] == \
        [(float(np.float32(q)), m, 16) for _, q, m in combos]
    assert bytes(rs[3]["root_q"].tobytes()) == np.float32(-0.0).tobytes()           # the sign of -0.0 survives the view
    for lam in (0.0, 0.25, 1.0):
        got = F.mixed_z(smp, lam)
        assert got.dtype == np.float32 and got.shape == (len(combos),)
        for k, (z, q, m) in enumerate(combos):
            want = np.float32((1.0 - lam) * float(z) + lam * float(np.float32(q))) if (m and lam > 0.0) else np.float32(z)
            assert got[k].tobytes() == want.tobytes(), (lam, z, q, m)               # the same IEEE operations: bit for bit
            if lam == 1.0 and m:
                assert got[k] == np.float32(q)                                       # lambda = 1 returns root_q exactly
            if not m or lam == 0.0:
                assert got[k] == np.float32(z)
    assert F.mixed_z(smp, 1.0)[[k for k, c in enumerate(combos) if c == (1, 0.3, 1)][0]] == np.float32(0.3)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            F.mixed_z(smp, bad)
    # the dense adapter: z of every tuple (and of its mirror image) is mixed_z of its record, in ply order
    res = np.zeros(1, dtype=F.RESULT_DTYPE)
    res[0]["slot"], res[0]["game_seq"], res[0]["n_samples"] = 0, 1, len(combos)
    plain, _ = F.to_reference_tuples(smp, res)
    assert [t[2] for t in plain] == [float(z) for z, _, _ in combos for _ in (0, 1)]
    for lam in (0.0, 0.25, 1.0):
        data, per_game = F.to_reference_tuples(smp, res, q_mix=lam)
        want = F.mixed_z(smp, lam)
        assert per_game == [(0, 0, len(combos))] and len(data) == 2 * len(combos)
        assert [t[2] for t in data] == [float(w) for w in want for _ in (0, 1)]
        for (s0, p0, _), (s1, p1, _) in zip(plain, data):
            assert (s0 == s1).all() and (p0 == p1).all()                             # planes and pi do not depend on the option


def _train_config(**extra):
    return types.SimpleNamespace(min_buffer_size=4, num_epochs=1, batch_size=8, **extra)


def test_train_network_refuses_a_mixed_target_without_marked_records():
    """Before any kernel call, so a CPU buffer shows it: lambda > 0 on a buffer whose records carry no root statistics."""
    import torch
    from xiangqi_alphazero_amd import hip, training
    smp, combos = _records()
    unmarked = smp[[k for k, c in enumerate(combos) if c[2] == 0]]
    buf = training.ReplayBuffer(200, device="cpu")
    assert buf.root_stats_coverage() == 0.0                                           # empty
    buf.extend(unmarked)
    assert buf.root_stats_coverage() == 0.0 and len(buf) == 2 * len(unmarked)
    net = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10])
    with pytest.raises(hip.XqError, match="root statistics"):
        training.train_network(net, opt, sch, buf, _train_config(), q_mix=0.5)
    with pytest.raises(hip.XqError, match="root statistics"):                          # the config's lambda is the default
        training.train_network(net, opt, sch, buf, _train_config(value_target_q_mix=0.25))
    for bad in (-0.5, 1.5):
        with pytest.raises(hip.XqError, match="value_target_q_mix"):
            training.train_network(net, opt, sch, buf, _train_config(), q_mix=bad)
    assert training.train_network(net, opt, sch, training.ReplayBuffer(200, device="cpu"), _train_config(), q_mix=0.5) == {}
    # coverage over the ring's live records only: 1 marked of the 4 held after the ring wrapped
    ring = training.ReplayBuffer(8, device="cpu")                                      # 4 records
    marked = smp[[k for k, c in enumerate(combos) if c[2] == 1]]
    ring.extend(marked[:3])
    assert ring.root_stats_coverage() == 1.0
    ring.extend(unmarked[:3])                                                          # wraps: holds marked[2], unmarked[0..2]
    assert ring.count == 4 and ring.root_stats_coverage() == 0.25


def test_python_layer_reads_the_config_keys(monkeypatch, tmp_path):
    from xiangqi_alphazero_amd import engine, hip, mcts, selfplay, train_loop, training
    for fn in (engine.parse_engine_options, engine.SelfPlayEngine.__init__, selfplay.run_games):
        assert "root_stats" in inspect.signature(fn).parameters, fn
    assert "q_mix" in inspect.signature(training.train_network).parameters
    assert "q_mix" in inspect.signature(training.ReplayBuffer.batch).parameters
    assert "return_values" in inspect.signature(mcts.MCTS.search_many).parameters
    made = []

    class Stop(Exception):
        pass

    def fake_engine(cfg, device="cuda", **kw):
        made.append(kw)
        raise Stop

    monkeypatch.setattr(engine, "SelfPlayEngine", fake_engine)
    monkeypatch.setattr(selfplay.evaluator, "make_evaluator", lambda m, d, k: (object(), "fake"))
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
    for extra, kw, want in (({}, {}, False), (dict(record_root_stats=True), {}, True), (dict(value_target_q_mix=0.5), {}, True),
                            (dict(value_target_q_mix=0.0), {}, False), (dict(record_root_stats=True), dict(root_stats=False), False),
                            ({}, dict(root_stats=True), True)):
        with pytest.raises(Stop):
            selfplay.run_games(None, types.SimpleNamespace(**base, **extra), 4, "cpu", **kw)
        assert made[-1]["root_stats"] is want, (extra, kw)
    with pytest.raises(hip.XqError, match="gumbel"):
        selfplay.run_games(None, types.SimpleNamespace(**base, value_target_q_mix=0.5, gumbel_considered=8), 4, "cpu")
    with pytest.raises(hip.XqError, match="value_target_q_mix"):
        selfplay.run_games(None, types.SimpleNamespace(**base, value_target_q_mix=1.5), 4, "cpu")
    # the loop checks the keys at construction
    loop_cfg = dict(base, num_channels=16, num_res_blocks=1, num_games_per_iter=4, learning_rate=0.01, weight_decay=1e-4,
                    lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40, min_buffer_size=4, num_epochs=1, batch_size=8,
                    eval_games=4, eval_simulations=4, eval_win_rate=0.55, save_interval=2, num_iterations=1,
                    checkpoint_dir=str(tmp_path))
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**loop_cfg), device="cpu", seed=1)
    assert loop.q_mix == 0.0 and loop.record_root_stats is False
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**loop_cfg, value_target_q_mix=0.25), device="cpu", seed=1)
    assert loop.q_mix == 0.25 and loop.record_root_stats is True
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**loop_cfg, record_root_stats=True), device="cpu", seed=1)
    assert loop.q_mix == 0.0 and loop.record_root_stats is True
    with pytest.raises(hip.XqError, match="gumbel"):
        train_loop.AlphaZeroLoop(types.SimpleNamespace(**loop_cfg, value_target_q_mix=0.25, gumbel_considered=8), device="cpu")
    # ... once: self-play and the train step are handed the loop's two values, whatever the config says by then
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**loop_cfg, value_target_q_mix=0.25), device="cpu", seed=1)
    loop.config.value_target_q_mix = 0.75
    with pytest.raises(Stop):
        loop._play_shard(2)
    assert made[-1]["root_stats"] is True
    seen = {}
    monkeypatch.setattr(training, "train_network", lambda *a, **kw: seen.update(kw) or {})
    assert loop.train_network() == {} and seen["q_mix"] == 0.25
    # a key that holds None is the absent key, for both readers
    assert selfplay.root_stats_q_mix(types.SimpleNamespace(value_target_q_mix=None)) == 0.0


def test_mcts_root_value():
    from xiangqi_alphazero_amd import mcts
    assert mcts.root_value(np.zeros(0, np.int32), np.zeros(0)) == np.float32(0.0)      # no legal move
    assert mcts.root_value(np.array([0, 0], np.int32), np.array([0.0, 0.0])) == np.float32(0.0)
    v = mcts.root_value(np.array([1, 2, 0], np.int32), np.array([0.1, 0.2, 0.0]))
    assert isinstance(v, np.float32) and v == np.float32((0.1 + 0.2) / 3.0)
    w = np.array([0.1, 0.7, -0.3, 1e-17, 0.2])
    n = np.array([3, 5, 2, 1, 5], np.int32)
    seq = 0.0
    for x in w:
        seq += float(x)
    assert mcts.root_value(n, w) == np.float32(seq / 16.0)
