"""CPU checks of game records (include/xq_hip.h: xq_game_record, xq_engine_init_gr, xq_replay_games_batch): the record's layout
in C, ctypes and numpy; records == NULL and enabled = 0 being the xq_engine_*_em pair over every accepted option combination of
tests/test_engine_options.py; every refusal on the C side before any launch and in parse_engine_options with a message that
names the option; the argument errors of the drains and of the replay; the keywords of the Python layer."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_engine_options import ACCEPTED, _cfg, raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_gr", "xq_engine_init_gr", "xq_engine_drain_games", "xq_engine_drain_games_device",
       "xq_engine_game_records_stats_read", "xq_replay_games_batch")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _ref(x):
    return None if x is None else C.byref(x)


def _bytes_gr(lib, cfg, K, flags, cap, fp, gz, ar, records, rules=None, solver=None, root_stats=None, mirror=None):
    return lib.xq_engine_workspace_bytes_gr(C.byref(cfg), K, flags, *(_ref(s) for s in (cap, fp, gz, ar, rules, solver, root_stats,
                                                                                       mirror, records)))


def _bytes_em(lib, cfg, K, flags, cap, fp, gz, ar):
    return lib.xq_engine_workspace_bytes_em(C.byref(cfg), K, flags, *(_ref(s) for s in (cap, fp, gz, ar)), None, None, None, None)


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for name in NEW:
        assert name in hip.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "#define XQ_RECORD_MAX_PLIES 504" in header


def test_record_layout_in_c_ctypes_and_numpy():
    hip, _ = _lib()
    from xiangqi_alphazero_amd import sample_format as F
    assert hip.GAME_RECORD_DTYPE is F.GAME_RECORD_DTYPE
    dt = hip.GAME_RECORD_DTYPE
    assert C.sizeof(hip.GameRecord) == dt.itemsize == hip.RECORD_BYTES == 1024      # the C side: static_assert in the sources
    assert hip.RECORD_MAX_PLIES == F.RECORD_MAX_PLIES == 504
    want = dict(slot=0, game_seq=4, winner=8, reason=9, n_moves=10, opening_plies=12, n_samples=14, moves=16)
    for name, off in want.items():
        assert getattr(hip.GameRecord, name).offset == off == dt.fields[name][1], name
        assert getattr(hip.GameRecord, name).size == dt.fields[name][0].itemsize, name
    assert dt.names == tuple(n for n, _ in hip.GameRecord._fields_)
    assert C.sizeof(hip.GameRecordsOpts) == 16 and C.sizeof(hip.GameRecordsStats) == 32
    # the result's fields sit where the record's do: one join key, one winner / reason
    for name in ("slot", "game_seq", "winner", "reason"):
        assert F.RESULT_DTYPE.fields[name] == dt.fields[name]


@pytest.mark.parametrize("name,cfg_kw,kw", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_null_and_disabled_are_the_em_pair(name, cfg_kw, kw):
    hip, lib = _lib()
    cfg = _cfg(cfg_kw)
    want = _bytes_em(lib, cfg, *raw(kw))
    assert want > 0
    assert _bytes_gr(lib, cfg, *raw(kw), None) == want
    assert _bytes_gr(lib, cfg, *raw(kw), hip.GameRecordsOpts(0, 0)) == want
    assert _bytes_gr(lib, cfg, *raw(kw), hip.GameRecordsOpts(0, 77)) == want


@pytest.mark.parametrize("name,cfg_kw,kw", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_enabled_adds_exactly_its_words(name, cfg_kw, kw):
    """On, the workspace grows by the ring, the log, the opening counts and the head, each rounded to 256 bytes, plus at most
    255 bytes of alignment in front of them; a search-only engine is refused."""
    hip, lib = _lib()
    cfg = _cfg(cfg_kw)
    got = _bytes_gr(lib, cfg, *raw(kw), hip.GameRecordsOpts(1, 5))
    if cfg.manual_moves == 1:
        assert got == 0
        return
    G = cfg.n_games
    words = 5 * 1024 + -(-G * 504 * 2 // 256) * 256 + -(-G * 2 // 256) * 256 + 256
    base = _bytes_em(lib, cfg, *raw(kw))
    assert base + words <= got <= base + words + 255 and got % 256 == 0


def test_every_refusal_comes_back_without_a_gpu():
    hip, lib = _lib()
    from xiangqi_alphazero_amd import engine
    plain = (1, 0, None, None, None, None)

    def n(cfg, rec, **kw):
        return _bytes_gr(lib, cfg, *plain, rec, **kw)

    cfg = _cfg({})
    assert n(cfg, hip.GameRecordsOpts(1, 1)) > 0
    for i in range(2):                                     # a non-zero reserved word, on or off
        for enabled in (0, 1):
            rec = hip.GameRecordsOpts(enabled, 4)
            rec.reserved[i] = 1
            assert n(cfg, rec) == 0, (enabled, i)
    assert n(cfg, hip.GameRecordsOpts(2, 4)) == 0 and n(cfg, hip.GameRecordsOpts(-1, 4)) == 0      # enabled outside {0, 1}
    assert n(cfg, hip.GameRecordsOpts(1, 0)) == 0 and n(cfg, hip.GameRecordsOpts(1, -3)) == 0      # max_out_games < 1
    assert n(_cfg(dict(manual_moves=1)), hip.GameRecordsOpts(1, 4)) == 0                           # search only
    assert n(_cfg(dict(manual_moves=2)), hip.GameRecordsOpts(1, 4)) > 0                            # arena games are games
    assert n(_cfg(dict(max_game_length=504)), hip.GameRecordsOpts(1, 4)) > 0
    assert n(_cfg(dict(max_game_length=505)), hip.GameRecordsOpts(1, 4)) == 0
    assert n(_cfg(dict(random_opening_moves=504)), hip.GameRecordsOpts(1, 4)) > 0
    assert n(_cfg(dict(random_opening_moves=505)), hip.GameRecordsOpts(1, 4)) == 0
    assert n(_cfg(dict(max_game_length=505)), hip.GameRecordsOpts(0, 4)) == n(_cfg(dict(max_game_length=505)), None) > 0
    # whatever the narrower pairs refuse stays refused
    assert n(cfg, hip.GameRecordsOpts(1, 4), mirror=hip.EvalMirrorOpts(2)) == 0
    assert n(cfg, hip.GameRecordsOpts(1, 4), rules=hip.RulesOpts(2)) == 0
    # it goes with every other option
    assert n(cfg, hip.GameRecordsOpts(1, 4), rules=hip.RulesOpts(1), solver=hip.SolverOpts(1), root_stats=hip.RootStatsOpts(1),
             mirror=hip.EvalMirrorOpts(1)) > 0
    for _, cfg_kw, kw in ACCEPTED:
        if cfg_kw.get("manual_moves") != 1:
            assert _bytes_gr(lib, _cfg(cfg_kw), *raw(kw), hip.GameRecordsOpts(1, 4)) > 0, kw

    # the parser refuses the same first, with a message that names the option
    P = engine.parse_engine_options
    opts = P(cfg, record_games=True)
    assert bytes(opts.game_records) == bytes(hip.GameRecordsOpts(1, cfg.max_out_results))           # the default ring
    assert bytes(P(cfg, record_games=True, max_out_games=3).game_records) == bytes(hip.GameRecordsOpts(1, 3))
    assert P(cfg).game_records is None and P(cfg, record_games=False).game_records is None
    for bad_cfg, kw in ((dict(manual_moves=1), dict(record_games=True)), (dict(max_game_length=505), dict(record_games=True)),
                        (dict(random_opening_moves=505), dict(record_games=True)), ({}, dict(record_games=True, max_out_games=0)),
                        ({}, dict(record_games=True, max_out_games=-1)), ({}, dict(record_games=True, max_out_games=1.5)),
                        ({}, dict(record_games=2))):
        with pytest.raises(hip.XqError, match="record_games"):
            P(_cfg(bad_cfg), **kw)
    with pytest.raises(hip.XqError, match="max_out_games"):
        P(cfg, max_out_games=4)
    assert P(_cfg(dict(max_game_length=504)), record_games=True).game_records is not None


def test_init_refuses_before_touching_the_workspace():
    """xq_engine_init_gr with refused options returns XQ_ERR_ARG before it looks at the workspace pointer's contents: a host
    address stands in for the device buffer and is never written."""
    hip, lib = _lib()
    cfg = _cfg(dict(manual_moves=1))
    h = hip.Engine()
    buf = (C.c_uint8 * 1024)()
    base = (C.addressof(buf) + 255) & ~255
    rec = hip.GameRecordsOpts(1, 4)
    rc = lib.xq_engine_init_gr(C.byref(h), C.byref(cfg), 1, 0, None, None, None, None, None, None, None, None, C.byref(rec), base, 1 << 40,
                               None, None)
    assert rc == -1 and not any(buf) and h.pad0 == 0


def test_drains_and_replay_argument_errors():
    hip, lib = _lib()
    h = hip.Engine()                                       # a handle without the option (all zero): refused before any HIP call
    n = C.c_int(-7)
    out = np.zeros(2, dtype=hip.GAME_RECORD_DTYPE)
    st = hip.GameRecordsStats()
    assert lib.xq_engine_drain_games(C.byref(h), out.ctypes.data, 2, C.byref(n), None) == -1
    assert lib.xq_engine_drain_games_device(C.byref(h), out.ctypes.data, 2, C.byref(n), None) == -1
    assert lib.xq_engine_game_records_stats_read(C.byref(h), C.byref(st), None) == -1
    assert lib.xq_engine_drain_games(None, out.ctypes.data, 2, C.byref(n), None) == -1
    assert lib.xq_engine_drain_games_device(None, None, 0, C.byref(n), None) == -1
    assert lib.xq_engine_drain_games(C.byref(h), out.ctypes.data, 2, None, None) == -1
    assert lib.xq_engine_game_records_stats_read(C.byref(h), None, None) == -1
    assert n.value == -7 and not out.view(np.uint8).any()
    status = np.zeros(1, dtype=np.int32)
    args = (None,) * 5
    assert lib.xq_replay_games_batch(None, None, 1, 0, *args, status.ctypes.data, None, None, None) == -1      # no records
    assert lib.xq_replay_games_batch(out.ctypes.data, None, 1, 0, *args, None, None, None, None) == -1         # no status
    assert lib.xq_replay_games_batch(out.ctypes.data, None, -1, 0, *args, status.ctypes.data, None, None, None) == -1
    assert lib.xq_replay_games_batch(out.ctypes.data, None, 1, 2, *args, status.ctypes.data, None, None, None) == -1
    assert lib.xq_replay_games_batch(None, None, 0, 0, *args, None, None, None, None) == 0                     # n = 0: a no-op


def test_python_layer_keywords():
    hip, _ = _lib()
    from xiangqi_alphazero_amd import arena, engine, selfplay
    for fn, names in ((engine.parse_engine_options, ("record_games", "max_out_games")),
                      (engine.SelfPlayEngine.__init__, ("record_games", "max_out_games")), (engine.arena_engine, ("record_games",)),
                      (selfplay.run_games, ("record_games",)), (selfplay.parallel_self_play, ("record_games",)),
                      (arena.play_arena, ("record_games",)), (arena.evaluate_models, ("record_games",))):
        for name in names:
            assert name in inspect.signature(fn).parameters, (fn.__name__, name)
    assert inspect.signature(selfplay.run_games).parameters["record_games"].default is None
    assert list(inspect.signature(engine.replay_games).parameters) == ["records", "stop_ply", "perpetual_check", "device"]
    for name in ("drain_games", "drain_games_device", "game_records_stats"):
        assert callable(getattr(engine.SelfPlayEngine, name))
    with pytest.raises(hip.XqError, match="GAME_RECORD_DTYPE"):
        engine.replay_games(np.zeros(2, dtype=np.uint8))
