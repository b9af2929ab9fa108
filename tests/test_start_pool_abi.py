"""CPU checks of the start-position pool (include/xq_hip.h: xq_positions_check_batch, xq_engine_init_sp, xq_start_pool_draw_host):
the exports; pool == NULL and n == 0 being the xq_engine_*_gr pair over every accepted option combination of
tests/test_engine_options.py; every refusal on the C side before any launch and in the Python layer with a message that names the
option; the host draw; `start_pool.from_fens`; the loop's keys, key by key."""
import ctypes as C
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

from test_engine_options import ACCEPTED, _cfg, raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_positions_check_batch", "xq_engine_workspace_bytes_sp", "xq_engine_init_sp", "xq_start_pool_draw_host",
       "xq_engine_start_indices", "xq_engine_start_pool_stats_read")
PTR = 4096              # a pointer that is not NULL and is never followed: every call below returns before a launch


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _ref(x):
    return None if x is None else C.byref(x)


def _bytes_sp(lib, cfg, K, flags, cap, fp, gz, ar, pool, records=None, rules=None, solver=None, root_stats=None, mirror=None):
    return lib.xq_engine_workspace_bytes_sp(C.byref(cfg), K, flags, *(_ref(s) for s in (cap, fp, gz, ar, rules, solver, root_stats,
                                                                                       mirror, records, pool)))


def _bytes_gr(lib, cfg, K, flags, cap, fp, gz, ar):
    return lib.xq_engine_workspace_bytes_gr(C.byref(cfg), K, flags, *(_ref(s) for s in (cap, fp, gz, ar)), None, None, None, None, None)


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for name in NEW:
        assert name in hip.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header), name
    for text in ("#define XQ_POSITION_FATAL 15", "#define XQ_POSITION_NO_MOVE 16", "#define XQ_START_POOL_MAX (1 << 20)",
                 "#define XQ_RNG_KIND_START_POOL 11", "x0 = philox_u64(seed, rank, slot, 11, game_seq, 0)"):
        assert text in header, text
    assert (hip.POSITION_FATAL, hip.POSITION_NO_MOVE, hip.START_POOL_MAX, hip.RNG_KIND_START_POOL) == (15, 16, 1 << 20, 11)
    assert C.sizeof(hip.StartPool) == 32 and hip.StartPool.prob.offset == 24 and C.sizeof(hip.StartPoolStats) == 32


@pytest.mark.parametrize("name,cfg_kw,kw", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_null_and_empty_are_the_gr_pair(name, cfg_kw, kw):
    hip, lib = _lib()
    cfg = _cfg(cfg_kw)
    want = _bytes_gr(lib, cfg, *raw(kw))
    assert want > 0
    assert _bytes_sp(lib, cfg, *raw(kw), None) == want
    assert _bytes_sp(lib, cfg, *raw(kw), hip.StartPool(None, None, 0, 0, 0.0)) == want      # n = 0: nothing else is looked at
    assert _bytes_sp(lib, cfg, *raw(kw), hip.StartPool(PTR, PTR, 0, 0, 0.5)) == want


@pytest.mark.parametrize("name,cfg_kw,kw", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_a_pool_adds_exactly_its_words(name, cfg_kw, kw):
    """On, the workspace grows by the rows, the slots' indices and the head, each rounded to 256 bytes, plus at most 255 bytes of
    alignment in front of them; search-only and arena engines are refused."""
    hip, lib = _lib()
    cfg = _cfg(cfg_kw)
    got = _bytes_sp(lib, cfg, *raw(kw), hip.StartPool(PTR, PTR, 7, 0, 0.25))
    if cfg.manual_moves != 0:
        assert got == 0
        return
    G = cfg.n_games
    words = -(-7 * 96 // 256) * 256 + -(-G * 4 // 256) * 256 + 256
    base = _bytes_gr(lib, cfg, *raw(kw))
    assert base + words <= got <= base + words + 255 and got % 256 == 0


def test_every_refusal_comes_back_without_a_gpu():
    hip, lib = _lib()
    plain = (1, 0, None, None, None, None)

    def n(cfg, pool, **kw):
        return _bytes_sp(lib, cfg, *plain, pool, **kw)

    def init(cfg, pool, records=None):
        """xq_engine_init_sp on a host address that stands in for the workspace: refused before it is touched."""
        h = hip.Engine()
        buf = (C.c_uint8 * 1024)()
        base = (C.addressof(buf) + 255) & ~255
        rc = lib.xq_engine_init_sp(C.byref(h), C.byref(cfg), 1, 0, *([None] * 8), _ref(records), _ref(pool), base, 1 << 40, None, None)
        assert not any(buf) and h.pad0 == 0
        return rc

    cfg = _cfg({})
    good = hip.StartPool(PTR, PTR, 3, 0, 0.5)
    assert n(cfg, good) > n(cfg, None) > 0
    assert n(cfg, hip.StartPool(PTR, PTR, 1 << 20, 0, 1.0)) > 0 and n(cfg, hip.StartPool(PTR, PTR, 1, 0, 1e-300)) > 0
    refused = [("n < 0", hip.StartPool(PTR, PTR, -1, 0, 0.5)), ("n > 2^20", hip.StartPool(PTR, PTR, (1 << 20) + 1, 0, 0.5)),
               ("prob = 0", hip.StartPool(PTR, PTR, 3, 0, 0.0)), ("prob < 0", hip.StartPool(PTR, PTR, 3, 0, -0.5)),
               ("prob > 1", hip.StartPool(PTR, PTR, 3, 0, 1.0000001)), ("prob NaN", hip.StartPool(PTR, PTR, 3, 0, math.nan)),
               ("prob inf", hip.StartPool(PTR, PTR, 3, 0, math.inf)),
               ("reserved", hip.StartPool(PTR, PTR, 3, 1, 0.5)), ("reserved, n = 0", hip.StartPool(PTR, PTR, 0, 1, 0.5)),
               ("no boards", hip.StartPool(None, PTR, 3, 0, 0.5)), ("no sides", hip.StartPool(PTR, None, 3, 0, 0.5))]
    for what, pool in refused:
        assert n(cfg, pool) == 0, what
        assert init(cfg, pool) == -1, what
    for mm in (1, 2):                                      # search-only and arena engines
        assert n(_cfg(dict(manual_moves=mm)), good) == 0 and init(_cfg(dict(manual_moves=mm)), good) == -1
        assert n(_cfg(dict(manual_moves=mm)), None) > 0
    rec = hip.GameRecordsOpts(1, 4)                        # game records enabled
    assert n(cfg, good, records=rec) == 0 and init(cfg, good, records=rec) == -1
    assert n(cfg, good, records=hip.GameRecordsOpts(0, 4)) == n(cfg, good)
    assert n(cfg, None, records=rec) > 0
    # whatever the narrower pairs refuse stays refused
    assert n(cfg, good, mirror=hip.EvalMirrorOpts(2)) == 0 and n(cfg, good, rules=hip.RulesOpts(2)) == 0
    assert n(_cfg(dict(n_games=0)), good) == 0
    bad_flag = _bytes_sp(lib, cfg, 1, 1 << 6, None, None, None, None, good)     # the handle's private bit is no caller's flag
    assert bad_flag == 0
    # it goes with every other self-play option
    assert n(cfg, good, rules=hip.RulesOpts(1), solver=hip.SolverOpts(1), root_stats=hip.RootStatsOpts(1),
             mirror=hip.EvalMirrorOpts(1)) > 0
    for _, cfg_kw, kw in ACCEPTED:
        if not cfg_kw.get("manual_moves"):
            assert _bytes_sp(lib, _cfg(cfg_kw), *raw(kw), good) > 0, kw


def test_readers_and_check_argument_errors():
    hip, lib = _lib()
    h = hip.Engine()                                       # a handle without the option (all zero): refused before any HIP call
    p = C.c_void_p(77)
    st = hip.StartPoolStats()
    assert lib.xq_engine_start_indices(C.byref(h), C.byref(p)) == -1 and p.value == 77
    assert lib.xq_engine_start_indices(None, C.byref(p)) == -1
    assert lib.xq_engine_start_pool_stats_read(C.byref(h), C.byref(st), None) == -1
    assert lib.xq_engine_start_pool_stats_read(None, C.byref(st), None) == -1
    assert lib.xq_positions_check_batch(None, None, 0, None, None) == 0                  # n = 0: a no-op
    assert lib.xq_positions_check_batch(PTR, PTR, -1, PTR, None) == -1
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
        assert lib.xq_positions_check_batch(args[0], args[1], 2, args[2], None) == -1


def test_host_draw():
    hip, lib = _lib()
    from xiangqi_alphazero_amd import start_pool
    draw = start_pool.index_of
    n = 5
    a = [draw(7, 0, s, g, n, 0.5) for s in range(8) for g in range(1, 9)]
    assert a == [draw(7, 0, s, g, n, 0.5) for s in range(8) for g in range(1, 9)]           # deterministic
    assert set(a) <= set(range(-1, n)) and -1 in a
    full = [draw(7, 0, s, g, n, 1.0) for s in range(16) for g in range(1, 17)]
    assert -1 not in full and set(full) == set(range(n))                                    # never -1 at prob 1; every entry
    share = sum(draw(3, 0, s, g, 9, 0.25) >= 0 for s in range(64) for g in range(1, 65))
    sd = math.sqrt(4096 * 0.25 * 0.75)                                                      # 27.7: five of them are about 139
    assert abs(share - 1024) <= 5 * sd, share
    # the entry is the second draw's remainder: the first draw alone decides pool or not
    assert [x >= 0 for x in a] == [draw(7, 0, s, g, 11, 0.5) >= 0 for s in range(8) for g in range(1, 9)]
    base = [draw(11, 2, s, g, 1000, 1.0) for s in range(4) for g in range(1, 9)]
    assert base != [draw(12, 2, s, g, 1000, 1.0) for s in range(4) for g in range(1, 9)]    # seed
    assert base != [draw(11 + (1 << 32), 2, s, g, 1000, 1.0) for s in range(4) for g in range(1, 9)]     # its high word too
    assert base != [draw(11, 3, s, g, 1000, 1.0) for s in range(4) for g in range(1, 9)]    # rank
    assert base != [draw(11, 2, s + 4, g, 1000, 1.0) for s in range(4) for g in range(1, 9)]    # slot
    assert base != [draw(11, 2, s, g + 8, 1000, 1.0) for s in range(4) for g in range(1, 9)]    # game_seq
    assert len(set(base)) > 24
    # the C call with arguments outside its domain draws nothing; the Python layer names them
    assert lib.xq_start_pool_draw_host(1, 0, 0, 1, 0, 0.5) == -1 and lib.xq_start_pool_draw_host(1, 0, 0, 1, 4, math.nan) == -1
    assert lib.xq_start_pool_draw_host(1, 0, 0, 1, 4, 1.5) == -1
    for bad in (dict(n=0), dict(prob=0.0), dict(prob=math.nan), dict(slot=-1), dict(rank=-1), dict(game_seq=-1)):
        with pytest.raises(hip.XqError, match="start_pool_index"):
            draw(**{**dict(seed=1, rank=0, slot=0, game_seq=1, n=4, prob=0.5), **bad})


def test_host_draw_is_the_documented_philox():
    """xq_start_pool_draw_host against the header's formula on the evaluation mirror's host Philox (tests/eval_mirror_model.py)."""
    hip, lib = _lib()
    from eval_mirror_model import philox_u64
    from xiangqi_alphazero_amd import start_pool
    for seed, rank, slot, g, n, prob in ((5, 0, 0, 1, 7, 0.5), (2 ** 40 + 3, 3, 17, 9, 1000, 0.25), (9, 1, 2, 3, 1, 1.0)):
        x0, x1 = philox_u64(seed, rank, slot, 11, g, 0), philox_u64(seed, rank, slot, 11, g, 1)
        want = x1 % n if (x0 >> 11) * 2.0 ** -53 < prob else -1
        assert start_pool.index_of(seed, rank, slot, g, n, prob) == want


def test_from_fens_round_trips_board_to_fen(tmp_path):
    hip, _ = _lib()
    import golden_io as G
    from xiangqi_alphazero_amd import start_pool
    from xiangqi_alphazero_amd.sample_format import board_to_fen
    c = G.corpus()
    pick = np.arange(0, len(c["board"]), 97)
    lines = ["# a pool of %d positions" % len(pick), ""] + [board_to_fen(c["board"][i], int(c["side"][i])) for i in pick]
    lines.insert(5, "   # an indented comment")
    lines.insert(9, "   ")
    for source in (lines, "\n".join(lines) + "\n"):
        boards, sides = start_pool.from_fens(source)
        assert boards.dtype == np.int8 and sides.dtype == np.int8 and boards.shape == (len(pick), 90)
        assert boards.tobytes() == np.ascontiguousarray(c["board"][pick]).tobytes() and sides.tolist() == c["side"][pick].tolist()
    path = tmp_path / "pool.txt"
    path.write_text("\n".join(lines) + "\n")
    boards, sides = start_pool.from_fens(str(path))
    assert boards.tobytes() == np.ascontiguousarray(c["board"][pick]).tobytes() and sides.tolist() == c["side"][pick].tolist()
    assert [board_to_fen(b, int(s)) for b, s in zip(boards, sides)] == [ln for ln in lines if ln.strip() and not ln.lstrip().startswith("#")]
    dup = start_pool.from_fens([lines[2], lines[2], lines[3]])                  # duplicates are kept
    assert dup[0].shape == (3, 90) and dup[0][0].tobytes() == dup[0][1].tobytes()
    empty = start_pool.from_fens(["# nothing"])
    assert empty[0].shape == (0, 90) and empty[1].shape == (0,)
    with pytest.raises(ValueError, match="FEN"):
        start_pool.from_fens(["no position"])


def test_python_layer_keywords_and_refusals():
    hip, _ = _lib()
    from xiangqi_alphazero_amd import engine, selfplay, start_pool
    for fn in (engine.SelfPlayEngine.__init__, selfplay.run_games, selfplay.parallel_self_play):
        assert inspect.signature(fn).parameters["start_pool"].default is None, fn.__name__
    for name in ("start_indices", "start_pool_stats"):
        assert callable(getattr(engine.SelfPlayEngine, name))
    assert list(inspect.signature(start_pool.index_of).parameters) == ["seed", "rank", "slot", "game_seq", "n", "prob"]
    for name in ("from_fens", "from_table", "from_records"):
        assert callable(getattr(start_pool, name))
    assert list(inspect.signature(start_pool.from_table).parameters) == ["tb", "n", "kinds", "seed", "min_plies"]
    assert list(inspect.signature(start_pool.from_records).parameters)[:6] == ["records", "n", "seed", "min_ply", "max_ply",
                                                                                "perpetual_check"]
    P = engine.parse_start_pool
    cfg = _cfg({})
    boards, sides = np.zeros((3, 10, 9), dtype=np.int8), np.ones(3, dtype=np.int8)
    assert P(cfg, None) is None
    b, s, p = P(cfg, (boards, sides.tolist(), 1))
    assert b.shape == (3, 90) and b.dtype == np.int8 and s.dtype == np.int8 and p == 1.0
    for bad_cfg, pool, kw in (({}, (boards, sides), {}), ({}, (boards, sides[:2], 0.5), {}), ({}, (boards[:, :5], sides, 0.5), {}),
                              ({}, (boards[:0], sides[:0], 0.5), {}), ({}, (boards, sides, 0.0), {}), ({}, (boards, sides, 1.5), {}),
                              ({}, (boards, sides, math.nan), {}), ({}, (boards, sides, "x"), {}), ({}, 5, {}),
                              (dict(manual_moves=1), (boards, sides, 0.5), {}), (dict(manual_moves=2), (boards, sides, 0.5), {}),
                              ({}, (boards, sides, 0.5), dict(record_games=True))):
        with pytest.raises(hip.XqError, match="start_pool"):
            P(_cfg(bad_cfg), pool, **kw)


def _loop_config(**kw):
    return types.SimpleNamespace(**kw)


def test_loop_keys_one_by_one(tmp_path):
    hip, _ = _lib()
    from xiangqi_alphazero_amd.sample_format import board_to_fen
    from xiangqi_alphazero_amd.train_loop import _start_pool_options as opts
    from oracle import xq_oracle as O
    path = tmp_path / "start.txt"
    path.write_text("# two positions\n" + board_to_fen(O.initial_board(), 1) + "\n" + board_to_fen(O.initial_board(), -1) + "\n")
    assert opts(_loop_config()) is None
    assert opts(_loop_config(start_positions_file=None, start_positions_endgame=None, start_positions_prob=None)) is None
    on = opts(_loop_config(start_positions_file=str(path), start_positions_prob=0.25))
    assert on["file"] == str(path) and on["boards"].shape == (2, 90) and on["sides"].tolist() == [1, -1]
    assert on["endgame"] is None and on["prob"] == 0.25
    eg = opts(_loop_config(start_positions_endgame=64, endgame_signature="R", start_positions_prob=1))
    assert eg["endgame"] == 64 and eg["file"] is None and len(eg["boards"]) == 0 and eg["prob"] == 1.0
    both = opts(_loop_config(start_positions_file=str(path), start_positions_endgame=8, endgame_signature="CA",
                             start_positions_prob=0.5))
    assert both["endgame"] == 8 and len(both["boards"]) == 2
    cases = [
        (dict(start_positions_file=7, start_positions_prob=0.5), "start_positions_file"),
        (dict(start_positions_endgame=1.5, endgame_signature="R", start_positions_prob=0.5), "start_positions_endgame"),
        (dict(start_positions_endgame=True, endgame_signature="R", start_positions_prob=0.5), "start_positions_endgame"),
        (dict(start_positions_endgame=0, endgame_signature="R", start_positions_prob=0.5), "start_positions_endgame"),
        (dict(start_positions_endgame=(1 << 20) + 1, endgame_signature="R", start_positions_prob=0.5), "start_positions_endgame"),
        (dict(start_positions_endgame=8, start_positions_prob=0.5), "endgame_signature"),
        (dict(start_positions_file=str(path)), "start_positions_prob"),                    # required, no default
        (dict(start_positions_endgame=8, endgame_signature="R"), "start_positions_prob"),
        (dict(start_positions_file=str(path), start_positions_prob=0.0), "start_positions_prob"),
        (dict(start_positions_file=str(path), start_positions_prob=1.01), "start_positions_prob"),
        (dict(start_positions_file=str(path), start_positions_prob=math.nan), "start_positions_prob"),
        (dict(start_positions_file=str(path), start_positions_prob="half"), "start_positions_prob"),
        (dict(start_positions_prob=2.0), "start_positions_prob"),                          # out of range, the pool on or not
        (dict(start_positions_prob=0.5), "start_positions_prob"),                          # a probability without a source
        (dict(start_positions_file=str(path), start_positions_prob=0.5, record_games=True), "record_games"),
        (dict(start_positions_file=str(path), start_positions_prob=0.5, game_records_dir=str(tmp_path)), "game_records_dir"),
        (dict(start_positions_endgame=8, endgame_signature="R", start_positions_prob=0.5, record_games=True), "record_games"),
    ]
    for kw, names in cases:
        with pytest.raises(hip.XqError, match=names):
            opts(_loop_config(**kw))
    bad = tmp_path / "bad.txt"
    bad.write_text("not a position\n")
    with pytest.raises(hip.XqError, match="start_positions_file"):
        opts(_loop_config(start_positions_file=str(bad), start_positions_prob=0.5))
    none = tmp_path / "none.txt"
    none.write_text("# no position\n")
    with pytest.raises(hip.XqError, match="start_positions_file"):
        opts(_loop_config(start_positions_file=str(none), start_positions_prob=0.5))
    with pytest.raises(FileNotFoundError):
        opts(_loop_config(start_positions_file=str(tmp_path / "missing.txt"), start_positions_prob=0.5))
