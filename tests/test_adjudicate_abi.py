"""CPU-side checks of table adjudication (xq_tb_adjudicate_batch, xq_engine_adjudicate; include/xq_hip.h):
the exports, the refusals before any launch in C, the same refusals as XqError from parse_adjudicate / SelfPlayEngine / play_arena,
and the way of the option from the config keys to run_games.  No GPU is needed by any of it."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
RA = (C.c_int8 * 2)(5, -2)                               # the signature "Ra"
RA_ENTRIES = 162 * 91 * 6


@pytest.fixture(scope="module")
def lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


def _fake_engine(manual_moves=0, n_games=8):
    from xiangqi_alphazero_amd import hip
    e = hip.Engine()
    e.cfg.n_games, e.cfg.num_simulations, e.cfg.manual_moves = n_games, 32, manual_moves
    for i in range(32):
        e.p[i] = 0x200000 + 0x1000 * i                  # never dereferenced: every call below fails first
    return e


def _opts(draws=1, both_colours=1, min_ply=1, reserved=0):
    from xiangqi_alphazero_amd import hip
    return hip.AdjudicateOpts(draws, both_colours, min_ply, reserved)


def _table(signature="R"):
    from xiangqi_alphazero_amd import endgame
    return endgame.Tablebase(signature, np.zeros(endgame.entries(signature), dtype=np.int16))


def test_the_symbols_are_declared_exported_and_typed(lib):
    from xiangqi_alphazero_amd import hip
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "int xq_tb_adjudicate_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table, int64_t entries," in header
    assert "int xq_engine_adjudicate(const xq_engine *eng, const int8_t *pieces, int n_pieces, const int16_t *dev_table" in header
    assert "#define XQ_REASON_TABLE 5" in header and hip.REASON_TABLE == 5
    assert "typedef struct xq_adjudicate_opts {" in header
    assert [f[0] for f in hip.AdjudicateOpts._fields_] == ["draws", "both_colours", "min_ply", "reserved"]
    assert C.sizeof(hip.AdjudicateOpts) == 16
    vp, i32 = C.c_void_p, C.c_int32
    for name in ("xq_tb_adjudicate_batch", "xq_engine_adjudicate"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert lib.xq_tb_adjudicate_batch.argtypes == [vp, i32, vp, C.c_int64, vp, vp, i32, C.POINTER(hip.AdjudicateOpts), vp, vp, vp, vp]
    assert lib.xq_engine_adjudicate.argtypes == [C.POINTER(hip.Engine), vp, i32, vp, C.c_int64, C.POINTER(hip.AdjudicateOpts), vp, vp]
    assert lib.xq_tb_entries(RA, 2) == RA_ENTRIES


@pytest.mark.parametrize("manual", [0, 2], ids=["selfplay", "arena"])
def test_engine_refusals_in_c_before_any_launch(lib, manual):
    B, tab, cnt = C.byref, 0x400000, 0x500000
    call = lib.xq_engine_adjudicate
    eng, ok = _fake_engine(manual), _opts()
    assert call(None, RA, 2, tab, RA_ENTRIES, B(ok), cnt, None) == ARG
    assert call(B(eng), RA, 2, None, RA_ENTRIES, B(ok), cnt, None) == ARG
    assert call(B(eng), RA, 2, tab, RA_ENTRIES, None, cnt, None) == ARG
    assert call(B(eng), RA, 2, tab, RA_ENTRIES, B(ok), None, None) == ARG
    assert call(B(eng), (C.c_int8 * 2)(5, 9), 2, tab, RA_ENTRIES, B(ok), cnt, None) == ARG          # a bad signature
    assert call(B(eng), None, 2, tab, RA_ENTRIES, B(ok), cnt, None) == ARG
    assert call(B(eng), RA, 6, tab, RA_ENTRIES, B(ok), cnt, None) == ARG
    for entries in (RA_ENTRIES - 1, RA_ENTRIES + 1, 0, -1):
        assert call(B(eng), RA, 2, tab, entries, B(ok), cnt, None) == ARG, entries
    for bad in (dict(reserved=1), dict(min_ply=-1), dict(draws=2), dict(draws=-1), dict(both_colours=2), dict(both_colours=-1)):
        assert call(B(eng), RA, 2, tab, RA_ENTRIES, B(_opts(**bad)), cnt, None) == ARG, bad
    for m in (1, 3, -1):                                                                           # search-only, and no mode at all
        assert call(B(_fake_engine(m)), RA, 2, tab, RA_ENTRIES, B(ok), cnt, None) == ARG, m
    assert call(B(_fake_engine(manual, n_games=0)), RA, 2, tab, RA_ENTRIES, B(ok), cnt, None) == ARG


def test_batch_refusals_in_c_before_any_launch(lib):
    B, p = C.byref, 0x400000
    call = lib.xq_tb_adjudicate_batch
    ok = _opts(min_ply=0)
    assert call(RA, 2, p, RA_ENTRIES, p, p, 0, B(ok), p, p, p, None) == 0                           # an empty batch is a no-op
    assert call(RA, 2, None, RA_ENTRIES, None, None, 0, B(ok), None, None, None, None) == 0
    assert call(RA, 2, p, RA_ENTRIES, p, p, -1, B(ok), p, p, p, None) == ARG
    assert call(RA, 2, p, RA_ENTRIES, p, p, 4, None, p, p, p, None) == ARG
    assert call(RA, 2, p, RA_ENTRIES + 1, p, p, 4, B(ok), p, p, p, None) == ARG
    assert call((C.c_int8 * 1)(1), 1, p, 162, p, p, 4, B(ok), p, p, p, None) == ARG                 # a king is no signature piece
    for hole in range(6):
        ptrs = [p] * 6
        ptrs[hole] = None
        assert call(RA, 2, ptrs[0], RA_ENTRIES, ptrs[1], ptrs[2], 4, B(ok), ptrs[3], ptrs[4], ptrs[5], None) == ARG, hole
    for bad in (dict(reserved=1), dict(min_ply=-1), dict(draws=2), dict(both_colours=2)):
        assert call(RA, 2, p, RA_ENTRIES, p, p, 4, B(_opts(**bad)), p, p, p, None) == ARG, bad


def test_parse_adjudicate_refuses_by_name():
    from xiangqi_alphazero_amd import engine, hip
    tb = _table()
    selfplay_cfg, arena_cfg = engine.make_config(8, 16), engine.make_config(8, 16, manual_moves=2, add_noise=False)
    search_cfg = engine.make_config(8, 16, manual_moves=1)
    assert engine.parse_adjudicate(selfplay_cfg, None) is None
    for cfg in (selfplay_cfg, arena_cfg):
        tables, opts = engine.parse_adjudicate(cfg, ((tb,), None))
        assert tables == (tb,) and (opts.draws, opts.both_colours, opts.min_ply, opts.reserved) == (1, 1, 1, 0)
    tables, opts = engine.parse_adjudicate(selfplay_cfg, (tb, dict(draws=False, both_colours=False, min_ply=0)))
    assert tables == (tb,) and (opts.draws, opts.both_colours, opts.min_ply) == (0, 0, 0)
    assert len(engine.parse_adjudicate(selfplay_cfg, ([tb] * 4, {}))[0]) == 4
    refused = [(search_cfg, ((tb,), {}), "search"), (selfplay_cfg, ([tb] * 5, {}), "tables"), (selfplay_cfg, ([], {}), "tables"),
               (selfplay_cfg, ((tb,), dict(draws=2)), "draws"), (selfplay_cfg, ((tb,), dict(both_colours="yes")), "both_colours"),
               (selfplay_cfg, ((tb,), dict(min_ply=-1)), "min_ply"), (selfplay_cfg, ((tb,), dict(min_ply=1.5)), "min_ply"),
               (selfplay_cfg, ((tb,), dict(min_ply=True)), "min_ply"), (selfplay_cfg, ((tb,), dict(plies=3)), "options"),
               (selfplay_cfg, (("R",), {}), "Tablebase"), (selfplay_cfg, tb, "tables, options"), (selfplay_cfg, ((tb,), 3), "options")]
    for cfg, arg, word in refused:
        with pytest.raises(hip.XqError, match="adjudicate") as ei:
            engine.parse_adjudicate(cfg, arg)
        assert word in str(ei.value), (arg, str(ei.value))


def test_the_engine_and_the_arena_refuse_without_a_gpu(monkeypatch):
    from xiangqi_alphazero_amd import arena, engine, hip, selfplay
    tb = _table()
    with pytest.raises(hip.XqError, match="adjudicate.*search"):
        engine.SelfPlayEngine(engine.make_config(8, 16, manual_moves=1), "cuda", adjudicate=((tb,), {}))
    with pytest.raises(hip.XqError, match="adjudicate.*tables"):
        engine.SelfPlayEngine(engine.make_config(8, 16), "cuda", adjudicate=([tb] * 5, {}))
    with pytest.raises(hip.XqError, match="adjudicate.*min_ply"):
        engine.SelfPlayEngine(engine.make_config(8, 16), "cuda", adjudicate=((tb,), dict(min_ply=-2)))
    for kw in ({}, dict(opening_plies=2)):
        with pytest.raises(hip.XqError, match="adjudicate.*draws"):
            arena.play_arena(None, None, 4, 8, 20, adjudicate=((tb,), dict(draws=7)), **kw)
        with pytest.raises(hip.XqError, match="adjudicate.*tables"):
            arena.play_arena(None, None, 4, 8, 20, adjudicate=([tb] * 5, None), **kw)
    for fn in (engine.SelfPlayEngine.__init__, engine.arena_engine, arena.play_arena, selfplay.run_games):
        assert inspect.signature(fn).parameters["adjudicate"].default is None, fn
    assert engine.ADJUDICATE_DEFAULTS == dict(draws=True, both_colours=True, min_ply=1)
    sig = inspect.signature(hip.tb_adjudicate_batch).parameters
    assert sig["draws"].default is True and sig["both_colours"].default is True
    # off, the arena builds its engine by the call it made before
    made = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        made.append(kw)
        raise Stop

    monkeypatch.setattr(engine, "SelfPlayEngine", fake)
    for kw in ({}, dict(opening_plies=2)):
        with pytest.raises(Stop):
            arena.play_arena(None, None, 4, 8, 20, **kw)
        assert "adjudicate" not in made[-1]
        arg = ((tb,), dict(min_ply=3))
        with pytest.raises(Stop):
            arena.play_arena(None, None, 4, 8, 20, adjudicate=arg, **kw)
        assert made[-1]["adjudicate"] is arg


def test_records_to_text_prints_reason_5():
    from xiangqi_alphazero_amd import sample_format
    rec = np.zeros(1, dtype=sample_format.GAME_RECORD_DTYPE)
    rec["winner"], rec["reason"] = 1, 5
    text = sample_format.records_to_text(rec)
    assert "1-0 reason=5 " in text
    assert int(sample_format.records_from_text(text)["reason"][0]) == 5


def _loop_config(tmp_path, **extra):
    return types.SimpleNamespace(
        num_channels=16, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=4,
        max_game_length=30, random_opening_moves=2, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
        learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40, min_buffer_size=4,
        num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55, save_interval=2, num_iterations=1,
        checkpoint_dir=str(tmp_path), **extra)


def test_the_loop_checks_its_keys_at_construction(tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop
    for extra, key in ((dict(adjudicate_signatures="Ra"), "adjudicate_signatures"), (dict(adjudicate_signatures=["Rx"]), "adjudicate_signatures"),
                       (dict(adjudicate_signatures=["R"] * 5), "adjudicate_signatures"), (dict(adjudicate_draws=1), "adjudicate_draws"),
                       (dict(adjudicate_signatures=["R"], adjudicate_min_ply=-1), "adjudicate_min_ply"),
                       (dict(adjudicate_min_ply=0.5), "adjudicate_min_ply")):
        with pytest.raises(hip.XqError, match=key):
            train_loop.AlphaZeroLoop(_loop_config(tmp_path, **extra), device="cpu", seed=1)
    loop = train_loop.AlphaZeroLoop(_loop_config(tmp_path, adjudicate_signatures=["R", "ra"]), device="cpu", seed=1)
    assert loop.adjudicate == dict(signatures=["R", "ra"], draws=True, min_ply=1)
    assert train_loop.AlphaZeroLoop(_loop_config(tmp_path), device="cpu", seed=1).adjudicate is None
    assert train_loop.AlphaZeroLoop(_loop_config(tmp_path, adjudicate_signatures=[]), device="cpu", seed=1).adjudicate is None


@pytest.mark.parametrize("on", [True, False], ids=["on", "absent"])
def test_the_config_keys_reach_run_games(monkeypatch, tmp_path, on):
    """config.adjudicate_signatures / adjudicate_draws / adjudicate_min_ply are read once; on, self-play gets the tables (the
    endgame yardstick's own table for its signature, generated once) and logs the three fields; absent, run_games is called as
    before and nothing is logged."""
    import torch
    from xiangqi_alphazero_amd import endgame, selfplay, train_loop
    extra = dict(adjudicate_signatures=["R", "Ra"], adjudicate_draws=False, adjudicate_min_ply=2, endgame_signature="Ra") if on else {}
    loop = train_loop.AlphaZeroLoop(_loop_config(tmp_path, **extra), device="cpu", seed=1)
    loop.config.adjudicate_signatures, loop.config.adjudicate_min_ply = ["C"], 9      # read once
    generated, seen = [], []

    def fake_generate(signature, device="cuda", max_passes=None):
        generated.append(endgame.signature_text(signature))
        return _table(signature)

    def fake_run_games(model, config, n, device, **kw):
        seen.append(kw)
        st = dict(adjudicated_games=3, adjudicated_decisive=2, adjudicated_drawn=1, start_pool=None, start_pool_games=0)
        return torch.empty((0, 640), dtype=torch.uint8), torch.empty((0, 16), dtype=torch.uint8), st, 0.0

    monkeypatch.setattr(endgame.Tablebase, "generate", staticmethod(fake_generate))
    monkeypatch.setattr(selfplay, "run_games", fake_run_games)
    for _ in range(2):
        stats = loop.self_play()
    if not on:
        assert all("adjudicate" not in kw for kw in seen) and not any(k.startswith("adjudicated") for k in stats) and generated == []
        return
    tables, options = seen[-1]["adjudicate"]
    assert [t.signature for t in tables] == ["R", "Ra"] and options == dict(draws=False, min_ply=2)
    assert sorted(generated) == ["R", "Ra"] and tables[1] is loop._endgame_table()          # once each, and one "Ra" table for both
    assert seen[0]["adjudicate"][0] is tables
    assert (stats["adjudicated_games"], stats["adjudicated_decisive"], stats["adjudicated_drawn"]) == (3, 2, 1)
