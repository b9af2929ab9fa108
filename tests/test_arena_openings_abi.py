"""CPU checks of the arena options' ABI (include/xq_hip.h, xq_engine_init_ar): exports and header text, arena == NULL being
xq_engine_init_gz, the workspace (only arena-option engines grow), every refusal returned before any launch, the packed-arena
calls on NULL, and the Python layer: `evaluate_models` with the options off calls `play_arena` exactly as before, an odd
`eval_games` with openings is refused, and arena.py keeps clear of the self-play options."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_ar", "xq_engine_init_ar", "xq_engine_arena_openings", "xq_engine_compact_arena",
       "xq_engine_packed_arena", "xq_engine_expand_packed_arena")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    assert ("typedef struct xq_arena_opts { int32_t opening_plies; int32_t first_game; uint32_t reserved[2]; } xq_arena_opts;"
            in header)
    assert C.sizeof(hip.ArenaOpts) == 16 and hip.ArenaOpts.first_game.offset == 4 and hip.ArenaOpts.reserved.offset == 8
    assert C.sizeof(hip.Engine) == 384 and C.sizeof(hip.EngineConfig) == 112          # the handle and the config are as they were
    # the rules are written down where the host model is written from
    for phrase in ("g = first_game + s", "p = g / 2", "x_i % cnt", "philox_u64(cfg.seed, 0, p, 8, i, 0)",
                   "entry i of the slot's own stream 1", "position with NO opening, as self-play does; its recorded count is 0",
                   "((first_game + s) even) == (red is to move in the slot's REAL game)", "rows_evaluated grows by n_live0 + n_live1",
                   "arena == NULL is xq_engine_init_gz exactly"):
        assert phrase in header, phrase


def test_arena_null_is_init_gz():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    gz = hip.Gumbel(16, 0, 50.0, 1.0)
    for cfg in (engine.make_config(64, 100), engine.make_config(8, 24, manual_moves=2), engine.make_config(8, 24, manual_moves=1)):
        for K, flags, g in ((1, 0, None), (4, 0, None), (1, 1, None), (1, 0, gz), (2, 1, None)):
            gr = None if g is None else C.byref(g)
            want = lib.xq_engine_workspace_bytes_gz(C.byref(cfg), K, flags, None, None, gr)
            assert lib.xq_engine_workspace_bytes_ar(C.byref(cfg), K, flags, None, None, gr, None) == want
    # what xq_engine_init_gz refuses stays refused, through either entry point
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    ok = engine.make_config(8, 50)
    for cfg2, K, flags in ((ok, 1, 2), (ok, 2, 1), (ok, 0, 0), (engine.make_config(8, 50, manual_moves=2), 2, 0)):
        assert lib.xq_engine_workspace_bytes_ar(C.byref(cfg2), K, flags, None, None, None, None) == 0
        assert lib.xq_engine_init_gz(C.byref(h), C.byref(cfg2), K, flags, None, None, None, fake_ws, 1 << 40, None, None) == -1
        assert lib.xq_engine_init_ar(C.byref(h), C.byref(cfg2), K, flags, None, None, None, None, fake_ws, 1 << 40, None, None) == -1


def test_only_arena_option_engines_grow():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    for G_, S in ((10, 100), (1024, 100), (3, 7)):
        cfg = engine.make_config(G_, S, manual_moves=2)
        plain = lib.xq_engine_workspace_bytes(C.byref(cfg))
        assert plain > 0 and lib.xq_engine_workspace_bytes_ar(C.byref(cfg), 1, 0, None, None, None, None) == plain
        sizes = []
        for plies in (0, 4, 16):
            ar = hip.ArenaOpts(plies, 0)
            got = lib.xq_engine_workspace_bytes_ar(C.byref(cfg), 1, 0, None, None, None, C.byref(ar))
            sizes.append(got)
            # the record (4 + 32 B per slot) and two buffer sets of rows, planes, moves and counts (4 + 5400 + 256 + 4 B per slot)
            extra = 16 + G_ * 36 + 8 + 2 * G_ * (4 + 5400 + 256 + 4)
            assert plain + extra <= got <= plain + extra + 12 * 256, (G_, S, plies)     # regions are 256-byte aligned
        assert sizes[0] == sizes[1] == sizes[2]
        ar = hip.ArenaOpts(4, 7)
        assert lib.xq_engine_workspace_bytes_ar(C.byref(cfg), 1, 0, None, None, None, C.byref(ar)) == sizes[0]


def _bad_cases(hip, engine):
    arena = engine.make_config(8, 50, manual_moves=2)
    good = hip.ArenaOpts(4, 0)
    res0, res1 = hip.ArenaOpts(4, 0), hip.ArenaOpts(4, 0)
    res0.reserved[0], res1.reserved[1] = 1, 1
    return [("manual_moves 0", engine.make_config(8, 50), 1, 0, None, None, None, good),
            ("manual_moves 1", engine.make_config(8, 50, manual_moves=1), 1, 0, None, None, None, good),
            ("opening_plies -1", arena, 1, 0, None, None, None, hip.ArenaOpts(-1, 0)),
            ("opening_plies 17", arena, 1, 0, None, None, None, hip.ArenaOpts(17, 0)),
            ("first_game -1", arena, 1, 0, None, None, None, hip.ArenaOpts(4, -1)),
            ("first_game + n_games beyond int32", arena, 1, 0, None, None, None, hip.ArenaOpts(4, 2 ** 31 - 4)),
            ("reserved[0]", arena, 1, 0, None, None, None, res0),
            ("reserved[1]", arena, 1, 0, None, None, None, res1),
            # whatever xq_engine_init_gz refuses for an arena engine
            ("K = 2", arena, 2, 0, None, None, None, good),
            ("tree reuse", arena, 1, 1, None, None, None, good),
            ("unknown flags", arena, 1, 2, None, None, None, good),
            ("playout cap", arena, 1, 0, hip.PlayoutCap(10, 0, 0.25), None, None, good),
            ("forced playouts", arena, 1, 0, None, hip.ForcedPlayouts(2.0), None, good),
            ("gumbel", arena, 1, 0, None, None, hip.Gumbel(16, 0, 50.0, 1.0), good),
            ("no games", engine.make_config(0, 50, manual_moves=2), 1, 0, None, None, None, good)]


def test_ar_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h = hip.Engine()
    ref = lambda x: None if x is None else C.byref(x)
    for what, cfg, K, flags, cap, fp, gz, ar in _bad_cases(hip, engine):
        assert lib.xq_engine_workspace_bytes_ar(C.byref(cfg), K, flags, ref(cap), ref(fp), ref(gz), C.byref(ar)) == 0, what
        assert lib.xq_engine_init_ar(C.byref(h), C.byref(cfg), K, flags, ref(cap), ref(fp), ref(gz), C.byref(ar), fake_ws,
                                     1 << 40, None, None) == -1, what
    # allowed: the boundaries
    cfg = engine.make_config(8, 50, manual_moves=2)
    for ar in (hip.ArenaOpts(0, 0), hip.ArenaOpts(16, 0), hip.ArenaOpts(4, 2 ** 31 - 1 - 8)):
        assert lib.xq_engine_workspace_bytes_ar(C.byref(cfg), 1, 0, None, None, None, C.byref(ar)) > 0
    # injected draws need their pointer, as always
    inj = engine.make_config(8, 50, manual_moves=2, inject_len=4)
    ar = hip.ArenaOpts(4, 0)
    assert lib.xq_engine_init_ar(C.byref(h), C.byref(inj), 1, 0, None, None, None, C.byref(ar), fake_ws, 1 << 40, None, None) == -1


def test_packed_arena_calls_refuse_null_and_plain_engines():
    hip, lib = _lib()
    one = C.c_void_p(256)
    pbs = (hip.PackedBuffers * 2)()
    pa, pc = C.c_void_p(), C.c_void_p()
    assert lib.xq_engine_compact_arena(None, one, None) == -1
    assert lib.xq_engine_packed_arena(None, pbs) == -1
    assert lib.xq_engine_expand_packed_arena(None, one, one, one, one, None) == -1
    assert lib.xq_engine_arena_openings(None, C.byref(pa), C.byref(pc)) == -1
    plain = hip.Engine()                               # a handle without the option bit (all zero): refused before any launch
    plain.cfg.n_games = 8
    assert lib.xq_engine_compact_arena(C.byref(plain), one, None) == -1
    assert lib.xq_engine_packed_arena(C.byref(plain), pbs) == -1
    assert lib.xq_engine_expand_packed_arena(C.byref(plain), one, one, one, one, None) == -1
    assert lib.xq_engine_arena_openings(C.byref(plain), C.byref(pa), C.byref(pc)) == -1


def test_python_rejects_bad_arena_opts():
    from xiangqi_alphazero_amd import engine, hip
    arena_cfg = engine.make_config(4, 16, manual_moves=2)
    with pytest.raises(hip.XqError, match="arena_opts"):
        engine.SelfPlayEngine(engine.make_config(4, 16), "cpu", arena_opts=(4, 0))
    for bad in ((-1, 0), (17, 0), (4, -1), (4,), 4, "xy", (2.5, 0), (4, 2 ** 31)):
        with pytest.raises(hip.XqError, match="arena_opts"):
            engine.SelfPlayEngine(arena_cfg, "cpu", arena_opts=bad)
    import torch
    if not torch.cuda.is_available():                  # a valid option gets as far as the product path's own refusal
        with pytest.raises(hip.XqError, match="GPU"):
            engine.SelfPlayEngine(arena_cfg, "cpu", arena_opts=(4, 0))


def _config(**kw):
    base = dict(eval_games=6, eval_simulations=8, max_game_length=20, c_puct=1.5, eval_win_rate=0.55)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_evaluate_models_off_calls_play_arena_as_before(monkeypatch):
    from xiangqi_alphazero_amd import arena
    from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE
    calls = []

    def fake_play_arena(en, eo, n, sims, maxlen, c_puct, device, policy_is_probs=False, first_game=0):   # today's signature
        calls.append((en, eo, n, sims, maxlen, c_puct, device, policy_is_probs, first_game))
        res = np.zeros(n, dtype=RESULT_DTYPE)
        res["slot"], res["winner"], res["steps"] = np.arange(n), 1, 9
        return res

    monkeypatch.setattr(arena, "play_arena", fake_play_arena)
    monkeypatch.setattr(arena.ev_mod, "make_evaluator", lambda net, device, kind: (("ev", net), "fake"))
    for cfg in (_config(), _config(arena_opening_plies=0, arena_seed=5), _config(arena_opening_plies=None)):
        calls.clear()
        out = arena.evaluate_models("new", "old", cfg, "cpu")
        assert calls == [(("ev", "new"), ("ev", "old"), 6, 8, 20, 1.5, "cpu", False, 0)]
        assert sorted(out) == ["draws", "games", "model_updated", "new_wins", "old_wins", "win_rate"]
        assert (out["new_wins"], out["old_wins"], out["draws"]) == (3, 3, 0)


def test_evaluate_models_on_passes_the_options_and_adds_the_pair_statistics(monkeypatch):
    from xiangqi_alphazero_amd import arena
    from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE
    seen = {}

    def fake_play_arena(en, eo, n, sims, maxlen, c_puct, device, policy_is_probs=False, first_game=0, **kw):
        seen.update(kw)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        res["slot"], res["steps"] = np.arange(n), 9
        res["winner"] = [1, -1, 0, 1, -1, 1, 1, 0]
        kw["info"]["openings"] = np.arange(n * 16, dtype=np.uint16).reshape(n, 16)
        return res

    monkeypatch.setattr(arena, "play_arena", fake_play_arena)
    monkeypatch.setattr(arena.ev_mod, "make_evaluator", lambda net, device, kind: (None, "fake"))
    out = arena.evaluate_models("new", "old", _config(eval_games=8, arena_opening_plies=3, arena_seed=11), "cpu")
    assert seen["opening_plies"] == 3 and seen["seed"] == 11
    assert out["opening_plies"] == 3 and out["pairs"] == 4 and out["win_rate"] == 0.5 and not out["model_updated"]
    assert out["openings"].dtype == np.uint16 and out["openings"].shape == (8, 3) and out["openings"][1].tolist() == [16, 17, 18]
    assert abs(out["win_rate_se"] - (0.625 / 12.0) ** 0.5) < 1e-15
    assert out["win_rate_ci95"][0] < 0.5 < out["win_rate_ci95"][1]
    for k in ("new_wins", "old_wins", "draws", "win_rate", "model_updated"):          # the reference's keys stay
        assert k in out
    arena.evaluate_models("new", "old", _config(eval_games=8, arena_opening_plies=3, arena_seed=11), "cpu", seed=40)
    assert seen["seed"] == 40


def test_odd_eval_games_with_openings_is_refused(monkeypatch):
    from xiangqi_alphazero_amd import arena
    monkeypatch.setattr(arena, "play_arena", lambda *a, **k: pytest.fail("no game may start"))
    with pytest.raises(ValueError, match="even"):
        arena.evaluate_models("new", "old", _config(eval_games=7, arena_opening_plies=4), "cpu")


def test_train_loop_seeds_the_gate_by_iteration():
    from xiangqi_alphazero_amd import train_loop
    src = inspect.getsource(train_loop.AlphaZeroLoop._arena)
    assert "arena_seed" in src and "self.iteration" in src and "arena_opening_plies" in src


def test_arena_source_keeps_clear_of_the_self_play_options():
    from xiangqi_alphazero_amd import arena, engine
    src = inspect.getsource(arena)
    assert "gumbel" not in src and "forced_playouts" not in src
    sig = inspect.signature(arena.play_arena).parameters
    assert [sig[k].default for k in ("opening_plies", "seed", "packed", "inject")] == [0, 0, None, None]
    assert "arena_opts" in inspect.signature(engine.SelfPlayEngine.__init__).parameters
    for name in ("compact_arena", "expand_packed_arena", "arena_openings"):
        assert callable(getattr(engine.SelfPlayEngine, name))
