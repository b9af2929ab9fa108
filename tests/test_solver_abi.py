"""CPU checks of the proven-result search's ABI (include/xq_hip.h, xq_solver_opts): exports, struct sizes and header text;
solver == NULL and enabled = 0 being xq_engine_init_ru; every refusal on the C side before any launch and in
parse_engine_options with a message that names the option; the readers refused on an engine without the option; null pointers;
and the Python layer's plumbing of `solver` / `config.mcts_solver`."""
import ctypes as C
import inspect
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_sv", "xq_engine_init_sv", "xq_engine_read_root_states", "xq_engine_solver_stats_read")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _ref(x):
    return None if x is None else C.byref(x)


def _bad_solver(hip):
    out = [("enabled 2", hip.SolverOpts(2)), ("enabled -1", hip.SolverOpts(-1))]
    for e in (0, 1):
        for i in range(3):
            s = hip.SolverOpts(e)
            s.reserved[i] = 1
            out.append((f"enabled {e} reserved[{i}]", s))
    return out


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    assert "typedef struct xq_solver_opts { int32_t enabled; int32_t reserved[3]; } xq_solver_opts;" in header
    assert C.sizeof(hip.SolverOpts) == 16 and hip.SolverOpts.reserved.offset == 4
    assert C.sizeof(hip.SolverStats) == 64 and [n for n, _ in hip.SolverStats._fields_][:5] == list(hip.SOLVER_KEYS)
    assert C.sizeof(hip.Engine) == 384 and C.sizeof(hip.EngineConfig) == 112 and C.sizeof(hip.EngineStats) == 256
    for phrase in ("1. TERMINAL LEAF", "2. PROPAGATION", "3. DESCENT", "4. EARLY END OF A MOVE", "5. THE COUNTS A MOVE ENDS WITH",
                   "6. TREE REUSE", "7. UNCHANGED", "NOT the reference's \"every decided leaf is the mover's", "reserved1 = 1",
                   "solver == NULL or enabled = 0 is xq_engine_init_ru exactly", "+1 this move wins, -1 it loses, 2 draw, 0 unknown"):
        assert phrase in header, phrase
    assert hip.META_COUNT_MASK == 0x0FFF


def test_solver_null_and_zero_are_init_ru():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    gz, ar, cap, fp = hip.Gumbel(16, 0, 50.0, 1.0), hip.ArenaOpts(4, 0), hip.PlayoutCap(10, 0, 0.25), hip.ForcedPlayouts(2.0)
    ru = hip.RulesOpts(1)
    cases = [(engine.make_config(64, 100), 1, 0, None, None, None, None, None), (engine.make_config(64, 100), 4, 0, None, None, None, None, ru),
             (engine.make_config(64, 100), 1, 1, cap, fp, None, None, None), (engine.make_config(8, 24, manual_moves=1), 1, 0, None, None, gz, None, None),
             (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, ar, ru),
             (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, None, None)]
    for cfg, K, flags, c, f, g, a, r in cases:
        args = (C.byref(cfg), K, flags, _ref(c), _ref(f), _ref(g), _ref(a), _ref(r))
        want = lib.xq_engine_workspace_bytes_ru(*args)
        assert want > 0
        assert lib.xq_engine_workspace_bytes_sv(*args, None) == want
        assert lib.xq_engine_workspace_bytes_sv(*args, C.byref(hip.SolverOpts(0))) == want
        for what, bad in _bad_solver(hip):
            assert lib.xq_engine_workspace_bytes_sv(*args, C.byref(bad)) == 0, what
    # only solver engines grow: 64 bytes of counters per slot, rounded to the workspace's 256-byte regions
    on = hip.SolverOpts(1)
    for cfg, K, flags, c, f, g, a, r in ((engine.make_config(64, 100), 1, 0, None, None, None, None, None),
                                         (engine.make_config(64, 100), 1, 1, cap, None, None, None, ru),
                                         (engine.make_config(8, 24, manual_moves=1), 1, 0, None, None, None, None, None),
                                         (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, ar, None),
                                         (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, None, None)):
        args = (C.byref(cfg), K, flags, _ref(c), _ref(f), _ref(g), _ref(a), _ref(r))
        off, grown = lib.xq_engine_workspace_bytes_ru(*args), lib.xq_engine_workspace_bytes_sv(*args, C.byref(on))
        assert off < grown <= off + 64 * cfg.n_games + 512


# what the solver refuses: (name, config keywords, leaves_per_step, C structs (cap, forced, gumbel), Python keywords, message part)
REFUSED = [("leaves", {}, 4, (None, None, None), dict(leaves_per_step=4), "leaves_per_step"),
           ("gumbel", {}, 1, (None, None, "gz"), dict(gumbel=(16, 50.0, 1.0)), "gumbel"),
           ("gumbel_search_only", dict(manual_moves=1), 1, (None, None, "gz"), dict(gumbel=(16, 50.0, 1.0)), "gumbel"),
           ("forced", {}, 1, (None, "fp", None), dict(forced_playouts=2.0), "forced_playouts"),
           ("cap_forced", {}, 1, ("cap", "fp", None), dict(playout_cap=(0.25, 8), forced_playouts=2.0), "forced_playouts")]


@pytest.mark.parametrize("name,cfg_kw,K,structs,kw,part", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_combinations_on_both_sides(name, cfg_kw, K, structs, kw, part):
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(**{**dict(n_games=4, num_simulations=32), **cfg_kw})
    made = dict(cap=hip.PlayoutCap(8, 0, 0.25), fp=hip.ForcedPlayouts(2.0), gz=hip.Gumbel(16, 0, 50.0, 1.0))
    c, f, g = (None if s is None else made[s] for s in structs)
    on, h, fake_ws = hip.SolverOpts(1), hip.Engine(), C.c_void_p(1 << 20)
    args = (C.byref(cfg), K, 0, _ref(c), _ref(f), _ref(g), None, None)
    assert lib.xq_engine_workspace_bytes_sv(*args, None) > 0                       # fine without the solver
    assert lib.xq_engine_workspace_bytes_sv(*args, C.byref(on)) == 0
    assert lib.xq_engine_init_sv(C.byref(h), *args, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    engine.parse_engine_options(cfg, **kw)
    with pytest.raises(hip.XqError, match="solver") as e:
        engine.parse_engine_options(cfg, solver=True, **kw)
    assert part in str(e.value)


ALLOWED = [("plain", {}, {}), ("tree_reuse", {}, dict(tree_reuse=True)), ("playout_cap", {}, dict(playout_cap=(0.25, 8))),
           ("reuse_cap_cache_rule", {}, dict(tree_reuse=True, playout_cap=(0.25, 8), eval_cache_entries=64, perpetual_check=True)),
           ("search_only", dict(manual_moves=1), {}), ("arena", dict(manual_moves=2), {}),
           ("arena_opts", dict(manual_moves=2), dict(arena_opts=(4, 0)))]


@pytest.mark.parametrize("name,cfg_kw,kw", ALLOWED, ids=[a[0] for a in ALLOWED])
def test_allowed_combinations_on_both_sides(name, cfg_kw, kw):
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(**{**dict(n_games=4, num_simulations=32), **cfg_kw})
    off, on = engine.parse_engine_options(cfg, **kw), engine.parse_engine_options(cfg, solver=True, **kw)
    assert off.solver is None and engine.parse_engine_options(cfg, solver=False, **kw).solver is None
    assert isinstance(on.solver, hip.SolverOpts) and bytes(on.solver) == bytes(hip.SolverOpts(1)) and tuple(on)[:2] == tuple(off)[:2]
    refs = [_ref(o) for o in tuple(on)[2:]] + [_ref(on.rules)]
    assert lib.xq_engine_workspace_bytes_sv(C.byref(cfg), on.K, on.flags, *refs, C.byref(on.solver)) > \
        lib.xq_engine_workspace_bytes_ru(C.byref(cfg), on.K, on.flags, *refs) > 0
    for bad in (2, "yes", None):
        with pytest.raises(hip.XqError, match="solver"):
            engine.parse_engine_options(cfg, solver=bad, **kw)


def test_init_sv_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h, cfg, on = hip.Engine(), engine.make_config(8, 50), hip.SolverOpts(1)
    none = (None,) * 5
    for what, bad in _bad_solver(hip):
        assert lib.xq_engine_init_sv(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(bad), fake_ws, 1 << 40, None, None) == -1, what
    assert lib.xq_engine_init_sv(None, C.byref(cfg), 1, 0, *none, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_sv(C.byref(h), None, 1, 0, *none, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_sv(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(on), None, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_sv(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(on), C.c_void_p((1 << 20) + 8), 1 << 40, None,
                                 None) == -1                                   # workspace not 256-byte aligned
    inj = engine.make_config(8, 50, inject_len=4)
    assert lib.xq_engine_init_sv(C.byref(h), C.byref(inj), 1, 0, *none, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_sv(C.byref(h), C.byref(cfg), 1, 0, *none, C.byref(on), fake_ws, 16, None, None) == -3   # XQ_ERR_WORKSPACE
    # what xq_engine_init_ru refuses stays refused with the solver on
    for cfg2, K, flags in ((cfg, 1, 2), (cfg, 0, 0), (engine.make_config(8, 50, manual_moves=1), 1, 1)):
        assert lib.xq_engine_workspace_bytes_sv(C.byref(cfg2), K, flags, *none, C.byref(on)) == 0


def test_readers_refuse_an_engine_without_the_option_and_null_pointers():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    # handles as xq_engine_init* leaves them, made by hand: the checks come before any device access
    off = hip.Engine()
    off.cfg = engine.make_config(4, 32)
    on = hip.Engine()
    on.cfg = engine.make_config(4, 32)
    on.pad0 = 1 << 25                                  # "solver on"
    cs, rs, st = (C.c_int8 * hip.MAXM)(), C.c_int8(), hip.SolverStats()
    assert lib.xq_engine_read_root_states(C.byref(off), 0, cs, C.byref(rs), None) == -1
    assert lib.xq_engine_solver_stats_read(C.byref(off), C.byref(st), None) == -1
    assert lib.xq_engine_read_root_states(None, 0, cs, C.byref(rs), None) == -1
    assert lib.xq_engine_solver_stats_read(None, C.byref(st), None) == -1
    assert lib.xq_engine_read_root_states(C.byref(on), 0, None, C.byref(rs), None) == -1
    assert lib.xq_engine_read_root_states(C.byref(on), 0, cs, None, None) == -1
    assert lib.xq_engine_read_root_states(C.byref(on), -1, cs, C.byref(rs), None) == -1
    assert lib.xq_engine_read_root_states(C.byref(on), 4, cs, C.byref(rs), None) == -1
    assert lib.xq_engine_solver_stats_read(C.byref(on), None, None) == -1


def test_python_layer_passes_the_option_down(monkeypatch):
    from xiangqi_alphazero_amd import arena, engine, mcts, selfplay, train_loop
    for fn in (engine.parse_engine_options, engine.SelfPlayEngine.__init__, engine.arena_engine, selfplay.run_games,
               selfplay.parallel_self_play, arena.play_arena, arena.evaluate_models, mcts.MCTS.__init__):
        assert "solver" in inspect.signature(fn).parameters, fn
    for name in ("read_root_states", "solver_stats"):
        assert callable(getattr(engine.SelfPlayEngine, name))
    # config.mcts_solver reaches the gate: evaluate_models hands play_arena solver=True, and nothing when the key is absent or off
    seen = []

    def fake_play_arena(en, eo, games, sims, max_len, c_puct, device, **kw):
        import numpy as np
        from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE
        seen.append(kw)
        return np.zeros(games, dtype=RESULT_DTYPE)

    monkeypatch.setattr(arena, "play_arena", fake_play_arena)
    monkeypatch.setattr(arena.ev_mod, "make_evaluator", lambda m, d, k: (object(), None))
    base = dict(eval_games=4, eval_simulations=8, c_puct=1.5, max_game_length=20, eval_win_rate=0.55)
    out = arena.evaluate_models(None, None, types.SimpleNamespace(**base, mcts_solver=True))
    assert seen[-1].get("solver") is True and out["solver"] is True
    out = arena.evaluate_models(None, None, types.SimpleNamespace(**base))
    assert "solver" not in seen[-1] and "solver" not in out
    out = arena.evaluate_models(None, None, types.SimpleNamespace(**base, mcts_solver=True), solver=False)
    assert "solver" not in seen[-1]
    # play_arena hands it to the engine it builds, plain and with arena options
    made = []

    class Stop(Exception):
        pass

    def fake_engine(cfg, device="cuda", **kw):
        made.append(kw)
        raise Stop

    monkeypatch.undo()
    monkeypatch.setattr(engine, "SelfPlayEngine", fake_engine)
    for kw in ({}, dict(opening_plies=2), dict(info={})):
        for solver in (True, False):
            with pytest.raises(Stop):
                arena.play_arena(None, None, 4, 8, 20, solver=solver, **kw)
            assert made[-1]["solver"] is solver, kw


@pytest.mark.parametrize("flag", [True, False, None], ids=["on", "off", "absent"])
def test_loop_searches_and_gates_under_one_value(monkeypatch, tmp_path, flag):
    """An AlphaZeroLoop reads config.mcts_solver once and hands that one value to self-play and to the arena gate."""
    import torch
    from xiangqi_alphazero_amd import arena, selfplay, train_loop
    cfg = types.SimpleNamespace(
        num_channels=16, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=4,
        max_game_length=30, random_opening_moves=2, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
        learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40, min_buffer_size=4,
        num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55, save_interval=2, num_iterations=1,
        checkpoint_dir=str(tmp_path))
    if flag is not None:
        cfg.mcts_solver = flag
    seen = {}

    def fake_run_games(model, config, n, device, **kw):
        seen["selfplay"] = kw["solver"]
        return torch.empty((0, 640), dtype=torch.uint8), torch.empty((0, 16), dtype=torch.uint8), {}, 0.0

    def fake_evaluate_models(new, old, config, device, kind, **kw):
        seen.setdefault("arena", []).append(kw["solver"])
        return {"model_updated": False}

    monkeypatch.setattr(selfplay, "run_games", fake_run_games)
    monkeypatch.setattr(arena, "evaluate_models", fake_evaluate_models)
    loop = train_loop.AlphaZeroLoop(cfg, device="cpu", seed=1)
    loop._play_shard(4)
    loop._arena()
    cfg.arena_opening_plies = 2                        # the paired-openings branch of the gate passes it as well
    cfg.mcts_solver = not flag                         # ... and a later change of the config does not split the loop
    loop._arena()
    assert seen == {"selfplay": bool(flag), "arena": [bool(flag)] * 2} and loop.solver is bool(flag)


def test_solver_move_choice():
    """mcts.solver_choice, the move MCTS.get_action(temperature=0) takes from a solver engine's root: the first proven win, else
    the first maximum of the visits over the moves not shown to lose, else (every move loses) of all visits."""
    import numpy as np
    from xiangqi_alphazero_amd import mcts
    a, v = np.array([10, 20, 30, 40], dtype=np.uint16), np.array([5, 9, 2, 9])
    assert mcts.solver_choice(a, v, np.array([0, 0, 0, 0], dtype=np.int8)) == 20            # nothing proven: the first maximum
    assert mcts.solver_choice(a, v, np.array([0, -1, 0, 2], dtype=np.int8)) == 40           # the most visited move loses
    assert mcts.solver_choice(a, v, np.array([-1, 0, 1, 1], dtype=np.int8)) == 30           # the first proven win, however few visits
    assert mcts.solver_choice(a, v, np.array([-1, -1, -1, -1], dtype=np.int8)) == 20        # lost: plain visits
    assert mcts.solver_choice(a, np.array([7, 0, 0, 0]), np.array([-1, 0, 2, 0], dtype=np.int8)) == 20   # unvisited but not lost
