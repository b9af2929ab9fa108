"""CPU-side checks of the settled-move cutoff (xq_engine_settle; include/xq_hip.h): the export, the
refusals before any launch in C, the same refusals as XqError from parse_early_stop / SelfPlayEngine / MCTS / AlphaZeroLoop, and
the way of the option from config.early_stop_decided to the engine.  No GPU is needed by any of it."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
# pad0 of an engine handle (csrc/xq_engine_state.cuh): leaves per step in the low 16 bits, XQ_ENGINE_TREE_REUSE in bit 16, then
# the options' private bits
PAD0 = dict(leaves=4, reuse=1 << 16, cap=1 << 30, forced=1 << 29, gumbel=1 << 28, solver=1 << 25)


@pytest.fixture(scope="module")
def lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


def _fake_engine(manual_moves=2, pad0=0, n_games=8, sims=32):
    from xiangqi_alphazero_amd import hip
    e = hip.Engine()
    e.cfg.n_games, e.cfg.num_simulations, e.cfg.manual_moves, e.pad0 = n_games, sims, manual_moves, pad0
    for i in range(32):
        e.p[i] = 0x200000 + 0x1000 * i                  # never dereferenced: every call below fails first
    return e


def test_the_symbol_is_declared_exported_and_typed(lib):
    from xiangqi_alphazero_amd import hip
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "int xq_engine_settle(const xq_engine *eng, unsigned long long *dev_counters" in header
    assert "xq_engine_settle" in hip.EXPORTS and hasattr(lib, "xq_engine_settle")
    assert lib.xq_engine_settle.argtypes == [C.POINTER(hip.Engine), C.c_void_p, C.c_void_p]


@pytest.mark.parametrize("manual", [1, 2], ids=["search_only", "arena"])
def test_refusals_in_c_before_any_launch(lib, manual):
    B, buf = C.byref, 0x400000
    assert lib.xq_engine_settle(None, buf, None) == ARG
    assert lib.xq_engine_settle(B(_fake_engine(manual)), None, None) == ARG
    assert lib.xq_engine_settle(B(_fake_engine(0)), buf, None) == ARG                       # self-play
    assert lib.xq_engine_settle(B(_fake_engine(3)), buf, None) == ARG
    assert lib.xq_engine_settle(B(_fake_engine(manual, n_games=0)), buf, None) == ARG
    for name, bits in PAD0.items():
        assert lib.xq_engine_settle(B(_fake_engine(manual, pad0=bits)), buf, None) == ARG, name
    # the options it goes with do not make it refuse by themselves: the perpetual-check rule, game records, the evaluation mirror
    # are not in the list, and a refusal of theirs would show here as ARG on a handle that is otherwise refused for one reason
    assert lib.xq_engine_settle(B(_fake_engine(manual, pad0=PAD0["solver"] | (1 << 26))), buf, None) == ARG


REFUSED = [
    (dict(leaves_per_step=4), "leaves_per_step"),
    (dict(solver=True), "solver"),
    (dict(gumbel=(4, 50.0, 1.0)), "gumbel"),
    (dict(playout_cap=(0.25, 4)), "playout_cap"),
    (dict(forced_playouts=2.0), "forced_playouts"),
    (dict(tree_reuse=True), "tree_reuse"),
]


@pytest.mark.parametrize("opts, word", REFUSED, ids=[r[1] for r in REFUSED])
def test_refusals_name_the_option(opts, word):
    from xiangqi_alphazero_amd import engine, hip
    for manual in (1, 2):
        cfg = engine.make_config(8, 16, manual_moves=manual)
        assert engine.parse_early_stop(cfg, False, **opts) is False
        with pytest.raises(hip.XqError, match="early_stop") as ei:
            engine.parse_early_stop(cfg, True, **opts)
        assert word in str(ei.value)


def test_the_engine_refuses_without_a_gpu():
    from xiangqi_alphazero_amd import engine, hip
    with pytest.raises(hip.XqError, match="early_stop.*self-play"):
        engine.SelfPlayEngine(engine.make_config(8, 16), "cuda", early_stop=True)
    with pytest.raises(hip.XqError, match="early_stop.*self-play"):
        engine.parse_early_stop(engine.make_config(8, 16), True)
    with pytest.raises(hip.XqError, match="early_stop must be a bool"):
        engine.parse_early_stop(engine.make_config(8, 16, manual_moves=1), 2)
    search = engine.make_config(8, 16, manual_moves=1, add_noise=False)
    arena_cfg = engine.make_config(8, 16, manual_moves=2, add_noise=False)
    for kw, word in ((dict(leaves_per_step=4), "leaves_per_step"), (dict(solver=True), "solver"),
                     (dict(gumbel=(4, 50.0, 1.0)), "gumbel")):
        with pytest.raises(hip.XqError, match="early_stop") as ei:
            engine.SelfPlayEngine(search, "cuda", early_stop=True, **kw)
        assert word in str(ei.value)
    with pytest.raises(hip.XqError, match="early_stop.*solver"):
        engine.SelfPlayEngine(arena_cfg, "cuda", early_stop=True, solver=True)
    with pytest.raises(hip.XqError, match="early_stop.*solver"):
        engine.arena_engine(arena_cfg, "cuda", 2, 0, solver=True, early_stop=True)
    for cfg in (search, arena_cfg):                                                           # it goes with these
        assert engine.parse_early_stop(cfg, True) is True
    for fn in (engine.SelfPlayEngine.__init__, engine.arena_engine):
        assert inspect.signature(fn).parameters["early_stop"].default is False


def test_mcts_checks_at_construction_and_keys_its_engines(monkeypatch):
    from xiangqi_alphazero_amd import engine, hip, mcts
    assert inspect.signature(mcts.MCTS.__init__).parameters["early_stop"].default is False
    with pytest.raises(hip.XqError, match="early_stop.*solver"):
        mcts.MCTS(lambda x: x, 8, solver=True, early_stop=True)
    with pytest.raises(hip.XqError, match="early_stop.*leaves_per_step"):
        mcts.MCTS(lambda x: x, 8, leaves_per_step=4, early_stop=True)
    made = []

    class Stop(Exception):
        pass

    def fake_engine(cfg, device="cuda", **kw):
        made.append((int(cfg.n_games), int(cfg.manual_moves), kw))
        raise Stop

    monkeypatch.setattr(engine, "SelfPlayEngine", fake_engine)
    game = types.SimpleNamespace(board=np.zeros((10, 9), np.int8), current_player=1, move_count=0, no_capture_count=0, history=[])
    on, off = mcts.MCTS(lambda x: x, 8, early_stop=True), mcts.MCTS(lambda x: x, 8)
    assert on.early_stop is True and off.early_stop is False
    for m, call, want in ((on, lambda: on.get_action(game, temperature=0), True),
                          (on, lambda: on.get_action(game, temperature=1.0), False),       # a sampled move wants every count
                          (on, lambda: on.search(game, temperature=0.0, add_noise=False), False),
                          (on, lambda: on.search_many([game, game], add_noise=False), False),
                          (on, lambda: on.search_decided([game, game]), True),
                          (off, lambda: off.get_action(game, temperature=0), False),
                          (off, lambda: off.search_decided([game]), False)):
        with pytest.raises(Stop):
            call()
        assert made[-1][1] == 1 and made[-1][2]["early_stop"] is want
    monkeypatch.setattr(engine, "SelfPlayEngine", lambda cfg, device="cuda", **kw: object())
    m = mcts.MCTS(lambda x: x, 8, early_stop=True)
    a, b, c = m._engine(1, False), m._engine(1, False, True), m._engine(1, True, True)
    assert a is not b and b is not c and m._engine(1, False, False) is a and m._engine(1, False, True) is b
    assert set(m._engines) == {(1, False), (1, False, True), (1, True, True)}      # the full searches keep their key


def test_play_arena_and_the_yardsticks_hand_it_on(monkeypatch):
    from xiangqi_alphazero_amd import arena, baseline, endgame, engine, mcts, tactics
    for fn in (arena.play_arena, endgame.hold_rate, endgame.play_out):
        assert inspect.signature(fn).parameters["early_stop"].default is False, fn
    assert inspect.signature(arena.evaluate_models).parameters["early_stop"].default is None
    made = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        made.append(kw)
        raise Stop

    monkeypatch.setattr(engine, "SelfPlayEngine", fake)
    for kw in ({}, dict(opening_plies=2), dict(info={})):
        for flag in (True, False):
            with pytest.raises(Stop):
                arena.play_arena(None, None, 4, 8, 20, early_stop=flag, **kw)
            assert made[-1]["early_stop"] is flag, kw
    # the baseline match and the tactics pass, whose signatures are closed, search with the MCTS they are handed
    searcher = mcts.MCTS(lambda x: x, 8, early_stop=True)
    assert mcts.as_mcts(searcher, 99, 1.0, "cuda", "hip", solver=True) is searcher
    assert mcts.as_mcts(searcher, 99, 1.0, "cuda", "hip").num_simulations == 8              # its own simulations hold
    monkeypatch.setattr(mcts, "MCTS", type("FakeMCTS", (), {"__init__": lambda self, *a, **kw: fake(**kw)}))
    with pytest.raises(Stop):
        mcts.as_mcts(object(), 16, 1.5, "cuda", "hip", seed=2, solver=True)
    assert made[-1] == dict(seed=2, solver=True)
    for fn in (baseline.play_vs_baseline, tactics.solve_rate, endgame._searched_moves):      # each searches through the one door
        src = inspect.getsource(fn)
        assert "search_decided(" in src and "search_many(" not in src, fn
    for fn in (baseline.play_vs_baseline, tactics.solve_rate):
        assert "as_mcts(model_or_evaluator" in inspect.getsource(fn)


@pytest.mark.parametrize("plies", [0, 2], ids=["plain", "openings"])
def test_evaluate_models_reads_the_key_and_reports_the_option(monkeypatch, plies):
    from xiangqi_alphazero_amd import arena
    from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE
    seen = []

    def fake_play_arena(en, eo, games, *a, **kw):
        seen.append(kw)
        if "info" in kw:
            kw["info"]["openings"] = np.zeros((games, 16), dtype=np.uint16)
        return np.zeros(games, dtype=RESULT_DTYPE)

    monkeypatch.setattr(arena.ev_mod, "make_evaluator", lambda m, d, k: (object(), "fake"))
    monkeypatch.setattr(arena, "play_arena", fake_play_arena)
    base = dict(eval_games=4, eval_simulations=8, max_game_length=20, c_puct=1.5, eval_win_rate=0.55, arena_opening_plies=plies)
    for extra, kw, want in (({}, {}, False), (dict(early_stop_decided=True), {}, True), (dict(early_stop_decided=False), {}, False),
                            (dict(early_stop_decided=True), dict(early_stop=False), False), ({}, dict(early_stop=True), True)):
        out = arena.evaluate_models(None, None, types.SimpleNamespace(**base, **extra), "cpu", **kw)
        assert seen[-1].get("early_stop", False) is want and out.get("early_stop", False) is want
        assert want or "early_stop" not in seen[-1]          # off: play_arena is called as before


def _loop_config(tmp_path, **extra):
    return types.SimpleNamespace(
        num_channels=16, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=4,
        max_game_length=30, random_opening_moves=2, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
        learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40, min_buffer_size=4,
        num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55, save_interval=2, num_iterations=1,
        checkpoint_dir=str(tmp_path), **extra)


def test_the_loop_refuses_the_solver_beside_it_and_names_both_keys(tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop
    with pytest.raises(hip.XqError) as ei:
        train_loop.AlphaZeroLoop(_loop_config(tmp_path, early_stop_decided=True, mcts_solver=True), device="cpu", seed=1)
    assert "early_stop_decided" in str(ei.value) and "mcts_solver" in str(ei.value)
    assert train_loop.AlphaZeroLoop(_loop_config(tmp_path, mcts_solver=True), device="cpu", seed=1).early_stop is False


@pytest.mark.parametrize("flag", [True, False, None], ids=["on", "off", "absent"])
def test_the_config_key_reaches_the_gate_and_the_yardsticks(monkeypatch, tmp_path, flag):
    """config.early_stop_decided (absent: off) is read once; on, the arena gate and the endgame calls get early_stop=True and
    the baseline match and the tactics pass an MCTS built with it; off, every call is the call it was; self-play never gets it."""
    import torch
    from xiangqi_alphazero_amd import arena, baseline, endgame, mcts, selfplay, tactics, train_loop
    extra = {} if flag is None else dict(early_stop_decided=flag)
    loop = train_loop.AlphaZeroLoop(_loop_config(tmp_path, **extra), device="cpu", seed=1)
    assert loop.early_stop is bool(flag)
    loop.config.early_stop_decided = not flag            # read once
    seen = {}

    class Stop(Exception):
        pass

    def catch(name):
        def f(*a, **kw):
            seen[name] = dict(kw, first=a[0] if a else None)
            raise Stop
        return f

    class FakeMCTS:
        def __init__(self, model, sims, *a, **kw):
            self.model, self.sims, self.kw = model, sims, kw

    monkeypatch.setattr(mcts, "MCTS", FakeMCTS)

    def fake_run_games(model, config, n, device, **kw):
        seen["selfplay"] = kw
        return torch.empty((0, 640), dtype=torch.uint8), torch.empty((0, 16), dtype=torch.uint8), {}, 0.0

    monkeypatch.setattr(selfplay, "run_games", fake_run_games)
    monkeypatch.setattr(arena, "evaluate_models", catch("arena"))
    monkeypatch.setattr(baseline, "play_vs_baseline", catch("baseline"))
    monkeypatch.setattr(tactics, "solve_rate", catch("tactics"))
    monkeypatch.setattr(endgame, "hold_rate", catch("hold"))
    monkeypatch.setattr(endgame, "play_out", catch("play_out"))
    loop._play_shard(2)
    assert "early_stop" not in seen["selfplay"]
    loop.baseline = dict(games=2, depth=1, simulations=4, opening_plies=2, interval=1)
    loop.tactics, loop._tactics_puzzles = dict(simulations=4, max_moves=3), object()
    loop.endgame, loop._endgame_tb, loop._endgame_positions = dict(simulations=4, signature="KRK", kind="win"), object(), ((), ())
    loop.endgame_playout, loop._endgame_playout_positions = dict(positions=1, max_plies=5), ((), ())
    calls = dict(arena=loop._arena, baseline=loop.play_baseline, tactics=loop.score_tactics, hold=loop.score_endgame,
                 play_out=loop.play_out_endgame)
    for name, call in calls.items():
        with pytest.raises(Stop):
            call()
        first = seen[name]["first"]
        if name in ("baseline", "tactics"):
            assert "early_stop" not in seen[name]
            if flag:
                assert isinstance(first, FakeMCTS) and first.model is loop.best_model and first.sims == 4
                assert first.kw["early_stop"] is True and first.kw["solver"] is False and first.kw["perpetual_check"] is False
            else:
                assert first is loop.best_model
        elif flag:
            assert seen[name]["early_stop"] is True, name
        else:
            assert "early_stop" not in seen[name], name
    loop.config.arena_opening_plies = 2                  # the gate's other call
    with pytest.raises(Stop):
        loop._arena()
    assert seen["arena"].get("early_stop", False) is bool(flag) and "seed" in seen["arena"]
