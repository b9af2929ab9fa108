"""CPU checks of the perpetual-check rule's ABI (include/xq_hip.h, xq_rules_opts): exports and header text, rules == NULL and
perpetual_check = 0 being xq_engine_init_ar, no workspace of its own, every refusal returned before any launch, and the Python
layer: the flag joins the one option path with every other option, and the config key reaches self-play and the gate alike."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_engine_workspace_bytes_ru", "xq_engine_init_ru", "xq_game_over_batch_ex")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _bad_rules(hip):
    out = [("perpetual_check 2", hip.RulesOpts(2)), ("perpetual_check -1", hip.RulesOpts(-1))]
    for i in range(3):
        r = hip.RulesOpts(1)
        r.reserved[i] = 1
        out.append((f"reserved[{i}]", r))
    return out


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    assert "typedef struct xq_rules_opts { int32_t perpetual_check; int32_t reserved[3]; } xq_rules_opts;" in header
    assert C.sizeof(hip.RulesOpts) == 16 and hip.RulesOpts.reserved.offset == 4
    assert C.sizeof(hip.Engine) == 384 and C.sizeof(hip.EngineConfig) == 112          # the handle and the config are as they were
    assert C.sizeof(hip.EngineStats) == 256
    for phrase in ("entry e = 0, 1, ... = the board e + 1 plies ago", "E = the oldest entry of the window that equals the current board",
                   "exactly one of the two holds: that side loses", "5 repetition draw, 6 perpetual-check loss",
                   "rules == NULL or perpetual_check = 0 is xq_engine_init_ar exactly", "Chase rules",
                   "4 rules: repetition, perpetual check"):
        assert phrase in header, phrase
    assert len(hip.OVER_KINDS) == 7 and hip.OVER_KINDS[6] == "perpetual_check"


def test_rules_null_and_zero_are_init_ar():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    gz, ar, cap, fp = hip.Gumbel(16, 0, 50.0, 1.0), hip.ArenaOpts(4, 0), hip.PlayoutCap(10, 0, 0.25), hip.ForcedPlayouts(2.0)
    ref = lambda x: None if x is None else C.byref(x)
    cases = [(engine.make_config(64, 100), 1, 0, None, None, None, None), (engine.make_config(64, 100), 4, 0, None, None, None, None),
             (engine.make_config(64, 100), 1, 1, cap, fp, None, None), (engine.make_config(8, 24, manual_moves=1), 1, 0, None, None, gz, None),
             (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, ar), (engine.make_config(8, 24, manual_moves=2), 1, 0, None, None, None, None)]
    for cfg, K, flags, c, f, g, a in cases:
        want = lib.xq_engine_workspace_bytes_ar(C.byref(cfg), K, flags, ref(c), ref(f), ref(g), ref(a))
        assert want > 0
        for rules in (None, hip.RulesOpts(0), hip.RulesOpts(1)):                 # the rule adds no workspace either
            assert lib.xq_engine_workspace_bytes_ru(C.byref(cfg), K, flags, ref(c), ref(f), ref(g), ref(a), ref(rules)) == want
        for what, bad in _bad_rules(hip):
            assert lib.xq_engine_workspace_bytes_ru(C.byref(cfg), K, flags, ref(c), ref(f), ref(g), ref(a), C.byref(bad)) == 0, what
    # what xq_engine_init_ar refuses stays refused with the rule on
    ok, on = engine.make_config(8, 50), hip.RulesOpts(1)
    for cfg2, K, flags in ((ok, 1, 2), (ok, 2, 1), (ok, 0, 0), (engine.make_config(8, 50, manual_moves=2), 2, 0)):
        assert lib.xq_engine_workspace_bytes_ru(C.byref(cfg2), K, flags, None, None, None, None, C.byref(on)) == 0


def test_init_ru_rejects_bad_arguments_before_any_launch():
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    fake_ws = C.c_void_p(1 << 20)                      # never dereferenced: the argument checks come first
    h, cfg, on = hip.Engine(), engine.make_config(8, 50), hip.RulesOpts(1)
    for what, bad in _bad_rules(hip):
        assert lib.xq_engine_init_ru(C.byref(h), C.byref(cfg), 1, 0, None, None, None, None, C.byref(bad), fake_ws, 1 << 40, None,
                                     None) == -1, what
    assert lib.xq_engine_init_ru(None, C.byref(cfg), 1, 0, None, None, None, None, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_ru(C.byref(h), None, 1, 0, None, None, None, None, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_ru(C.byref(h), C.byref(cfg), 1, 0, None, None, None, None, C.byref(on), None, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_ru(C.byref(h), C.byref(cfg), 1, 0, None, None, None, None, C.byref(on), C.c_void_p((1 << 20) + 8),
                                 1 << 40, None, None) == -1                     # workspace not 256-byte aligned
    inj = engine.make_config(8, 50, inject_len=4)
    assert lib.xq_engine_init_ru(C.byref(h), C.byref(inj), 1, 0, None, None, None, None, C.byref(on), fake_ws, 1 << 40, None, None) == -1
    assert lib.xq_engine_init_ru(C.byref(h), C.byref(cfg), 1, 0, None, None, None, None, C.byref(on), fake_ws, 16, None, None) == -3   # XQ_ERR_WORKSPACE


def test_game_over_batch_ex_rejects_bad_arguments_before_any_launch():
    hip, lib = _lib()
    one, on = C.c_void_p(256), hip.RulesOpts(1)
    args = [one, one, one, one, one]
    assert lib.xq_game_over_batch_ex(*args, -1, C.byref(on), one, one, None) == -1
    for i in range(5):
        a = list(args)
        a[i] = None
        assert lib.xq_game_over_batch_ex(*a, 4, C.byref(on), one, one, None) == -1, i
    assert lib.xq_game_over_batch_ex(*args, 4, C.byref(on), None, one, None) == -1          # dev_out is required, dev_kind is not
    for what, bad in _bad_rules(hip):
        assert lib.xq_game_over_batch_ex(*args, 4, C.byref(bad), one, one, None) == -1, what
        assert lib.xq_game_over_batch_ex(*args, 0, C.byref(bad), one, one, None) == -1, what
    # n = 0 is a no-op, with or without rules and pointers
    assert lib.xq_game_over_batch_ex(None, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.xq_game_over_batch_ex(None, None, None, None, None, 0, C.byref(on), None, None, None) == 0


OTHERS = [("plain", {}, {}), ("leaves", {}, dict(leaves_per_step=4)), ("tree_reuse", {}, dict(tree_reuse=True)),
          ("playout_cap", {}, dict(playout_cap=(0.25, 8))), ("forced_playouts", {}, dict(forced_playouts=2.0)),
          ("reuse_cap_forced_cache", {}, dict(tree_reuse=True, playout_cap=(0.25, 8), forced_playouts=2.0, eval_cache_entries=64)),
          ("gumbel", {}, dict(gumbel=(16, 50.0, 1.0))), ("gumbel_search_only", dict(manual_moves=1), dict(gumbel=(8, 50.0, 1.0))),
          ("search_only_leaves", dict(manual_moves=1), dict(leaves_per_step=8)), ("arena", dict(manual_moves=2), {}),
          ("arena_opts", dict(manual_moves=2), dict(arena_opts=(4, 0)))]


@pytest.mark.parametrize("name,cfg_kw,kw", OTHERS, ids=[c[0] for c in OTHERS])
def test_parse_engine_options_accepts_the_flag_with_each_other_option(name, cfg_kw, kw):
    from xiangqi_alphazero_amd import engine
    hip, lib = _lib()
    cfg = engine.make_config(**{**dict(n_games=4, num_simulations=32), **cfg_kw})
    off, on = engine.parse_engine_options(cfg, **kw), engine.parse_engine_options(cfg, perpetual_check=True, **kw)
    assert off.rules is None and engine.parse_engine_options(cfg, perpetual_check=False, **kw).rules is None
    assert isinstance(on.rules, hip.RulesOpts) and bytes(on.rules) == bytes(hip.RulesOpts(1))
    assert len(on) == 6 and on[:2] == off[:2]                       # the tuple stays the argument list of xq_engine_*_ar
    for a, b in zip(on[2:], off[2:]):
        assert (a is None) == (b is None) and (a is None or bytes(a) == bytes(b))
    refs = [None if s is None else C.byref(s) for s in on[2:]]
    n = lib.xq_engine_workspace_bytes_ru(C.byref(cfg), on.K, on.flags, *refs, C.byref(on.rules))
    assert n > 0 and n == lib.xq_engine_workspace_bytes_ar(C.byref(cfg), on.K, on.flags, *refs)


def test_python_refuses_a_flag_that_is_no_bool():
    from xiangqi_alphazero_amd import engine, hip
    for bad in (2, "yes", 0.5, None):
        with pytest.raises(hip.XqError, match="perpetual_check"):
            engine.parse_engine_options(engine.make_config(4, 32), perpetual_check=bad)


def test_signatures_default_to_off():
    from xiangqi_alphazero_amd import arena, engine, hip, mcts, selfplay
    for fn in (engine.parse_engine_options, engine.SelfPlayEngine.__init__, engine.arena_engine, mcts.MCTS.__init__, arena.play_arena,
               hip.game_over_batch):
        assert inspect.signature(fn).parameters["perpetual_check"].default is False, fn
    for fn in (selfplay.run_games, selfplay.parallel_self_play, arena.evaluate_models):          # None: the config decides
        assert inspect.signature(fn).parameters["perpetual_check"].default is None, fn
    assert inspect.signature(hip.game_over_batch).parameters["return_kind"].default is False
    assert engine.RULES_REASONS == (1, 4)


def _arena_config(**kw):
    base = dict(eval_games=6, eval_simulations=8, max_game_length=20, c_puct=1.5, eval_win_rate=0.55)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_evaluate_models_reads_the_config_key_once_and_passes_it_on(monkeypatch):
    from xiangqi_alphazero_amd import arena
    from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE
    seen = []

    def fake_play_arena(en, eo, n, sims, maxlen, c_puct, device, policy_is_probs=False, first_game=0, **kw):
        seen.append(kw)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        res["slot"], res["steps"], res["winner"] = np.arange(n), 9, 1
        if "info" in kw:
            kw["info"]["openings"] = np.zeros((n, 16), dtype=np.uint16)
        return res

    monkeypatch.setattr(arena, "play_arena", fake_play_arena)
    monkeypatch.setattr(arena.ev_mod, "make_evaluator", lambda net, device, kind: (None, "fake"))
    out = arena.evaluate_models("new", "old", _arena_config(perpetual_check_loses=True), "cpu")
    assert seen[-1] == {"perpetual_check": True} and out["perpetual_check"] is True
    out = arena.evaluate_models("new", "old", _arena_config(perpetual_check_loses=True, arena_opening_plies=2), "cpu")
    assert seen[-1]["perpetual_check"] is True and seen[-1]["opening_plies"] == 2
    out = arena.evaluate_models("new", "old", _arena_config(perpetual_check_loses=False), "cpu")
    assert seen[-1] == {} and "perpetual_check" not in out                      # off: the reference's gate, called as before
    arena.evaluate_models("new", "old", _arena_config(), "cpu", perpetual_check=True)           # the argument wins over the config
    assert seen[-1] == {"perpetual_check": True}
    arena.evaluate_models("new", "old", _arena_config(perpetual_check_loses=True), "cpu", perpetual_check=False)
    assert seen[-1] == {}


@pytest.mark.parametrize("flag", [True, False, None], ids=["on", "off", "absent"])
def test_loop_trains_and_gates_under_one_rule(monkeypatch, tmp_path, flag):
    """An AlphaZeroLoop reads config.perpetual_check_loses once and hands that one value to self-play and to the arena gate."""
    import torch
    from xiangqi_alphazero_amd import arena, selfplay, train_loop
    cfg = types.SimpleNamespace(
        num_channels=16, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=4,
        max_game_length=30, random_opening_moves=2, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
        learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40, min_buffer_size=4,
        num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55, save_interval=2, num_iterations=1,
        checkpoint_dir=str(tmp_path))
    if flag is not None:
        cfg.perpetual_check_loses = flag
    seen = {}

    def fake_run_games(model, config, n, device, **kw):
        seen["selfplay"] = kw["perpetual_check"]
        return torch.empty((0, 640), dtype=torch.uint8), torch.empty((0, 16), dtype=torch.uint8), {}, 0.0

    def fake_evaluate_models(new, old, config, device, kind, **kw):
        seen["arena"] = kw["perpetual_check"]
        return {"model_updated": False}

    monkeypatch.setattr(selfplay, "run_games", fake_run_games)
    monkeypatch.setattr(arena, "evaluate_models", fake_evaluate_models)
    loop = train_loop.AlphaZeroLoop(cfg, device="cpu", seed=1)
    loop._play_shard(4)
    loop._arena()
    cfg.arena_opening_plies = 2                        # the paired-openings branch of the gate passes it as well
    cfg.perpetual_check_loses = not flag               # ... and a later change of the config does not split the loop
    loop._arena()
    assert seen == {"selfplay": bool(flag), "arena": bool(flag)} and loop.perpetual_check is bool(flag)
