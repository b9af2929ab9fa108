"""The opt-in perpetual-check rule on the GPU (xq_rules_opts: xq_game_over_batch_ex, xq_engine_init_ru).

* xq_game_over_batch_ex equals the host model (tests/perpetual_check_model.py) on every fixture of the rule and on the corpus, rule
  on and off, done / winner / kind, at n = 1, WPW - 1, WPW + 1 and a few hundred mixed boards; rules = NULL is xq_game_over_batch;
* the root of a search-only engine at PC-red / PC-black ply 12 has status 4 and the checked side as winner (off: 1 and a draw);
* at the leaves (k_select, and k_select_multi at K = 4) the repeating child is backed up like a mate, takes more visits than under
  the reference's draw, and every search equals the host model bit for bit; a checker that completes its own perpetual loses;
* off is off: an engine through xq_engine_init_ru(NULL) and through xq_engine_init_ar plays byte-identical games;
* on runs clean: alone and with tree reuse plus the evaluation cache, eager and replayed from a graph;
* play_arena with the flag builds rule-on engines.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import golden_io as G
import perpetual_check_model as M
from test_playout_cap_gpu import _inject_array, _records_sha, _run
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

WPW = 4            # positions per workgroup of k_game_over (csrc/xq_batch.hip)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _batch_cases():
    """[(name, board, side, move_count, no_capture, hist[12, 90] oldest first and zero padded)] with the model's verdicts
    (kind, winner) off and on, computed once."""
    states = []
    for name, make in (("pc_red", M.pc_red), ("pc_black", M.pc_black), ("quiet", M.quiet), ("pc_red_rotated", M.pc_red_rotated)):
        for plies in range(13):
            states.append((f"{name}@{plies}", M.state_of(make(plies))))
    states += [(name, state) for name, state, _, _ in M.synthetic_cases()]
    board, side, mc, nc, hist = M.state_of(M.pc_red(12))
    for name, sq in (("black_king_missing", 9 * 9 + 4), ("red_king_missing", 3)):      # king capture precedes everything
        b = board.copy()
        b[sq] = 0
        states.append((name, (b, side, mc, nc, hist)))
    d = G.corpus()
    for i in sorted(set(np.nonzero(d["done"])[0].tolist()) | set(range(0, len(d["board"]), 9))):
        states.append((f"corpus{i}", (d["board"][i], int(d["side"][i]), int(d["move_count"][i]), int(d["no_capture"][i]),
                                      G.history_tail(d, i))))
    out = []
    for name, (board, side, mc, nc, hist) in states:
        h = np.zeros((12, 90), dtype=np.int8)
        hist = np.asarray(hist, dtype=np.int8).reshape(-1, 90)
        h[:len(hist)] = hist
        out.append(dict(name=name, board=np.asarray(board, dtype=np.int8).reshape(90), side=side, mc=mc, nc=nc, hist=h,
                        off=M.verdict(board, side, mc, nc, hist, False), on=M.verdict(board, side, mc, nc, hist, True)))
    return out


def _pick(names):
    by = {c["name"]: c for c in _batch_cases()}
    return [by[n] for n in names]


BATCHES = {"n1": ["pc_red@12"], "wpw_minus_1": ["quiet@12", "pc_black@12", "short_span"],
           "wpw_plus_1": ["pc_red@11", "both_check", "ply_200", "one_quiet_move", "pc_red_rotated@12"], "mixed": None}


@pytest.mark.parametrize("batch", list(BATCHES), ids=list(BATCHES))
def test_game_over_batch_ex_equals_the_model(batch):
    from xiangqi_alphazero_amd import hip
    cases = _batch_cases() if BATCHES[batch] is None else _pick(BATCHES[batch])
    n = len(cases)
    assert n == {"n1": 1, "wpw_minus_1": WPW - 1, "wpw_plus_1": WPW + 1}.get(batch, n) and (batch != "mixed" or n > 200)
    args = (_t(np.stack([c["board"] for c in cases])), _t(np.array([c["side"] for c in cases], dtype=np.int8)),
            _t(np.array([c["mc"] for c in cases], dtype=np.int32)), _t(np.array([c["nc"] for c in cases], dtype=np.int32)),
            _t(np.stack([c["hist"] for c in cases])))
    plain = hip.game_over(*args).cpu().numpy()
    for rule in ("off", "on"):
        out, kind = hip.game_over_batch(*args, perpetual_check=rule == "on", return_kind=True)
        out, kind = out.cpu().numpy(), kind.cpu().numpy()
        for i, c in enumerate(cases):
            want_kind, want_winner = c[rule]
            assert (int(out[i, 0]), int(out[i, 1]), int(kind[i])) == (int(want_kind != M.NOT_OVER), want_winner, want_kind), (c["name"], rule)
        if rule == "off":
            assert out.tobytes() == plain.tobytes()
    assert hip.game_over_batch(*args).cpu().numpy().tobytes() == plain.tobytes()           # rules = NULL, no kind
    if batch == "mixed":                                # the mix holds every ending, and the rule changes some verdicts
        assert {c["on"][0] for c in cases} == set(range(7))
        assert sum(c["on"] != c["off"] for c in cases) >= 4


def _search_engine(n_slots, sims, K, perpetual):
    from xiangqi_alphazero_amd import engine
    return engine.SelfPlayEngine(engine.make_config(n_slots, sims, add_noise=False, manual_moves=True), leaves_per_step=K,
                                 perpetual_check=perpetual)


def _set(eng, slot, g):
    eng.set_position(slot, g.board, g.current_player, g.move_count, g.no_capture_count, g.history()[-12:])


def _uniform_steps(eng, max_steps):
    """Dense-protocol steps with the uniform stub (probability 1/8100 everywhere, value 0) until every slot holds."""
    import torch
    probs = torch.full((eng.rows, 8100), 1.0 / 8100.0, dtype=torch.float32, device="cuda")
    vals = torch.zeros(eng.rows, dtype=torch.float32, device="cuda")
    for _ in range(max_steps):
        eng.select()
        eng.expand(probs, vals, is_probs=True)
        if eng.held():
            return
    raise AssertionError("search did not finish")


@pytest.mark.parametrize("perpetual", [True, False], ids=["on", "off"])
def test_root_verdict(perpetual):
    from xiangqi_alphazero_amd import hip
    eng = _search_engine(2, 8, 1, perpetual)
    assert eng.perpetual_check is perpetual
    _set(eng, 0, M.pc_red(12))
    _set(eng, 1, M.pc_black(12))
    eng.select()
    status = eng.slot_ints[:, hip.GI_RSTATUS].cpu().tolist()
    winner = eng.slot_ints[:, hip.GI_RWINNER].cpu().tolist()
    assert (status, winner) == (([4, 4], [-1, 1]) if perpetual else ([1, 1], [0, 0]))
    _uniform_steps(eng, 2)                              # the terminal root is never searched
    assert eng.stats()["overflow"] == 0 and [eng.read_root(s)["sims_done"] for s in (0, 1)] == [0, 0]


def _hexes(x):
    return [float(v).hex() for v in x]


@pytest.mark.parametrize("K", [1, 4], ids=["k_select", "k_select_multi"])
def test_leaf_verdict_in_the_descent(K):
    sims = 64
    games = [M.pc_red(11), M.cycle_game(M.MATE_IN_ONE, [], 0), M.pc_red_rotated(11), M.quiet(11)]
    roots = {}
    for perpetual in (False, True):
        eng = _search_engine(len(games), sims, K, perpetual)
        for s, g in enumerate(games):
            _set(eng, s, g)
        _uniform_steps(eng, sims + 8)
        assert eng.stats()["overflow"] == 0
        for s, g in enumerate(games):
            r = eng.read_root(s)
            want = M.search(g, sims, K, M.uniform_priors, perpetual)
            assert r["sims_done"] == sims and r["root_visits"] == want["root_visits"], (s, perpetual)
            assert list(r["actions"]) == list(want["actions"]) and list(r["visits"]) == list(want["visits"]), (s, perpetual)
            assert _hexes(r["total_value"]) == _hexes(want["total_value"]) and _hexes(r["prior"]) == _hexes(want["prior"]), (s, perpetual)
            roots[perpetual, s] = r
    rep = M.PC_RED_CYCLE[3]                             # K -> (9,4): the third repetition, red has checked throughout
    off, on = roots[False, 0], roots[True, 0]
    assert sorted(on["actions"].tolist()) == sorted([rep, 76 * 90 + 67])
    i = list(on["actions"]).index(rep)
    assert off["total_value"][i] == 0.0 and off["visits"][i] > 0
    assert on["total_value"][i] == on["visits"][i] > off["visits"][i]
    mate = roots[True, 1]
    j = list(mate["actions"]).index(M.MATE_MOVE)
    assert mate["total_value"][j] == mate["visits"][j] > 0                     # the sign of a mating child
    rot = roots[True, 2]                                # red's own check would complete its perpetual: that child loses
    k = list(rot["actions"]).index(M.PC_RED_CYCLE[0])
    assert rot["visits"][k] > 0 and rot["total_value"][k] == -rot["visits"][k]
    assert roots[False, 2]["total_value"][k] == 0.0


N_GAMES, SIMS, INJ = 8, 16, 8192


def _selfplay_cfg(engine, inject):
    return engine.make_config(N_GAMES, SIMS, games_target=N_GAMES, max_game_length=40, inject_len=INJ if inject else 0, seed=11)


def test_off_is_off():
    import torch
    from xiangqi_alphazero_amd import engine, hip
    ev = _TorchStub()
    cfg = _selfplay_cfg(engine, True)
    inject = _inject_array([300 + s for s in range(N_GAMES)], INJ)

    def run(how):
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, inject=inject)
        assert not eng.perpetual_check
        base = (eng.ws.data_ptr() + 255) & ~255
        args = (base, eng.workspace_bytes, eng._inject.data_ptr(), hip.stream_ptr(eng.device))
        if how == "init_ru_null":
            assert eng.lib.xq_engine_workspace_bytes_ru(C.byref(cfg), 1, 0, None, None, None, None, None) == eng.workspace_bytes
            hip.check(eng.lib.xq_engine_init_ru(C.byref(eng.h), C.byref(cfg), 1, 0, None, None, None, None, None, *args), "xq_engine_init_ru")
        elif how == "init_ru_zero":
            zero = hip.RulesOpts(0)
            hip.check(eng.lib.xq_engine_init_ru(C.byref(eng.h), C.byref(cfg), 1, 0, None, None, None, None, C.byref(zero), *args),
                      "xq_engine_init_ru")
        elif how == "init_ar":
            hip.check(eng.lib.xq_engine_init_ar(C.byref(eng.h), C.byref(cfg), 1, 0, None, None, None, None, *args), "xq_engine_init_ar")
        torch.cuda.synchronize()
        st = _run(eng, N_GAMES, False, SIMS)
        sha, smp, res = _records_sha(eng)
        assert len(smp) > 0 and len(res) == N_GAMES and set(res["reason"].tolist()) <= {1, 2, 3}
        return sha, st

    want = run("init_ar")
    assert run("init_ru_null") == want and run("init_ru_zero") == want and run("constructor") == want


def _check_results(res, st):
    assert st["overflow"] == 0 and st["games_finished"] == N_GAMES == len(res)
    assert set(res["reason"].tolist()) <= {1, 2, 3, 4}
    assert all(int(r["winner"]) != 0 for r in res if int(r["reason"]) == 4)


@pytest.mark.parametrize("combo", ["alone", "reuse_and_cache"])
def test_on_runs_clean_and_replays(combo):
    from xiangqi_alphazero_amd import engine
    if combo == "alone":
        ev, kw = _TorchStub(), {}
    else:
        ev, kw = _hip_evaluator()[1], dict(tree_reuse=True, eval_cache_entries=64)
    shas = []
    for graph in (False, True):
        eng = engine.SelfPlayEngine(_selfplay_cfg(engine, False), evaluator=ev, perpetual_check=True, **kw)
        assert eng.perpetual_check and (eng.h.pad0 >> 26) & 1 == 1
        st = _run(eng, N_GAMES, graph, SIMS)
        sha, smp, res = _records_sha(eng)
        _check_results(res, st)
        assert len(smp) > 0
        shas.append(sha)
    assert shas[0] == shas[1]


@pytest.mark.parametrize("openings", [0, 2], ids=["plain", "arena_opts"])
def test_play_arena_builds_rule_on_engines(monkeypatch, openings):
    from xiangqi_alphazero_amd import arena, engine
    from test_arena_openings_gpu import _stub
    made = []

    class Spy(engine.SelfPlayEngine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(engine, "SelfPlayEngine", Spy)
    for flag in (True, False):
        res = arena.play_arena(_stub(True), _stub(False), 2, 8, 12, policy_is_probs=True, opening_plies=openings, seed=3,
                               perpetual_check=flag)
        assert len(res) == 2 and set(res["reason"].tolist()) <= {1, 2, 4}
    assert [e.perpetual_check for e in made] == [True, False]
    assert [(e.h.pad0 >> 26) & 1 for e in made] == [1, 0] and all((e.arena_opts is not None) == (openings > 0) for e in made)
