"""The proven-result search on the GPU (the SOLVER instances of k_select, xq_engine_init_sv) against tests/solver_model.py.

1. whole games with injected draws equal the host model record for record -- board, actions, v (rule 5), reserved1, z, winner,
   plies -- and counter for counter: sims, terminal simulations, the tree-reuse and cap counters and the five solver counters;
   the five recorded configurations with resignation off, tree reuse off and on, the playout cap off and on;
2. search only, red king and two rooks against a bare king: N, W, sims_done and the root states equal the model for positions of
   each kind -- mate in one (an early end with sims_done < S), decided only through propagation three levels up, the lost side to
   move (the root decided against it, every child LOSS, all S simulations run, the later ones as stops), a drawn node met again;
3. solver on where nothing is decidable: byte-identical to the solver-off engine, eager and replayed from a graph;
4. device RNG, the hand-written evaluator on peaked weights: the visits of every sample and their sum over the run follow rule 5,
   the reserved1 marks are the proven moves, the evaluation cache changes nothing;
5. arena games of two stub models, with and without arena options, equal the model's; no played move is shown to lose while a
   sibling is not.
"""
import numpy as np
import pytest

import arena_openings_model as AM
import leaf_batch_model as LB
import solver_model as SM
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key
from test_arena_openings_gpu import _stub, _table
from test_hip_engine import _run_steps, _set_from_game
from test_playout_cap_gpu import _engine_cfg, _inject_array, _play_stub, _records_sha, _run
from test_solver_model import FRESH, GAMES, IDS, no_resign
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

COUNTERS = ("sims", "terminal_sims", "fast_moves", "fast_sims", "reused_visits", "reroots") + SM.COUNTERS


# ---- 1. whole games ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, 0.5], ids=["nocap", "cap"])
@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
@pytest.mark.parametrize("game", GAMES, ids=IDS)
def test_games_equal_host_model(game, reuse, cap):
    from xiangqi_alphazero_amd import engine
    c, peaked, seed, name = game
    c = no_resign(c)
    S = int(c["num_simulations"])
    cap = None if cap is None else (cap, max(1, S // 4))
    want, winner, plies, mst = SM.play_game(c, peaked, seed, tree_reuse=reuse, cap=cap)
    print(name, "reuse", reuse, "cap", cap, "plies", plies, {k: mst[k] for k in SM.COUNTERS}, "fast_early", mst["fast_early"])
    if not reuse and cap is None:                      # the games that carry the conditions (tests/test_solver_model.py)
        assert (mst["proven_nodes"], mst["proven_stops"], mst["proven_moves"]) == FRESH[name]
    assert all(0 < int(w["visits"].sum()) <= S for w in want)
    n_slots, inj_len = 2, 16384
    eng = engine.SelfPlayEngine(_engine_cfg(engine, c, n_slots, inj_len, n_slots), inject=_inject_array([seed] * n_slots, inj_len),
                                tree_reuse=reuse, playout_cap=cap, solver=True)
    assert eng.solver
    st = _play_stub(eng, peaked, n_slots)
    samples, results = eng.drain()
    assert len(results) == n_slots
    for r in results:
        assert (int(r["winner"]), int(r["steps"]), int(r["n_samples"])) == (winner, plies, len(want))
    for slot in range(n_slots):
        mine = samples[samples["slot"] == slot]
        mine = mine[np.argsort(mine["ply"], kind="stable")]
        assert len(mine) == len(want)
        for k, (s, w) in enumerate(zip(mine, want)):
            n = int(s["n_moves"])
            assert list(s["actions"][:n]) == list(w["actions"]), k
            assert list(s["visits"][:n]) == list(w["visits"]), k
            assert int(s["reserved1"]) == w["proven"] and int(s["reserved0"]) == 0, k
            assert int(s["z"]) == w["z"] and bytes(s["board"].view(np.int8)) == bytes(w["board"]), k
            assert int(s["late_temp"]) == int(w["late"]) and int(s["side"]) == w["player"], k
    assert {k: st[k] for k in COUNTERS} == {k: n_slots * mst[k] for k in COUNTERS}
    assert st["samples_written"] == n_slots * len(want) and st["moves_played"] == n_slots * len(mst["moves"])


# ---- 2. search only, crafted positions ---------------------------------------------------------------------------------------
S_SEARCH = 256


def _candidates(seed, n, player, nocap=0):
    """Red king and two rooks against a bare black king on random squares: legal, not over, `player` to move."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        rk, bk = (rng.randint(0, 3), rng.randint(3, 6)), (rng.randint(7, 10), rng.randint(3, 6))
        r1, r2 = (rng.randint(0, 10), rng.randint(0, 9)), (rng.randint(0, 10), rng.randint(0, 9))
        if len({rk, bk, r1, r2}) < 4:
            continue
        g = SM.crafted_game([(*rk, 1), (*r1, 5), (*r2, 5), (*bk, -1)], player)
        g._g.no_capture = nocap
        if g.is_game_over()[0] or O.is_in_check(g.board, -player):
            continue
        out.append(g)
    return out


@pytest.fixture(scope="module")
def crafted():
    """(game, model search) for a handful of positions: red to move, black to move, and red to move one ply short of the
    no-capture draw; plus the issue's example."""
    games = _candidates(7, 6, 1) + _candidates(8, 3, -1) + _candidates(9, 2, 1, 119)
    games.append(SM.crafted_game([(1, 5, 1), (1, 7, 5), (3, 6, 5), (7, 3, -1)]))
    out = []
    for g in games:
        n = len(g.legal_actions())
        out.append((g, SM.search_position(g, S_SEARCH, noise=np.full(n, 1.0 / n))))
    return out


def test_search_only_equals_model_on_positions_of_each_kind(crafted):
    from xiangqi_alphazero_amd import engine
    S = S_SEARCH
    kinds = dict(mate_in_one=[], deep_propagation=[], lost_side=[], draw_stop=[])
    for i, (g, s) in enumerate(crafted):
        child, root = s.root_states()
        if s.early is not None and s.sims < S and s.proven_nodes == 2:
            kinds["mate_in_one"].append(i)              # the mating leaf and the root: an early end
        if s.state[0] != SM.UNKNOWN and s.max_propagation >= 3:
            kinds["deep_propagation"].append(i)
        if root == -1 and len(child) and (child == -1).all() and s.sims == S and s.proven_stops > 0:
            kinds["lost_side"].append(i)
        if s.draw_stops > 0:
            kinds["draw_stop"].append(i)
    print({k: v for k, v in kinds.items()})
    assert all(kinds.values()), kinds                  # the model asserts each condition on at least one position
    eng = engine.SelfPlayEngine(engine.make_config(len(crafted), S, add_noise=True, manual_moves=True), solver=True)
    for slot, (g, s) in enumerate(crafted):
        n = len(g.legal_actions())
        _set_from_game(eng, slot, g, np.full(n, 1.0 / n))
    _run_steps(eng, S + 2, [False] * len(crafted), stop=eng.held)
    st = eng.stats()
    assert st["overflow"] == 0 and eng.held() and st["moves_played"] == 0
    for slot, (g, s) in enumerate(crafted):
        want, r, rs = s.root(), eng.read_root(slot), eng.read_root_states(slot)
        child, root = s.root_states()
        assert r["sims_done"] == s.sims == r["root_visits"], slot
        assert list(r["actions"]) == list(want["actions"]) and list(r["visits"]) == list(want["visits"]), slot
        np.testing.assert_array_equal(r["total_value"], want["total_value"])
        assert list(rs["children"]) == list(child) and rs["root"] == root, slot
    early = [s for _, s in crafted if s.early is not None]
    assert st["proven_nodes"] == sum(s.proven_nodes for _, s in crafted)
    assert st["proven_stops"] == sum(s.proven_stops for _, s in crafted) > 0
    assert st["proven_moves"] == len(early) > 0 and st["unspent_sims"] == sum(S - s.sims for s in early)
    assert st["sims"] == sum(s.sims for _, s in crafted) and st["terminal_sims"] == sum(s.terminal_sims for _, s in crafted)
    assert st["removed_visits"] == 0                   # a search-only engine ends no move


def test_rule_four_is_tested_ahead_of_the_budget():
    """The winning child is proven by the LAST simulation of the budget: the search still ends by rule 4, with nothing unspent."""
    from xiangqi_alphazero_amd import engine
    g = next(c for c in _candidates(7, 6, 1) if any(_mates(c, int(a)) for a in c.legal_actions()))
    n = len(g.legal_actions())
    flat = np.full(n, 1.0 / n)
    S = SM.search_position(g, S_SEARCH, noise=flat).sims             # the simulation that proves the win
    s = SM.search_position(g, S, noise=flat)
    assert s.early is not None and s.sims == S == s.budget
    eng = engine.SelfPlayEngine(engine.make_config(1, S, add_noise=True, manual_moves=True), solver=True)
    _set_from_game(eng, 0, g, flat)
    _run_steps(eng, S + 2, [False])
    st, r, rs = eng.stats(), eng.read_root(0), eng.read_root_states(0)
    assert eng.held() and r["sims_done"] == S and rs["root"] == 1 and list(rs["children"]) == list(s.root_states()[0])
    assert (st["proven_moves"], st["unspent_sims"], st["proven_nodes"]) == (1, 0, s.proven_nodes)


# ---- 3. solver on, nothing decidable -------------------------------------------------------------------------------------------
def test_nothing_decidable_is_byte_identical_to_solver_off():
    from xiangqi_alphazero_amd import engine
    ev = _TorchStub()
    n_games, sims = 2, 12
    cfg = engine.make_config(n_games, sims, seed=5, games_target=n_games, max_game_length=30)

    def play(solver, graph):
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, solver=solver)
        st = _run(eng, n_games, graph, sims)
        sha, smp, res = _records_sha(eng)
        assert len(smp) > 0 and len(res) == n_games
        return st, sha

    st_off, sha_off = play(False, False)
    for graph in (False, True):
        st, sha = play(True, graph)
        assert sha == sha_off, graph
        assert all(st[k] == 0 for k in SM.COUNTERS) and st["terminal_sims"] == 0
        assert all(st[k] == st_off[k] for k in ("sims", "moves_played", "samples_written", "nodes_created", "depth_sum"))


# ---- 4. invariants under the device RNG ------------------------------------------------------------------------------------------
def _selfplay(ev, cache_entries, n_games=16, sims=24, seed=3):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(n_games, sims, seed=seed, games_target=n_games, max_game_length=200, enable_resign=False)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, eval_cache_entries=cache_entries, solver=True)
    assert eng.capture_step() and eng.launch_mode == "graph"
    while True:                                        # at most 200 plies of sims + 1 steps each, and the start of a game
        eng.step()
        if eng.steps % 64 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 210 * (sims + 2), "games did not finish"
    st = eng.stats()
    sha, smp, res = _records_sha(eng)
    return st, sha, smp, res


def test_device_rng_invariants_and_eval_cache():
    _, ev = _hip_evaluator(policy_gain=8.0)
    S = 24
    st, sha, smp, res = _selfplay(ev, 0)
    print({k: st[k] for k in COUNTERS}, "samples", len(smp))
    assert st["overflow"] == 0 and st["games_finished"] == 16 == len(res)
    assert st["proven_nodes"] > 0                      # something was decided in these games: the run is not the solver-off one
    sums = np.array([int(s["visits"][:s["n_moves"]].sum()) for s in smp])
    assert ((sums > 0) & (sums <= S)).all()
    assert int(sums.sum()) == S * len(smp) - st["removed_visits"]
    assert int((smp["reserved1"] == 1).sum()) == st["proven_moves"]          # no playout cap: no fast move ends early
    assert set(np.unique(smp["reserved1"]).tolist()) <= {0, 1}
    assert st["sims"] == S * st["moves_played"] - st["unspent_sims"]
    st_c, sha_c, _, _ = _selfplay(ev, 64)
    assert sha_c == sha and st_c["eval_cache_hits"] > 0
    assert all(st_c[k] == st[k] for k in COUNTERS + ("moves_played", "samples_written"))


# ---- 5. arena ------------------------------------------------------------------------------------------------------------------
ARENA = dict(games=4, sims=24, max_len=200, R=2)


def _arena_openings(options):
    games, R = ARENA["games"], ARENA["R"]
    if not options:
        return None, [[]] * games
    raw = [AM.choice_stream(900 + g // 2, R) for g in range(games)]
    inject = np.zeros((games, 4, R), dtype=np.uint64)
    for g in range(games):
        inject[g, 1] = raw[g]
    return inject, [AM.opening_actions(raw[g], R) for g in range(games)]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "arena_opts"])
def arena_case(request):
    """(options, inject, the model's games): the new model (peaked stub) is red in even games.  The model asserts that the games
    show the arena's half of the feature: a move whose rule-5 choice, the first maximum of v, is not the first maximum of N."""
    options = request.param
    inject, openings = _arena_openings(options)
    pri = (LB.stub_priors(True), LB.stub_priors(False))
    want = [SM.arena_game(pri, g % 2 == 0, ARENA["sims"], ARENA["max_len"], opening=openings[g]) for g in range(ARENA["games"])]
    moves = [m for _, _, ms, _ in want for m in ms]
    total = {k: sum(w[3][k] for w in want) for k in SM.COUNTERS + ("sims",)}
    print("arena", options, total, "moves", len(moves))
    assert any(not early and i != by_n for _, _, i, by_n, early in moves)     # rule 5 changed a move that rule 4 did not end
    assert total["proven_nodes"] > 0 and total["proven_stops"] > 0 and total["removed_visits"] > 0
    if not options:
        assert total["proven_moves"] > 0
    for _, child, i, _, _ in moves:                    # no played move is shown to lose while a sibling is not
        assert child[i] != -1 or (child == -1).all()
    return options, inject, want, total


def _play_recording_moves(eng, new_is_red):
    """Steps an arena engine with the two stub models (dense protocol) and reads every played move off the slots' boards ->
    per slot the actions played after the first root request (the opening, when there is one, comes before it)."""
    import torch
    from xiangqi_alphazero_amd import hip
    boards_view = eng.arena_views()["board"]
    cache, moves, prev = {}, [[] for _ in range(eng.G)], None
    for step in range(60000):
        x = eng.select().cpu().numpy()
        counts = eng.req_counts.cpu().numpy()
        ints = eng.slot_ints.cpu().numpy()
        boards = boards_view[:, :90].cpu().numpy()
        mc, side = ints[:, hip.GI_MC], ints[:, hip.GI_SIDE]
        if prev is not None:
            for slot in range(eng.G):
                if mc[slot] == prev[0][slot] + 1:
                    changed = np.nonzero(boards[slot] != prev[1][slot])[0]
                    assert len(changed) == 2, (slot, step)
                    frm = [int(q) for q in changed if boards[slot][q] == 0]
                    assert len(frm) == 1
                    to = int(changed[0] + changed[1]) - frm[0]
                    moves[slot].append(frm[0] * 90 + to)
                else:
                    assert mc[slot] == prev[0][slot], (slot, step)
        prev = (mc.copy(), boards.copy())
        probs = np.zeros((eng.rows, 8100), dtype=np.float32)
        vals = np.zeros(eng.rows, dtype=np.float32)
        for r in np.nonzero(counts > 0)[0]:
            peaked = bool((side[r] == 1) == new_is_red[r])        # the searching model: the new one is the peaked stub
            key = (state_key(x[r]), peaked)
            if key not in cache:
                cache[key] = predict_from_key(*key)
            probs[r], vals[r] = cache[key]
        eng.expand(torch.from_numpy(probs).cuda(), torch.from_numpy(vals).cuda(), is_probs=True)
        if step % 32 == 31 and eng.stats()["games_finished"] >= eng.G:
            break
    return moves


def test_arena_moves_equal_model(arena_case):
    """An arena engine stepped by hand: every played move, the results and the counters equal the model's."""
    from xiangqi_alphazero_amd import engine
    options, inject, want, total = arena_case
    games, sims, max_len, R = (ARENA[k] for k in ("games", "sims", "max_len", "R"))
    cfg = engine.make_config(games, sims, max_game_length=max_len, random_opening_moves=0, enable_resign=False, add_noise=False,
                             games_target=games, manual_moves=2, inject_len=R if options else 0)
    eng = engine.arena_engine(cfg, "cuda", R, 0, inject, solver=True) if options else engine.SelfPlayEngine(cfg, solver=True)
    assert eng.solver and (eng.arena_opts is not None) == options
    moves = _play_recording_moves(eng, [g % 2 == 0 for g in range(games)])
    st = eng.stats()
    _, res = eng.drain()
    assert st["overflow"] == 0 and len(res) == games
    assert _table(res[res["slot"].argsort()]) == [(w, plies) for w, plies, _, _ in want]
    for slot in range(games):
        assert moves[slot] == [m[0] for m in want[slot][2]], slot
    assert {k: st[k] for k in total} == total


def test_play_arena_with_solver_equals_model(arena_case):
    """arena.play_arena(solver=True): the model's results; with arena options (`info`) its counters as well."""
    from xiangqi_alphazero_amd import arena
    options, inject, want, total = arena_case
    kw = dict(opening_plies=ARENA["R"], inject=inject, info={}) if options else {}
    res = arena.play_arena(_stub(True), _stub(False), ARENA["games"], ARENA["sims"], ARENA["max_len"], policy_is_probs=True,
                           solver=True, **kw)
    assert _table(res) == [(w, plies) for w, plies, _, _ in want]
    if options:
        st = kw["info"]["stats"]
        assert st["overflow"] == 0 and {k: st[k] for k in total} == total


# ---- the serving shim ------------------------------------------------------------------------------------------------------------
def test_mcts_get_action_returns_the_proven_win():
    """MCTS(solver=True).get_action at temperature 0 under a flat evaluator: a position with a mate in one gives a mating move."""
    import types

    import torch
    from xiangqi_alphazero_amd import mcts

    def flat(x):
        return torch.zeros((x.shape[0], 8100), device=x.device), torch.zeros(x.shape[0], device=x.device)

    g = next(c for c in _candidates(7, 6, 1) if any(_mates(c, int(a)) for a in c.legal_actions()))
    pos = types.SimpleNamespace(board=g.board.copy(), current_player=1, move_count=0, no_capture_count=0, history=[])
    m = mcts.MCTS(flat, num_simulations=64, solver=True)
    a = m.get_action(pos, temperature=0.0, add_noise=False)
    assert _mates(g, a)
    eng = m._engine(1, False)
    r, rs = eng.read_root(0), eng.read_root_states(0)
    assert rs["root"] == 1 and r["sims_done"] < 64 and int(r["actions"][list(rs["children"]).index(1)]) == a
    assert eng.solver_stats()["proven_moves"] == 1


def _mates(g, action):
    h = g.clone()
    h.make_action(action)
    over, winner = h.is_game_over()
    return bool(over) and winner == g.current_player
