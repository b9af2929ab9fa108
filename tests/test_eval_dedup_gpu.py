"""The request dedup on the GPU (engine.SelfPlayEngine(eval_dedup=True), xq_evdedup_*): slots that ask for the same position in
the same step share one evaluated row, bit for bit the row each would have computed, so dedup-on games are byte-identical to
dedup-off games -- eager and graph-replayed, across a weight update, plain and with tree reuse, the playout cap and the solver --
while the network runs on fewer rows.  Network: 64 channels x 1 block, the narrowest the hand-written evaluator (the one with
live_rows) runs -- a 16-channel net is refused by it --, 16 simulations."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIMS, PLIES, GAMES = 16, 30, 16
DEDUP_KEYS = ("eval_dedup_requests", "eval_dedup_merged", "eval_dedup_collisions", "eval_dedup_mismatches")


def _net(seed=0, gain=8.0):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(64, 1)
    net.load_state_dict(weights.make_state_dict(64, 1, seed=seed, policy_gain=gain))
    return net


def _records(smp, res):
    """The rings fill in the order slots finish within a step, which is not fixed: compare the records sorted."""
    return np.sort(smp, order=["slot", "game_seq", "ply"]).tobytes(), np.sort(res, order=["slot", "game_seq"]).tobytes()


def _engine_stats(st):
    return {k: v for k, v in st.items() if k not in DEDUP_KEYS and k not in ("rows_evaluated", "path", "launch", "steps", "eval_dedup")}


def test_lockstep_first_step_evaluates_one_row():
    """G = 8 slots ask for the initial position: one row is evaluated, all eight slots are handed its bits -- the bits of the
    full-width evaluation -- and the packed rows past n_live, poisoned with NaN, are never read."""
    import torch
    from xiangqi_alphazero_amd import engine, evaluator, hip
    G = 8
    ev, _ = evaluator.make_evaluator(_net(), "cuda", "hip")
    cfg = engine.make_config(G, SIMS, random_opening_moves=0, max_game_length=PLIES, seed=5)
    eng = engine.SelfPlayEngine(cfg, "cuda", evaluator=ev, eval_dedup=True)
    assert eng.path == "dedup" and eng.dedup.table_size == 32
    x = eng.select()
    torch.cuda.synchronize()
    assert (x.view(G, -1) == x.view(G, -1)[0]).all().item() and (eng.req_counts == 44).all().item()
    full_ll, full_v = ev.evaluate_legal(x, eng.req_moves, eng.req_counts)
    full_ll, full_v = full_ll.clone(), full_v.clone()
    assert not torch.isnan(full_ll).any().item() and (full_ll.view(torch.int32) == full_ll.view(torch.int32)[0]).all().item()
    sp = hip.stream_ptr(eng.device)
    hip.check(eng.lib.xq_engine_compact_unique(hip.C.byref(eng.dedup.h), hip.C.byref(eng.h), x.data_ptr(), sp), "compact_unique")
    torch.cuda.synchronize()
    assert int(eng.n_live.cpu()[0]) == 1 and int(eng.packed_rows.cpu()[0]) == 0
    assert (eng.dedup.table() == 2 ** 31 - 1).all().item()
    ll_live, v_live = ev.evaluate_legal(eng.packed_x, eng.packed_moves, eng.packed_counts, n_live=eng.n_live)
    ll = torch.full((G, hip.MAXM), float("nan"), device="cuda")
    v = torch.full((G,), float("nan"), device="cuda")
    ll[:1], v[:1] = ll_live[:1], v_live[:1]
    eng.slot_logits.fill_(float("nan"))
    eng.slot_value.fill_(float("nan"))
    eng.expand_dedup(ll, v)
    torch.cuda.synchronize()
    assert torch.equal(eng.slot_logits.view(torch.int32), full_ll.view(torch.int32))
    assert torch.equal(eng.slot_value.view(torch.int32), full_v.view(torch.int32))
    st = eng.stats()
    assert st["rows_evaluated"] == 1 and {k: st[k] for k in DEDUP_KEYS} == dict(
        eval_dedup_requests=G, eval_dedup_merged=G - 1, eval_dedup_collisions=0, eval_dedup_mismatches=0)


def _play(opts, dedup, graph, update_after=120):
    """GAMES games on GAMES slots from a lockstep start, one weight update on the way; -> (samples, results, stats)."""
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    ev, _ = evaluator.make_evaluator(_net(0), "cuda", "hip")
    cfg = engine.make_config(GAMES, SIMS, max_game_length=PLIES, random_opening_moves=0, seed=9, games_target=GAMES,
                             max_out_samples=GAMES * (PLIES + 1), max_out_results=GAMES + 8)
    eng = engine.SelfPlayEngine(cfg, "cuda", evaluator=ev, eval_dedup=dedup, **opts)
    assert eng.path == ("dedup" if dedup else "packed")
    if graph:
        assert eng.capture_step(warmup=2)
    updated = False
    for _ in range(40):
        for _ in range(60):
            if not updated and eng.steps >= update_after:
                ev.update(_net(5))
                updated = True
            eng.step()
        if eng.stats()["games_finished"] >= GAMES:
            break
    assert updated and eng.launch_mode == ("graph" if graph else "eager")
    st = eng.stats()
    assert st["games_finished"] == GAMES
    smp, res = eng.drain()
    torch.cuda.synchronize()
    return smp, res, st


OPTIONS = dict(plain={}, tree_reuse=dict(tree_reuse=True), playout_cap=dict(playout_cap=(0.5, 6)), solver=dict(solver=True))


@pytest.mark.parametrize("name", list(OPTIONS))
def test_dedup_games_identical(name):
    opts = OPTIONS[name]
    s0, r0, st0 = _play(opts, False, True)
    assert len(s0) > 0 and len(r0) == GAMES and not any(k in st0 for k in DEDUP_KEYS)
    for graph in (False, True):
        smp, res, st = _play(opts, True, graph)
        print(f"{name} {'graph' if graph else 'eager'}: rows {st0['rows_evaluated']} -> {st['rows_evaluated']}, "
              + ", ".join(f"{k[11:]} {st[k]}" for k in DEDUP_KEYS))
        assert _records(smp, res) == _records(s0, r0)
        assert _engine_stats(st) == _engine_stats(st0)
        assert st["eval_dedup_requests"] == st0["rows_evaluated"]                  # every waiting slot is keyed
        assert st["rows_evaluated"] == st["eval_dedup_requests"] - st["eval_dedup_merged"]
        assert st["eval_dedup_merged"] >= GAMES - 1                                # the lockstep first step alone
        assert st["eval_dedup_mismatches"] == 0


def test_run_games_takes_the_argument_and_the_config_key():
    from xiangqi_alphazero_amd import selfplay
    cfg = types.SimpleNamespace(num_simulations=SIMS, c_puct=1.5, temperature_threshold=15, max_game_length=PLIES,
                                random_opening_moves=0, enable_resign=True, resign_threshold=-0.85, resign_check_steps=3,
                                num_games_per_iter=GAMES)
    net = _net(1)
    s0, r0, st0, _ = selfplay.run_games(net, cfg, GAMES, "cuda", seed=3)
    s1, r1, st1, _ = selfplay.run_games(net, cfg, GAMES, "cuda", seed=3, eval_dedup=True)
    assert (st0["path"], st0["eval_dedup"], st0["eval_dedup_merged"]) == ("packed", False, 0)
    assert (st1["path"], st1["eval_dedup"], st1["launch"]) == ("dedup", True, "graph")
    assert _records(s1, r1) == _records(s0, r0) and _engine_stats(st1) == _engine_stats(st0)
    assert st1["rows_evaluated"] == st1["eval_dedup_requests"] - st1["eval_dedup_merged"] < st0["rows_evaluated"]
    cfg.eval_dedup = True
    d2, st2 = selfplay.parallel_self_play(net, cfg, seed=3, return_compact=True)
    assert st2["path"] == "dedup" and st2["eval_dedup"] is True and st2["eval_dedup_merged"] == st1["eval_dedup_merged"]
    assert _records(st2["compact_samples"], st2["compact_results"]) == _records(s0, r0)


def test_search_many_returns_the_same_visits():
    """A search-only engine: eight positions, four of them equal."""
    import os
    from oracle import xq_oracle as O
    from xiangqi_alphazero_amd import mcts
    corpus = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpus.npz"))
    picks = [i for i in range(40, 400, 7) if len(O.legal_actions(corpus["board"][i], int(corpus["side"][i])))][:5]
    order = [0, 1, 0, 2, 0, 3, 0, 4]
    games = [types.SimpleNamespace(board=corpus["board"][picks[j]].reshape(10, 9), current_player=int(corpus["side"][picks[j]]),
                                   move_count=0, no_capture_count=0, history=[]) for j in order]
    net = _net(2)
    off = mcts.MCTS(net, num_simulations=SIMS, seed=4)
    on = mcts.MCTS(net, num_simulations=SIMS, seed=4, eval_dedup=True)
    pi0 = off.search_many(games, temperature=1.0, add_noise=False)
    pi1 = on.search_many(games, temperature=1.0, add_noise=False)
    assert all(np.array_equal(a, b) for a, b in zip(pi0, pi1))
    assert all(np.array_equal(pi1[0], pi1[j]) for j in (2, 4, 6)) and not np.array_equal(pi1[0], pi1[1])
    eng0, eng1 = off._engine(8, False), on._engine(8, False)
    assert eng1.path == "dedup" and eng0.path == "packed"
    for slot in range(8):
        r0, r1 = eng0.read_root(slot), eng1.read_root(slot)
        assert r0["visits"].tolist() == r1["visits"].tolist() and r0["actions"].tolist() == r1["actions"].tolist()
    st0, st1 = eng0.stats(), eng1.stats()
    assert st1["eval_dedup_merged"] >= 3 and st1["eval_dedup_mismatches"] == 0      # the four equal roots, at the least
    assert st1["rows_evaluated"] == st0["rows_evaluated"] - st1["eval_dedup_merged"]
