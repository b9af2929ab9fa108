"""GPU checks of the arena options (include/xq_hip.h, xq_engine_init_ar): with no opening the games are the reference's recorded
ones; injected and device-drawn openings are pairwise equal, distinct between pairs, shard-independent, and every game equals the
host model (tests/arena_openings_model.py) replayed from the recorded opening; the per-model packed step plays the games of the
masked and of the dense step and evaluates every request exactly once; the partition itself, slot by slot and bit for bit."""
import numpy as np
import pytest

import arena_openings_model as AM
import golden_io as G
from oracle import xq_oracle as O
from stub_eval import StubEvaluator, predict_from_key, state_key

pytestmark = pytest.mark.gpu


def _stub(peaked):
    """Dense-protocol stub evaluator over the engine's planes (probabilities: policy_is_probs=True)."""
    import torch
    cache = {}

    def f(x):
        xs = x.cpu().numpy()
        p = np.empty((xs.shape[0], 8100), dtype=np.float32)
        v = np.empty(xs.shape[0], dtype=np.float32)
        for i in range(xs.shape[0]):
            k = state_key(xs[i])
            if k not in cache:
                cache[k] = predict_from_key(k, peaked)
            p[i], v[i] = cache[k]
        return torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
    return f


def _table(res):
    return [(int(r["winner"]), int(r["steps"])) for r in res]


def _host_table(openings, counts, first_game, sims, max_len, new_peaked=True):
    new, old = O.make_eval(StubEvaluator(peaked=new_peaked).predict), O.make_eval(StubEvaluator(peaked=not new_peaked).predict)
    out = []
    for s in range(len(counts)):
        out.append(AM.play_game([int(a) for a in openings[s, :counts[s]]], new, old, (first_game + s) % 2 == 0, sims, max_len))
    return out


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_off_is_off(name):
    """xq_engine_init_ar with opening_plies = 0 (an arena-options engine: `info` asks for one), dense stubs: the reference's games."""
    from xiangqi_alphazero_amd import arena
    t = [x for x in G.arena_traces() if x["name"] == name][0]
    info = {}
    res = arena.play_arena(_stub(t["new_peaked"]), _stub(not t["new_peaked"]), t["eval_games"], t["eval_simulations"],
                           t["max_game_length"], policy_is_probs=True, opening_plies=0, info=info)
    assert [int(r["slot"]) for r in res] == list(range(t["eval_games"]))
    assert _table(res) == [(g["winner"], g["steps"]) for g in t["games"]]
    assert not info["opening_counts"].any() and not info["openings"].any() and info["stats"]["overflow"] == 0


def test_injected_openings_equal_the_host_model():
    from xiangqi_alphazero_amd import arena
    games, R, sims, max_len = 8, 3, 16, 40
    inject = np.zeros((games, 4, R), dtype=np.uint64)
    raw = [AM.choice_stream(500 + g // 2, R) for g in range(games)]          # partners: the same stream
    for g in range(games):
        inject[g, 1] = raw[g]
    info = {}
    res = arena.play_arena(_stub(True), _stub(False), games, sims, max_len, policy_is_probs=True, opening_plies=R, inject=inject,
                           info=info)
    want = [AM.opening_actions(raw[g], R) for g in range(games)]
    assert info["stats"]["overflow"] == 0
    for g in range(games):
        n = int(info["opening_counts"][g])
        assert n == len(want[g]) == R and info["openings"][g, :n].tolist() == want[g], g
        assert not info["openings"][g, n:].any()
    for p in range(games // 2):
        assert info["openings"][2 * p].tolist() == info["openings"][2 * p + 1].tolist()
    assert len({tuple(o) for o in want}) == games // 2                       # four streams, four openings
    assert _table(res) == _host_table(info["openings"], info["opening_counts"], 0, sims, max_len)
    assert all(s >= R for _, s in _table(res))


def test_device_rng_openings():
    from xiangqi_alphazero_amd import arena, engine
    games, R, sims, max_len = 64, 4, 8, 12
    info = {}
    res = arena.play_arena(_stub(True), _stub(False), games, sims, max_len, policy_is_probs=True, opening_plies=R, seed=11, info=info)
    op, cnt = info["openings"], info["opening_counts"]
    assert info["stats"]["overflow"] == 0 and set(cnt.tolist()) <= {0, R}
    for p in range(games // 2):
        assert op[2 * p].tolist() == op[2 * p + 1].tolist() and cnt[2 * p] == cnt[2 * p + 1]
    assert len({tuple(op[2 * p].tolist()) for p in range(games // 2)}) >= 30          # not one opening for all
    # every opening is a line of legal moves from the initial position
    for p in range(games // 2):
        g = O.Game()
        for a in op[2 * p, :cnt[2 * p]]:
            assert int(a) in g.legal_actions().tolist()
            g.make_action(int(a))
    full = _table(res)
    assert full == _host_table(op, cnt, 0, sims, max_len)
    # a shard that starts on an odd game index plays the same games
    info1 = {}
    res1 = arena.play_arena(_stub(True), _stub(False), 5, sims, max_len, policy_is_probs=True, opening_plies=R, seed=11, first_game=1,
                            info=info1)
    assert info1["openings"].tolist() == op[1:6].tolist() and _table(res1) == full[1:6]
    # another seed, other openings (one select starts every game: no need to play them)
    cfg = engine.make_config(games, sims, max_game_length=max_len, random_opening_moves=0, enable_resign=False, add_noise=False,
                             games_target=games, manual_moves=2, seed=12)
    eng = engine.SelfPlayEngine(cfg, arena_opts=(R, 0))
    eng.select()
    op2, cnt2 = eng.arena_openings()
    assert set(cnt2.tolist()) <= {0, R} and sum(op2[g].tolist() != op[g].tolist() for g in range(games)) >= 60


def _nets():
    from xiangqi_alphazero_amd import model, weights
    nets = []
    for seed in (1, 2):
        n = model.XiangqiNet(64, 2)
        n.load_state_dict(weights.make_state_dict(64, 2, seed=seed, policy_gain=4.0))
        nets.append(n)
    return nets


def test_packed_equals_masked_equals_dense(monkeypatch):
    from xiangqi_alphazero_amd import arena, evaluator
    nets = _nets()
    kw = dict(opening_plies=2, seed=3)

    def evs():
        return evaluator.make_evaluator(nets[0], "cuda", "hip")[0], evaluator.make_evaluator(nets[1], "cuda", "hip")[0]

    info = {}
    en, eo = evs()
    packed_graph = arena.play_arena(en, eo, 8, 12, 24, info=info, **kw)          # the shipped path: graph, side stream
    assert info["packed"] and info["stats"]["overflow"] == 0
    st = info["stats"]
    assert st["rows_evaluated"] == st["root_evals"] + st["leaf_evals"] > 0       # every request once, by one network
    assert st["rows_evaluated"] <= info["steps"] * 8
    monkeypatch.setenv("XQ_ARENA_GRAPH", "0")
    monkeypatch.setenv("XQ_ARENA_STREAMS", "0")
    en, eo = evs()
    info_e = {}
    packed_eager = arena.play_arena(en, eo, 8, 12, 24, packed=True, info=info_e, **kw)
    assert info_e["packed"] and info_e["stats"]["rows_evaluated"] == info_e["stats"]["root_evals"] + info_e["stats"]["leaf_evals"]
    monkeypatch.delenv("XQ_ARENA_GRAPH")
    monkeypatch.delenv("XQ_ARENA_STREAMS")
    en, eo = evs()
    info_m = {}
    masked = arena.play_arena(en, eo, 8, 12, 24, packed=False, info=info_m, **kw)
    assert not info_m["packed"] and info_m["stats"]["rows_evaluated"] == 0
    dense = arena.play_arena(lambda x: en(x), lambda x: eo(x), 8, 12, 24, **kw)
    assert _table(packed_graph) == _table(packed_eager) == _table(masked) == _table(dense)
    assert info["openings"].tolist() == info_e["openings"].tolist() == info_m["openings"].tolist()
    assert all(int(c) == 2 for c in info["opening_counts"]) and all(s >= 2 for _, s in _table(dense))
    # one evaluator on both sides: one stream, no shared output buffers between the two branches
    same_packed = arena.play_arena(en, en, 8, 12, 24, packed=True, **kw)
    same_dense = arena.play_arena(lambda x: en(x), lambda x: en(x), 8, 12, 24, **kw)
    assert _table(same_packed) == _table(same_dense)
    with pytest.raises(Exception, match="live_rows"):
        arena.play_arena(lambda x: en(x), lambda x: eo(x), 8, 12, 24, packed=True, **kw)


@pytest.mark.parametrize("first_game", [0, 1])
def test_the_partition_itself(first_game):
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    nets = _nets()
    en, eo = (evaluator.make_evaluator(n, "cuda", "hip")[0] for n in nets)
    G_ = 8
    cfg = engine.make_config(G_, 4, max_game_length=30, random_opening_moves=0, enable_resign=False, add_noise=False,
                             games_target=G_, manual_moves=2, seed=5)
    eng = engine.SelfPlayEngine(cfg, arena_opts=(2, first_game))
    new_is_red = ((torch.arange(G_, device="cuda") + first_game) % 2 == 0)
    sides, sizes = set(), set()
    for step in range(24):
        x = eng.select()
        eng.compact_arena()
        torch.cuda.synchronize()
        phase = eng.slot_ints[:, 3]
        waiting = ((phase == 2) | (phase == 4))
        red = eng.slot_ints[:, 0] == 1
        want = [(waiting & (new_is_red == red)).nonzero().view(-1).tolist(), (waiting & (new_is_red != red)).nonzero().view(-1).tolist()]
        got = []
        for m, s in enumerate(eng.arena_packed):
            n = int(s["n_live"].item())
            rows = s["rows"][:n].tolist()
            got.append(rows)
            assert rows == sorted(rows) and rows == want[m], (step, m)          # ascending, and the rule's set
            idx = torch.tensor(rows, dtype=torch.int64, device="cuda")
            assert torch.equal(s["x"][:n], x.index_select(0, idx))              # bit for bit
            assert torch.equal(s["moves"][:n], eng.req_moves.index_select(0, idx))
            assert torch.equal(s["counts"][:n], eng.req_counts.index_select(0, idx)) and bool((s["counts"][:n] > 0).all())
        assert not set(got[0]) & set(got[1])
        assert sorted(got[0] + got[1]) == waiting.nonzero().view(-1).tolist()
        sides |= set(red[waiting].tolist())
        sizes.add((len(got[0]), len(got[1])))
        s_new, s_old = eng.arena_packed
        ll_n, v_n = en.evaluate_legal(s_new["x"], s_new["moves"], s_new["counts"], n_live=s_new["n_live"])
        ll_o, v_o = eo.evaluate_legal(s_old["x"], s_old["moves"], s_old["counts"], n_live=s_old["n_live"])
        eng.expand_packed_arena(ll_n, v_n, ll_o, v_o)
    st = eng.stats()
    assert sides == {True, False} and st["overflow"] == 0 and st["moves_played"] >= G_
    assert st["rows_evaluated"] == st["root_evals"] + st["leaf_evals"]
    assert any(a > 0 and b > 0 for a, b in sizes)
    plain = engine.SelfPlayEngine(cfg)                                          # no arena options: the calls are refused
    for call in (plain.compact_arena, plain.arena_openings):
        with pytest.raises(Exception, match="arena_opts"):
            call()
