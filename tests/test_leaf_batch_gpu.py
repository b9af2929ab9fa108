"""Leaf batching on the GPU (k_select_multi / k_expand_multi / k_compact_multi, xq_engine_init_leaves).

* search only: root visits, W (as hex), priors and the collision count of every position equal the host model's
  (tests/leaf_batch_model.py, pinned against the reference at K = 1) -- stub evaluators with and without injected root
  noise, and the hand-written ResNet evaluator;
* self-play: visit counts sum to S, the virtual loss is zero after every step, no overflow, and the records are identical
  across runs, eager vs replayed steps, and packed vs full-width steps.
"""
import hashlib
import types

import numpy as np
import pytest

import golden_io as G
import leaf_batch_model as M
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key

pytestmark = pytest.mark.gpu


def _replay(actions):
    g = O.Game()
    for a in actions:
        g.make_action(a)
    return g


def _set(eng, slot, g, noise=None):
    eng.set_position(slot, g.board, g.current_player, g.move_count, g.no_capture_count, g.history()[-12:], noise)


def _vl_zero(eng):
    return not bool(eng.arena_views()["vl"].any().item())


def _run_stub_search(eng, peaked, max_steps):
    """Dense-protocol steps (probabilities, is_probs = 1) until every slot holds its search; checks vl after each step."""
    import torch
    cache = {}
    for step in range(max_steps):
        x = eng.select().cpu().numpy()
        counts = eng.req_counts.cpu().numpy()
        probs = np.zeros((eng.rows, 8100), dtype=np.float32)
        vals = np.zeros(eng.rows, dtype=np.float32)
        for r in np.nonzero(counts > 0)[0]:
            key = (state_key(x[r]), bool(peaked[r // eng.K]))
            if key not in cache:
                cache[key] = predict_from_key(*key)
            probs[r], vals[r] = cache[key]
        eng.expand(torch.from_numpy(probs).cuda(), torch.from_numpy(vals).cuda(), is_probs=True)
        assert _vl_zero(eng), step
        if eng.held():
            return step + 1
    raise AssertionError("search did not finish")


def _compare(eng, slot, want, tag):
    r = eng.read_root(slot)
    assert r["sims_done"] == eng.cfg.num_simulations and r["root_visits"] == want["root_visits"], tag
    assert list(r["actions"]) == list(want["actions"]), tag
    assert list(r["visits"]) == list(want["visits"]), tag
    assert [float(x).hex() for x in r["total_value"]] == [float(x).hex() for x in want["total_value"]], tag
    assert [float(x).hex() for x in r["prior"]] == [float(x).hex() for x in want["prior"]], tag
    assert int(eng.slot_counters()[slot, 19].item()) == want["collisions"], tag


@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("sims", [16, 100])
def test_search_equals_model_stub(K, sims):
    from xiangqi_alphazero_amd import engine
    traces = [t for t in G.mcts_traces() if t["sims"] == sims]
    eng = engine.SelfPlayEngine(engine.make_config(len(traces), sims, add_noise=False, manual_moves=True), leaves_per_step=K)
    games, noises = [], []
    for i, t in enumerate(traces):
        noise = None if t["eta"] is None else np.array([G.hexf(x) for x in t["eta"]])
        g = _replay(t["actions"])
        _set(eng, i, g, noise)
        games.append(g); noises.append(noise)
    peaked = [t["stub"] == "peaked" for t in traces]
    steps = _run_stub_search(eng, peaked, sims + 8)
    st = eng.stats()
    assert st["overflow"] == 0 and steps <= sims // 2 + 8
    coll = 0
    for i, t in enumerate(traces):
        want = M.search(games[i], sims, K, M.stub_priors(peaked[i]), noise=noises[i])
        _compare(eng, i, want, (t["name"], t["stub"], t["noisy"], K))
        coll += want["collisions"]
    assert st["collisions"] == coll and st["sims"] == sims * len(traces)
    assert st["leaf_steps"] > 0 and st["leaves_per_step_sum"] == st["leaf_evals"]


def _hip_evaluator(channels=64, blocks=2):
    from xiangqi_alphazero_amd import evaluator, model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=4.0))
    return evaluator.make_evaluator(net, "cuda", "hip")[0]


def _engine_priors(ev):
    """The model's evaluator for the HIP network: one position at a time through a K = 1 search-only engine (one slot, one
    root expansion), so priors are computed by the engine's own softmax; the value is the evaluator's row."""
    from xiangqi_alphazero_amd import engine
    e1 = engine.SelfPlayEngine(engine.make_config(1, 1, add_noise=False, manual_moves=True), evaluator=ev)

    def f(state, legal, game):
        _set(e1, 0, game)
        x = e1.select()
        ll, v = ev.evaluate_legal(x, e1.req_moves, e1.req_counts)
        e1.expand_legal(ll, v)
        r = e1.read_root(0)
        assert list(r["actions"]) == list(legal)
        pri = r["prior"].astype(np.float32) if not r["prior_is_f64"] else r["prior"]
        return pri, (2 if r["prior_is_f64"] else 0), float(v[0].item())
    return f


@pytest.mark.parametrize("K", [4, 8])
def test_search_equals_model_hip_evaluator(K):
    from xiangqi_alphazero_amd import engine
    ev = _hip_evaluator()
    d = G.corpus()
    picks = [i for i in range(5, len(d["board"]), 70) if not d["done"][i]][:6]
    games = []
    for i in picks:
        first = i - d["ply"][i]
        games.append(_replay([int(a) for a in d["taken"][first:i]]))
    sims = 48
    eng = engine.SelfPlayEngine(engine.make_config(len(games), sims, add_noise=False, manual_moves=True), evaluator=ev,
                                leaves_per_step=K)
    assert eng.path == "packed"
    for s, g in enumerate(games):
        _set(eng, s, g)
    for _ in range(sims + 8):
        eng.step()
        assert _vl_zero(eng)
        if eng.held():
            break
    assert eng.held() and eng.stats()["overflow"] == 0
    pf = _engine_priors(ev)
    for s, g in enumerate(games):
        model = M.LeafBatchSearch(g, sims, K, None)
        model.priors = lambda state, legal, _m=model: pf(state, legal, _m.current)
        want = model.run().root()
        _compare(eng, s, want, (s, K))


class _TorchStub:
    """Deterministic, capturable stub for the dense protocol: logits and value are elementwise functions of an exact
    integer key of the planes (0/1 planes times small integer weights: float32 sums are exact in any order)."""

    def __init__(self):
        import torch
        g = torch.Generator().manual_seed(5)
        self.w = torch.randint(1, 512, (1350,), generator=g).float().cuda()
        self.a = torch.randint(1, 1 << 12, (8100,), generator=g).float().cuda()

    def __call__(self, x):
        import torch
        key = (x.reshape(x.shape[0], -1) * self.w).sum(1)                       # exact integer < 2^24
        logits = torch.remainder(key[:, None] + self.a[None, :], 61.0) / 8.0      # exact
        value = (torch.remainder(key * 3.0, 201.0) - 100.0) / 128.0
        return logits, value


def _records_sha(eng):
    smp, res = eng.drain()
    smp = np.sort(smp, order=["slot", "game_seq", "ply"])
    res = np.sort(res, order=["slot", "game_seq"])
    return hashlib.sha256(smp.tobytes() + res.tobytes()).hexdigest(), smp, res


def _stub_selfplay(K, graph, n_games=12, sims=24):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(n_games, sims, seed=3, games_target=n_games, max_game_length=40)
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), leaves_per_step=K)
    assert eng.path == "full"
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while True:
        eng.step()
        if not graph:
            assert _vl_zero(eng)
        if eng.steps % 16 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 40 * (sims + 1), "games did not finish"
    assert _vl_zero(eng)
    st = eng.stats()
    sha, smp, res = _records_sha(eng)
    return st, sha, smp, res


@pytest.mark.parametrize("K", [4, 8])
def test_selfplay_stub_invariants_and_determinism(K):
    sims = 24
    st, sha, smp, res = _stub_selfplay(K, graph=False, sims=sims)
    assert st["overflow"] == 0 and st["games_finished"] >= 12 and len(smp) > 0
    assert all(int(s["visits"][:s["n_moves"]].sum()) == sims for s in smp)
    assert st["leaves_per_step_sum"] == st["leaf_evals"] and st["leaves_per_step_sum"] > st["leaf_steps"]
    st2, sha2, _, _ = _stub_selfplay(K, graph=False, sims=sims)
    assert sha2 == sha and st2 == st
    st3, sha3, _, _ = _stub_selfplay(K, graph=True, sims=sims)
    assert sha3 == sha


@pytest.mark.parametrize("K", [4, 8])
def test_selfplay_packed_equals_full_width_hip_evaluator(K):
    from xiangqi_alphazero_amd import engine
    ev = _hip_evaluator()
    n_games, sims = 16, 24

    def make():
        cfg = engine.make_config(n_games, sims, seed=7, games_target=n_games, max_game_length=40)
        return engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=K)

    full = make()
    n = 0
    while True:
        x = full.select()
        ll, v = ev.evaluate_legal(x, full.req_moves, full.req_counts)
        full.expand_legal(ll, v)
        n += 1
        if n % 16 == 0 and full.stats()["games_finished"] >= n_games:
            break
        assert n < 40 * (sims + 1), "games did not finish"
    st_full = full.stats()
    sha_full, smp, _ = _records_sha(full)
    packed = make()
    assert packed.path == "packed" and packed.capture_step()
    while packed.steps < n:
        packed.step()
    st_packed = packed.stats()
    sha_packed, _, _ = _records_sha(packed)
    assert st_full["overflow"] == 0 and len(smp) > 0
    assert all(int(s["visits"][:s["n_moves"]].sum()) == sims for s in smp)
    assert sha_packed == sha_full
    assert {k: v for k, v in st_packed.items() if k != "rows_evaluated"} == {k: v for k, v in st_full.items() if k != "rows_evaluated"}
    assert st_packed["rows_evaluated"] < n * n_games * K


def test_mcts_shim_with_leaves():
    """MCTS(..., leaves_per_step=8) finishes every search with exactly S simulations in far fewer steps."""
    from xiangqi_alphazero_amd import mcts
    ev = _hip_evaluator()
    m = mcts.MCTS(ev, num_simulations=100, leaves_per_step=8)
    o = O.Game()
    g = types.SimpleNamespace(board=o.board.copy(), current_player=o.current_player, move_count=0, no_capture_count=0,
                              history=[])                                   # the reference's XiangqiGame shape
    pi = m.search(g, temperature=1.0, add_noise=False)
    assert abs(pi.sum() - 1.0) < 1e-12
    eng = m._engines[(1, False)]
    r = eng.read_root(0)
    assert r["sims_done"] == 100 and int(r["visits"].sum()) == 100 and eng.steps < 40
