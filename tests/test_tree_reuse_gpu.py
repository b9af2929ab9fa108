"""Tree reuse on the GPU (k_select<true> / k_reroot / k_expand<true>, xq_engine_init_ex with XQ_ENGINE_TREE_REUSE).

* re-root: after the step that ends a move, the arena is the chosen child's subtree of the tree before that step, node for node
  (N, W and P bits, action, first child, child count, kind, child order), with root N = the children's visits and kind 1;
* whole games with injected draws equal the host model (tests/tree_reuse_model.py): samples, z, results and counters;
* records are byte-identical with reuse dropped before every step and reuse off, for init_ex(flags = 0) and init, for eager and
  replayed steps, and with and without the evaluation cache;
* run_games with the hand-written evaluator on peaked weights: the samples' visits are the new plus the reused simulations.
"""
import ctypes as C
import hashlib
import types

import numpy as np
import pytest

import golden_io as G
import tree_reuse_model as M
from draws import Stream
from stub_eval import predict_from_key, state_key

pytestmark = pytest.mark.gpu

PH_SEARCH, PH_FINISHED = 3, 5


def _stub_step(eng, peaked, cache):
    """One dense-protocol step (probabilities, is_probs = 1) with the host stub evaluator."""
    import torch
    x = eng.select().cpu().numpy()
    counts = eng.req_counts.cpu().numpy()
    probs = np.zeros((eng.rows, 8100), dtype=np.float32)
    vals = np.zeros(eng.rows, dtype=np.float32)
    for r in np.nonzero(counts > 0)[0]:
        key = state_key(x[r])
        if key not in cache:
            cache[key] = predict_from_key(key, peaked)
        probs[r], vals[r] = cache[key]
    eng.expand(torch.from_numpy(probs).cuda(), torch.from_numpy(vals).cuda(), is_probs=True)


def _snap(av, slot, mark):
    out = {k: av[k][slot, :mark].cpu().numpy() for k in ("N", "W", "P", "first")}
    out["action"] = av["action"][slot, :mark].cpu().numpy().view(np.uint16)
    out["meta"] = av["meta"][slot, :mark].cpu().numpy().view(np.uint16)
    out["board"] = av["board"][slot, :90].cpu().numpy()
    return out


def _played_action(old_board, new_board):
    diff = np.nonzero(old_board != new_board)[0]
    assert len(diff) == 2
    frm = [q for q in diff if new_board[q] == 0]
    assert len(frm) == 1
    to = [q for q in diff if q != frm[0]][0]
    return int(frm[0]) * 90 + int(to)


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("sims", [16, 100, 400])
def test_reroot_arena_is_the_chosen_subtree(sims, peaked):
    from xiangqi_alphazero_amd import engine
    G_ = 8
    eng = engine.SelfPlayEngine(engine.make_config(G_, sims, seed=11 + sims, max_game_length=60), tree_reuse=True)
    av = eng.arena_views()
    cache, checked, fresh, moves = {}, 0, 0, 0
    want = 12 if sims < 400 else G_
    for _ in range(3 * (sims + 2) + 40):
        si = eng.slot_ints.cpu().numpy()
        snaps = {s: _snap(av, s, int(si[s, 7])) for s in range(G_) if si[s, 4] == sims and si[s, 3] == PH_SEARCH}
        _stub_step(eng, peaked, cache)
        if not snaps:
            continue
        si2 = eng.slot_ints.cpu().numpy()
        cnt = eng.slot_counters().cpu().numpy()
        for s, old in snaps.items():
            moves += 1
            if si2[s, 3] == PH_FINISHED:                # the game ended at this root request
                continue
            new_board = av["board"][s, :90].cpu().numpy()
            a = _played_action(old["board"], new_board)
            f0, n0 = int(old["first"][0]), int(old["meta"][0]) & 0x3FFF
            c = f0 + list(old["action"][f0:f0 + n0]).index(a)
            mark = int(si2[s, 7])
            new = _snap(av, s, mark)
            if old["first"][c] < 0:                    # never expanded: a fresh root
                assert new["N"][0] == 0 and si2[s, 4] == 0 and new["action"][0] == 0
                fresh += 1
                continue
            order = M.compaction_order(old["first"], old["meta"] & 0x3FFF, c, int(old["N"].shape[0]))
            assert mark == len(order), (s, mark, len(order))
            tag = (sims, peaked, s, c)
            for k in ("W", "P", "action"):
                assert old[k][order].tobytes() == new[k].tobytes(), (k,) + tag
            assert list(new["first"]) == list(M.remap_first(old["first"], order)), tag
            assert list(new["meta"][1:]) == list(old["meta"][order][1:]), tag
            assert list(new["N"][1:]) == list(old["N"][order][1:]), tag
            n = int(new["meta"][0]) & 0x3FFF
            assert n == int(old["meta"][c]) & 0x3FFF and int(new["meta"][0]) >> 14 == 1 and new["first"][0] == 1, tag
            assert new["N"][0] == new["N"][1:1 + n].sum() == si2[s, 4] == old["N"][c] - 1, tag
            checked += 1
        if checked >= want:
            break
    st = eng.stats()
    assert checked >= want and st["overflow"] == 0, (checked, fresh, moves)
    assert st["reroots"] >= checked and st["reused_visits"] > 0


def _inject_array(seed, n_slots, length):
    arr = np.zeros((n_slots, 4, length), dtype=np.uint64)
    for kind in range(4):
        s = Stream(seed, kind + 1)
        arr[:, kind, :] = np.array([s.next_u64() for _ in range(length)], dtype=np.uint64)[None, :]
    return arr


_LONG = dict(num_simulations=48, c_puct=1.5, temperature_threshold=10, max_game_length=70, random_opening_moves=4,
             enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
GAMES = [(t["cfg"], t["stub"] == "peaked", t["seed"], t["name"]) for t in G.game_traces()] + [(_LONG, True, 31, "long_peaked")]


@pytest.mark.parametrize("game", GAMES, ids=[g[3] for g in GAMES])
def test_games_equal_host_model(game):
    from xiangqi_alphazero_amd import engine
    c, peaked, seed, _ = game
    n_slots, inj_len = 2, 16384
    cfg = engine.make_config(n_slots, c["num_simulations"], c_puct=c["c_puct"],
                             temperature_threshold=c["temperature_threshold"], max_game_length=c["max_game_length"],
                             random_opening_moves=c["random_opening_moves"], enable_resign=c["enable_resign"],
                             resign_threshold=c["resign_threshold"], resign_check_steps=c["resign_check_steps"],
                             add_noise=True, inject_len=inj_len, games_target=n_slots)
    eng = engine.SelfPlayEngine(cfg, inject=_inject_array(seed, n_slots, inj_len), tree_reuse=True)
    cache = {}
    for s in range(40000):
        _stub_step(eng, peaked, cache)
        if s % 32 == 31 and eng.stats()["games_finished"] >= n_slots:
            break
    st = eng.stats()
    assert st["overflow"] == 0 and st["games_finished"] == n_slots
    want, winner, plies, mst = M.play_game(c, peaked, seed, tree_reuse=True)
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
            assert list(s["actions"][:n]) == list(w["actions"]), (slot, k)
            assert list(s["visits"][:n]) == list(w["visits"]), (slot, k)
            assert int(s["z"]) == w["z"] and bytes(s["board"].view(np.int8)) == bytes(w["board"]), (slot, k)
    assert (st["sims"], st["reused_visits"], st["reroots"]) == tuple(n_slots * mst[k] for k in ("sims", "reused_visits", "reroots"))


class _TorchStub:
    """Deterministic, capturable dense-protocol stub: logits and value are elementwise functions of an exact integer key of the
    planes (0/1 planes times small integer weights: float32 sums are exact in any order)."""

    def __init__(self):
        import torch
        g = torch.Generator().manual_seed(5)
        self.w = torch.randint(1, 512, (1350,), generator=g).float().cuda()
        self.a = torch.randint(1, 1 << 12, (8100,), generator=g).float().cuda()

    def __call__(self, x):
        import torch
        key = (x.reshape(x.shape[0], -1) * self.w).sum(1)
        logits = torch.remainder(key[:, None] + self.a[None, :], 61.0) / 4.0
        value = (torch.remainder(key * 3.0, 201.0) - 100.0) / 128.0
        return logits, value


def _records_sha(eng):
    smp, res = eng.drain()
    smp = np.sort(smp, order=["slot", "game_seq", "ply"])
    res = np.sort(res, order=["slot", "game_seq"])
    return hashlib.sha256(smp.tobytes() + res.tobytes()).hexdigest(), smp


def _selfplay(ev, tree_reuse=False, graph=False, drop_every_step=False, init_ex_flags=None, cache_entries=0, n_games=12,
              sims=24, seed=3):
    import torch
    from xiangqi_alphazero_amd import engine, hip
    cfg = engine.make_config(n_games, sims, seed=seed, games_target=n_games, max_game_length=40)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, tree_reuse=tree_reuse, eval_cache_entries=cache_entries)
    if init_ex_flags is not None:                      # the same engine, initialised again through xq_engine_init_ex
        base = (eng.ws.data_ptr() + 255) & ~255
        hip.check(eng.lib.xq_engine_init_ex(C.byref(eng.h), C.byref(cfg), 1, init_ex_flags, base, eng.workspace_bytes, None,
                                            hip.stream_ptr(eng.device)), "xq_engine_init_ex")
        torch.cuda.synchronize()
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while True:
        if drop_every_step:
            eng.drop_reroots()
        eng.step()
        if eng.steps % 16 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 60 * (sims + 1), "games did not finish"
    st = eng.stats()
    sha, smp = _records_sha(eng)
    assert st["overflow"] == 0 and len(smp) > 0
    assert all(int(s["visits"][:s["n_moves"]].sum()) == sims for s in smp)
    return st, sha


def test_records_identical_where_reuse_must_not_matter():
    ev = _TorchStub()
    st_off, sha_off = _selfplay(ev)
    st_drop, sha_drop = _selfplay(ev, tree_reuse=True, drop_every_step=True)
    assert sha_drop == sha_off and st_drop["reroots"] == 0 and st_drop["sims"] == st_off["sims"]
    _, sha_ex0 = _selfplay(ev, init_ex_flags=0)
    assert sha_ex0 == sha_off
    st_on, sha_on = _selfplay(ev, tree_reuse=True)
    assert st_on["reroots"] > 0 and st_on["reused_visits"] > 0
    st_graph, sha_graph = _selfplay(ev, tree_reuse=True, graph=True)
    assert sha_graph == sha_on and st_graph["reused_visits"] == st_on["reused_visits"]


def _hip_evaluator(channels=64, blocks=2, policy_gain=4.0):
    from xiangqi_alphazero_amd import evaluator, model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=policy_gain))
    return net, evaluator.make_evaluator(net, "cuda", "hip")[0]


def test_reuse_with_eval_cache_equals_reuse_alone():
    _, ev = _hip_evaluator()
    st, sha = _selfplay(ev, tree_reuse=True, graph=True, n_games=16)
    st_c, sha_c = _selfplay(ev, tree_reuse=True, graph=True, n_games=16, cache_entries=64)
    assert sha_c == sha and st_c["eval_cache_hits"] > 0 and st_c["reused_visits"] == st["reused_visits"] > 0
    assert st_c["rows_evaluated"] < st["rows_evaluated"]


def test_run_games_peaked_weights_counts_reused_visits():
    from xiangqi_alphazero_amd import selfplay
    net, _ = _hip_evaluator(policy_gain=8.0)
    config = types.SimpleNamespace(num_simulations=64, c_puct=1.5, temperature_threshold=10, max_game_length=60,
                                   random_opening_moves=4, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
                                   tree_reuse=True)
    samples, results, st, _ = selfplay.run_games(net, config, 16, seed=5)
    assert st["tree_reuse"] and st["overflow"] == 0 and len(results) == 16
    visits = int(sum(int(s["visits"][:s["n_moves"]].sum()) for s in samples))
    assert visits == 64 * len(samples) == st["sims"] + st["reused_visits"]
    assert st["reused_visits"] > 0 and st["reroots"] > 0
