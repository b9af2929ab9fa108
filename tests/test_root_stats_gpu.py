"""Root statistics per sample (xq_engine_init_rs) and the q-mixed value target (xq_samples_to_batch_ex) on the GPU.

1. whole games with injected draws and the stub evaluator equal tests/root_stats_model.py: every existing field as the model's,
   the 20 bytes at offset 108 bit for bit -- plain, tree reuse, playout cap, forced playouts, solver, solver + reuse + cap; the
   rule-4 sample (root_q = 1, raw visits 79 of 100) and the sample whose quotient is exactly 1.0 among them;
2. off is today's engine: the records of an engine with the option on, their 20 bytes zeroed, are the records of an engine set up
   through xq_engine_init_sv on the same draws, whose own 20 bytes are zero -- eager and replayed, without and with the
   evaluation cache;
3. leaf batching, K = 4: on against off as in 2, and in every sample the mark, root_visits = the sum of visits[], |root_q| <= 1;
4. the batch kernel: opts = NULL and lambda = 0 are xq_samples_to_batch byte for byte; for lambda in {0.25, 0.5, 1} dev_z is
   sample_format.mixed_z bit for bit, planes and pi are the plain call's bytes, a mirrored row carries the same value; n = 1, 3,
   65 and 130 with repeated indices;
5. the train step (16x1 net, library path, batches of 32): lambda = 0 leaves the weights of two steps bit-identical to a run
   without the keyword; at lambda = 0.5 the reported value loss is the MSE against mixed_z; root_stats_coverage;
6. MCTS.search_many(return_values=True).
"""
import ctypes as C
import types

import numpy as np
import pytest

import golden_io as G
import root_stats_model as RS
from stub_eval import predict_from_key, state_key
from test_playout_cap_gpu import _engine_cfg, _inject_array, _play_stub
from test_root_stats_model import GAMES, IDS, model_game, options
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

PAD = slice(108, 128)

# the short recorded games under every option set; the two long ones where their samples are needed: `natural` holds the quotient
# of exactly 1.0, the S = 100 game the rule-4 sample (solver) and the deepest reuse
CASES = [(n, o) for n in ("resign", "maxlen", "resign_late") for o in ("plain", "reuse", "cap", "forced", "solver", "solver_reuse_cap")] + \
        [("natural", "plain"), ("natural", "cap"), ("long_peaked", "solver"), ("long_peaked", "solver_reuse_cap"),
         ("long_peaked", "reuse"), ("long_peaked", "forced")]

_played = {}


def _engine_kw(opt, S):
    kw = options(opt, S)
    return dict(tree_reuse=kw.get("tree_reuse", False), playout_cap=kw.get("cap"), forced_playouts=kw.get("forced"),
                solver=kw.get("solver", False))


def _gpu_game(name, opt):
    """One slot plays game `name` under option set `opt` with root statistics on -> (records in ply order, results, stats);
    played once per (game, option set), shared, never modified."""
    from xiangqi_alphazero_amd import engine
    if (name, opt) not in _played:
        c, peaked, seed, _ = GAMES[IDS.index(name)]
        inj_len = 16384
        eng = engine.SelfPlayEngine(_engine_cfg(engine, c, 1, inj_len, 1), inject=_inject_array([seed], inj_len), root_stats=True,
                                    **_engine_kw(opt, int(c["num_simulations"])))
        assert eng.root_stats
        st = _play_stub(eng, peaked, 1)
        samples, results = eng.drain()
        samples = samples[np.argsort(samples["ply"], kind="stable")]
        samples.setflags(write=False)
        _played[(name, opt)] = (samples, results, st)
    return _played[(name, opt)]


# ---- 1. whole games -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opt", CASES, ids=["%s-%s" % c for c in CASES])
def test_games_equal_host_model(name, opt):
    from xiangqi_alphazero_amd import sample_format as F
    want, winner, plies, mst = model_game(GAMES[IDS.index(name)], opt)
    mine, results, st = _gpu_game(name, opt)
    assert len(results) == 1 and (int(results[0]["winner"]), int(results[0]["steps"]), int(results[0]["n_samples"])) == \
        (winner, plies, len(want))
    assert len(mine) == len(want) and st["samples_written"] == len(want) and st["moves_played"] == len(mst["moves"])
    raw = mine.view(np.uint8).reshape(len(mine), 640)
    rs = F.root_stats(mine)
    for k, (s, w) in enumerate(zip(mine, want)):
        n = int(s["n_moves"])
        assert list(s["actions"][:n]) == list(w["actions"]), k
        assert list(s["visits"][:n]) == list(w["visits"]), k
        assert int(s["reserved1"]) == w["proven"] and int(s["reserved0"]) == 0, k
        assert int(s["z"]) == w["z"] and bytes(s["board"].view(np.int8)) == bytes(w["board"]), k
        assert int(s["late_temp"]) == int(w["late"]) and int(s["side"]) == w["player"], k
        assert bytes(raw[k, PAD]) == RS.pad_bytes(w), (k, rs[k], w["root_q"], w["root_visits"])
    if (name, opt) == ("long_peaked", "solver"):       # the rule-4 sample: +1 with the raw visits of an early end
        assert (float(rs[31]["root_q"]), int(rs[31]["root_visits"]), int(mine[31]["reserved1"])) == (1.0, 79, 1)
    if (name, opt) == ("natural", "plain"):            # the quotient that is exactly 1.0, without the solver
        ones = np.nonzero(rs["root_q"] == np.float32(1.0))[0]
        assert len(ones) == 1 and int(mine[ones[0]]["reserved1"]) == 0 and int(rs[ones[0]]["root_visits"]) == 16


# ---- 2. off is today's engine ---------------------------------------------------------------------------------------------------
def _sorted_records(eng):
    smp, res = eng.drain()
    return np.sort(smp, order=["slot", "game_seq", "ply"]), np.sort(res, order=["slot", "game_seq"])


def _run(eng, n_games, graph, sims):
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while True:
        eng.step()
        if eng.steps % 16 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 60 * (sims + 1), "games did not finish"
    st = eng.stats()
    assert st["overflow"] == 0
    return st


def _init_sv(eng, cfg, K=1):
    """The same engine, initialised again through xq_engine_init_sv with every option absent."""
    import torch
    from xiangqi_alphazero_amd import hip
    base = (eng.ws.data_ptr() + 255) & ~255
    hip.check(eng.lib.xq_engine_init_sv(C.byref(eng.h), C.byref(cfg), K, 0, None, None, None, None, None, None, base,
                                        eng.workspace_bytes, None, hip.stream_ptr(eng.device)), "xq_engine_init_sv")
    torch.cuda.synchronize()


def _on_against_off(on, off, n_games):
    """`on`'s records with their 20 bytes zeroed are `off`'s; `off`'s own 20 bytes are zero; every `on` sample is marked."""
    from xiangqi_alphazero_amd import sample_format as F
    smp_on, res_on = on
    smp_off, res_off = off
    assert len(smp_on) == len(smp_off) > 0 and len(res_on) == len(res_off) == n_games
    raw_on = smp_on.view(np.uint8).reshape(len(smp_on), 640).copy()
    raw_off = smp_off.view(np.uint8).reshape(len(smp_off), 640)
    assert not raw_off[:, PAD].any()
    assert (raw_on[:, 116] == 1).all() and not raw_on[:, 117:128].any()
    raw_on[:, PAD] = 0
    assert raw_on.tobytes() == raw_off.tobytes() and res_on.tobytes() == res_off.tobytes()
    rs = F.root_stats(smp_on)
    vsum = np.array([int(s["visits"][:s["n_moves"]].sum()) for s in smp_on])
    assert (rs["root_visits"] == vsum).all() and (np.abs(rs["root_q"]) <= 1.0).all()


@pytest.mark.parametrize("K", [1, 4], ids=["sequential", "leaves4"])
def test_off_is_the_engine_of_init_sv(K):
    """Part 2 (K = 1) and part 3 (leaf batching, K = 4): eager and replayed."""
    from xiangqi_alphazero_amd import engine
    ev = _TorchStub()
    n_games, sims = 2, 12
    cfg = engine.make_config(n_games, sims, seed=5, games_target=n_games, max_game_length=30)
    off_eng = engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=K)
    assert not off_eng.root_stats
    _init_sv(off_eng, cfg, K)
    st_off = _run(off_eng, n_games, False, sims)
    off = _sorted_records(off_eng)
    for graph in (False, True):
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=K, root_stats=True)
        st = _run(eng, n_games, graph, sims)
        _on_against_off(_sorted_records(eng), off, n_games)
        assert all(st[k] == st_off[k] for k in ("sims", "moves_played", "samples_written", "nodes_created", "depth_sum"))


def test_off_is_today_with_the_evaluation_cache():
    """Part 2 with the evaluation cache on, eager and replayed: the off engine of each mode is set up through xq_engine_init_sv."""
    from xiangqi_alphazero_amd import engine
    _, ev = _hip_evaluator()
    n_games, sims = 2, 12
    cfg = engine.make_config(n_games, sims, seed=3, games_target=n_games, max_game_length=30)
    for graph in (False, True):
        out = {}
        for on in (False, True):
            eng = engine.SelfPlayEngine(cfg, evaluator=ev, eval_cache_entries=64, root_stats=on)
            assert bool(eng.root_stats) == on
            if not on:
                _init_sv(eng, cfg)
            st = _run(eng, n_games, graph, sims)
            assert st["eval_cache_hits"] > 0 and eng.launch_mode == ("graph" if graph else "eager")
            out[on] = _sorted_records(eng)
        _on_against_off(out[True], out[False], n_games)


# ---- 4. the batch kernel --------------------------------------------------------------------------------------------------------
def _edge_records(template):
    """Hand-made edge records on a real record's position: unmarked with a root_q that must be ignored, root_q = +-1, z = 0."""
    from xiangqi_alphazero_amd import sample_format as F
    edge = np.repeat(template, 6)
    pad = np.zeros(6, dtype=F.ROOT_STATS_DTYPE)
    for k, (z, q, m) in enumerate([(1, -0.75, 0), (-1, 1.0, 1), (1, -1.0, 1), (0, 0.3, 1), (0, -1.0, 1), (0, 0.5, 0)]):
        edge[k]["z"] = z
        pad[k]["root_q"], pad[k]["root_visits"], pad[k]["has_root_stats"] = q, 16, m
    edge["pad"] = pad.view(np.uint8).reshape(6, 20)
    return edge


@pytest.fixture(scope="module")
def batch_records():
    """About 40 records: 34 of the GPU's `natural` game (the sample with root_q == 1.0 among them) and six hand-made ones."""
    from xiangqi_alphazero_amd import sample_format as F
    mine = _gpu_game("natural", "plain")[0]
    one = int(np.nonzero(F.root_stats(mine)["root_q"] == np.float32(1.0))[0][0])
    pick = sorted(set(range(0, len(mine), 6)) | {one})
    rec = np.concatenate([mine[pick], _edge_records(mine[5:6])])
    rec.setflags(write=False)
    return rec


def _batch(store, idx, flip, opts, ex=True, late_temperature=0.3):
    import torch
    from xiangqi_alphazero_amd import hip
    n = len(idx)
    di, df = torch.tensor(idx, dtype=torch.int32).cuda(), torch.tensor(flip, dtype=torch.uint8).cuda()
    states = torch.full((n, 15, 10, 9), -7.0, dtype=torch.float32).cuda()
    pi = torch.full((n, hip.ACTION_SPACE), -7.0, dtype=torch.float32).cuda()
    z = torch.full((n,), -7.0, dtype=torch.float32).cuda()
    if ex:
        rc = hip.lib().xq_samples_to_batch_ex(store.data_ptr(), di.data_ptr(), df.data_ptr(), n, late_temperature,
                                              None if opts is None else C.byref(opts), states.data_ptr(), pi.data_ptr(),
                                              z.data_ptr(), hip.stream_ptr())
    else:
        rc = hip.lib().xq_samples_to_batch(store.data_ptr(), di.data_ptr(), df.data_ptr(), n, late_temperature, states.data_ptr(),
                                           pi.data_ptr(), z.data_ptr(), hip.stream_ptr())
    hip.check(rc, "xq_samples_to_batch")
    torch.cuda.synchronize()
    return states.cpu().numpy(), pi.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_batch_kernel_mixed_target(batch_records, n):
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    rec = batch_records
    assert 38 <= len(rec) <= 46
    store = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), 640).copy()).cuda()
    rng = np.random.RandomState(n)
    idx = [len(rec) - 1 - (j % len(rec)) for j in range(n)] if n > 3 else list(rng.randint(0, len(rec), n))
    flip = [(j // len(rec) + j % len(rec)) % 2 for j in range(n)]      # past len(rec) an index comes back with the other flag
    plain = _batch(store, idx, flip, None, ex=False)
    for opts in (None, hip.BatchOpts(0.0)):
        got = _batch(store, idx, flip, opts)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain))
    assert plain[2].tobytes() == rec["z"][idx].astype(np.float32).tobytes()
    for lam in (0.25, 0.5, 1.0):
        states, pi, z = _batch(store, idx, flip, hip.BatchOpts(lam))
        want = F.mixed_z(rec, lam)[idx]
        assert z.tobytes() == want.tobytes(), (lam, z, want)
        assert states.tobytes() == plain[0].tobytes() and pi.tobytes() == plain[1].tobytes()
        if n > len(rec):                                               # the same record mirrored and not: one value
            assert flip[0] != flip[len(rec)] and idx[0] == idx[len(rec)] and z[0].tobytes() == z[len(rec)].tobytes()
    marked = F.root_stats(rec)["has_root_stats"][idx] == 1
    differs = F.mixed_z(rec, 0.5)[idx] != rec["z"][idx]
    assert not differs[~marked].any() and (n < 65 or differs[marked].any())


# ---- 5. the train step ----------------------------------------------------------------------------------------------------------
def _net_and_optimizer():
    import torch
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(16, 1)
    net.load_state_dict(weights.make_state_dict(16, 1, seed=11))
    net = net.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4)
    return net, opt, torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.1)


def test_train_step_mixed_target(batch_records):
    import torch
    import torch.nn.functional as Fn
    from xiangqi_alphazero_amd import training
    from xiangqi_alphazero_amd import sample_format as F
    rec = batch_records
    cfg = types.SimpleNamespace(min_buffer_size=10, num_epochs=1, batch_size=32)
    # lambda = 0: two steps (32 records, 64 logical samples), bit-identical to a run without the keyword
    buf = training.ReplayBuffer(50000)
    buf.extend(rec[:32].copy())
    end = []
    # the library's convolutions are held to their deterministic algorithms for the comparison, and one discarded run goes first:
    # the first convolution of a shape in a process may be served by another algorithm than every later one
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for kw in ({}, {}, dict(q_mix=0.0)):
            net, opt, sch = _net_and_optimizer()
            stats = training.train_network(net, opt, sch, buf, cfg, shuffle=False, **kw)
            assert stats["value_target_q_mix"] == 0.0
            end.append((stats, {k: v.cpu().numpy().tobytes() for k, v in net.state_dict().items()}))
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was
    differing = [k for k in end[1][1] if end[1][1][k] != end[2][1][k]]
    print("weights that differ between the run without the keyword and the run at lambda = 0:", differing)
    assert not differing and end[1][0] == end[2][0]
    # coverage: the share of marked records, counted in numpy
    share = float((F.root_stats(rec[:32])["has_root_stats"] == 1).mean())
    assert buf.root_stats_coverage() == share
    whole = training.ReplayBuffer(50000)
    whole.extend(rec.copy())
    assert whole.root_stats_coverage() == float((F.root_stats(rec)["has_root_stats"] == 1).mean()) < 1.0
    # lambda = 0.5: one batch (the last 16 records, edge records included, 32 logical samples); the reported value loss is the MSE
    # against mixed_z of the same indices
    tail = rec[-16:]
    one = training.ReplayBuffer(50000)
    one.extend(tail.copy())
    net, opt, sch = _net_and_optimizer()
    ref, _, _ = _net_and_optimizer()
    stats = training.train_network(net, opt, sch, one, cfg, shuffle=False, q_mix=0.5)
    assert stats["value_target_q_mix"] == 0.5
    states, _, z = one.batch(torch.arange(32), q_mix=0.5)
    target = torch.from_numpy(np.repeat(F.mixed_z(tail, 0.5), 2)).cuda()[:, None]
    assert z.cpu().numpy().tobytes() == target.cpu().numpy().tobytes()
    ref.train()
    with torch.no_grad():
        want = float(Fn.mse_loss(ref(states)[1], target))
        plain = float(Fn.mse_loss(ref(states)[1], torch.from_numpy(np.repeat(tail["z"].astype(np.float32), 2)).cuda()[:, None]))
    print("value loss", stats["value_loss"], "mse against mixed_z", want, "against z", plain)
    assert abs(stats["value_loss"] - want) <= 1e-6 * abs(want)
    assert abs(plain - want) > 1e-3 * abs(want)                        # the mixed target is another target on these records


# ---- 6. the serving shim --------------------------------------------------------------------------------------------------------
def test_mcts_search_many_returns_root_values():
    import torch
    from oracle import xq_oracle as O
    from xiangqi_alphazero_amd import mcts as M

    def stub(x):
        xs = x.cpu().numpy()
        pv = [predict_from_key(state_key(xs[i]), True) for i in range(len(xs))]
        return (torch.log(torch.from_numpy(np.stack([p for p, _ in pv])).cuda()),
                torch.tensor([v for _, v in pv], dtype=torch.float32).cuda())

    games = []
    for t in [x for x in G.mcts_traces() if x["sims"] == 100 and not x["noisy"] and x["stub"] == "peaked"][2:4]:
        g = O.Game()
        for a in t["actions"]:
            g.make_action(a)
        games.append(types.SimpleNamespace(board=g.board.copy(), current_player=g.current_player, move_count=g.move_count,
                                           no_capture_count=g.no_capture_count, history=[bytes(h) for h in g.history()]))
    m = M.MCTS(stub, num_simulations=16, c_puct=1.5)
    pis = m.search_many(games, temperature=1.0, add_noise=False)
    assert m.root_values.dtype == np.float32 and m.root_values.shape == (2,)
    pis2, values = m.search_many(games, temperature=1.0, add_noise=False, return_values=True)
    assert values.dtype == np.float32 and values.tobytes() == m.root_values.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pis, pis2))
    eng = m._engine(2, False)
    for slot in range(2):
        r = eng.read_root(slot)
        sum_w, sum_n = 0.0, 0
        for w, n in zip(r["total_value"], r["visits"]):
            sum_w += float(w)
            sum_n += int(n)
        assert sum_n == 16 and values[slot].tobytes() == np.float32(sum_w / sum_n).tobytes() and values[slot] != 0.0
