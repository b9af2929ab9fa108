"""The scoring pass and the policy-surprise epoch counts on the GPU (csrc/xq_score.hip).

1. xq_samples_to_requests against sample_format.encode_planes and the records' actions, bit for bit.
2. xq_score_samples against the float64 reference sample_format.sample_scores on hand-made logits (no network), within
   |got - ref| <= 2^-23 |ref| + 1e-12 (ce_ref + H_ref + 1): the one float32 cast, and the float64 summation order of at most 128
   terms with the device's log and exp at a few float64 ulp.  value and top1 exact; the written-back bytes are the score's and
   every other byte of every record is unchanged.
3. xq_surprise_counts against the host twin xq_surprise_count_host, bit for bit.
4. selfplay.score_samples end to end on a handful of short games, against a float64 torch forward of the same network.
5. train_network: surprise_weight = 0 is the run without the keyword, bit for bit; at 0.5 an epoch draws the reference's counts.
"""
import functools
import types

import numpy as np
import pytest

from policy_surprise_records import N_MOVES, score_records, set_policy_stats, surprise_records

pytestmark = pytest.mark.gpu

POOL = 130
SUM_BLOCK = 256        # threads per workgroup of the counts' reduction (csrc/xq_score.hip)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                     # a copy: the pool's arrays are read-only


def _raw(smp):
    return np.ascontiguousarray(smp).view(np.uint8).reshape(len(smp), 640)


@functools.lru_cache(maxsize=None)
def _pool():
    """130 hand-made records with their logits and values, and the float64 reference scores: computed once, never changed."""
    from xiangqi_alphazero_amd import sample_format as F
    smp, logits, value, notes = score_records(POOL, 11)
    ref = F.sample_scores(smp, logits, value, 0.3)
    for a in (smp, logits, value, ref):
        a.setflags(write=False)
    return smp, logits, value, notes, ref


def _indices(n, kind):
    """Rows for a launch of n: None (the first n records), a permutation that holds the records without moves, with one move and with
    128, or rows with repeats."""
    rng = np.random.default_rng(100 + n)
    if kind == "none":
        return None
    if kind == "permuted":
        must = [0, 1, 6][:n]                                         # n_moves 0, 1 and 128
        rest = [k for k in rng.permutation(POOL) if k not in must][:n - len(must)]
        return rng.permutation(np.array(must + rest, dtype=np.int32)).astype(np.int32)
    idx = rng.integers(0, POOL, n).astype(np.int32)
    idx[-1] = idx[0]                                                 # at least one record twice (n = 1: once)
    if n >= 3:
        idx[1] = 6
    return idx


# ---- 1. the gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "permuted", "repeats"])
@pytest.mark.parametrize("n", [1, 3, 5, 65, 130])
def test_samples_to_requests(n, kind):
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    smp = _pool()[0]
    assert [int(smp[k]["n_moves"]) for k in (0, 1, 6)] == [0, 1, 128]
    idx = _indices(n, kind)
    rows = np.arange(n) if idx is None else idx
    store = _t(_raw(smp))
    # sentinels behind the n rows: nothing past row n may be written
    x = torch.full((n + 1, 15, 10, 9), 7.0, device="cuda")
    moves = torch.full((n + 1, 128), -1, dtype=torch.int16, device="cuda")
    counts = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    if idx is None:
        hip.samples_to_requests(store[:n], None, out=(x[:n], moves[:n], counts[:n]))
    else:
        hip.samples_to_requests(store, _t(idx), out=(x[:n], moves[:n], counts[:n]))
    torch.cuda.synchronize()
    xs, ms, cs = x.cpu().numpy(), moves.cpu().numpy().view(np.uint16), counts.cpu().numpy()
    assert (xs[n] == 7.0).all() and (ms[n] == 0xFFFF).all() and cs[n] == -5
    for j, r in enumerate(rows):
        s = smp[r]
        m = int(s["n_moves"])
        assert xs[j].tobytes() == F.encode_planes(s["board"], int(s["side"])).tobytes(), (j, r)
        assert cs[j] == m and (ms[j, :m] == s["actions"][:m]).all() and (ms[j, m:] == 0).all(), (j, r)
    assert store.cpu().numpy().tobytes() == _raw(smp).tobytes()      # the records are only read


# ---- 2. the score kernel ----------------------------------------------------------------------------------------------------------
def _check_scores(got, ref, rows, value, label):
    """got: SCORE_DTYPE rows of the kernel; ref: the float64 reference rows of the same records."""
    worst = 0.0
    for j, r in enumerate(rows):
        g, w = got[j], ref[r]
        assert g["valid"] == w["valid"] and g["zero"].tolist() == [0, 0], (label, j, r)
        if not w["valid"]:
            assert g.tobytes() == bytes(16), (label, j, r)
            continue
        assert g["top1"] == w["top1"] and g["value"].tobytes() == np.float32(value[r]).tobytes(), (label, j, r)
        slack = 1e-12 * (w["policy_ce"] + w["entropy"] + 1.0)
        for f in ("policy_kl", "policy_ce"):
            err, bound = abs(float(g[f]) - w[f]), 2.0 ** -23 * abs(w[f]) + slack
            worst = max(worst, err / bound)
            assert err <= bound, (label, f, j, r, float(g[f]), w[f], err, bound)
        assert g["policy_kl"] >= 0.0
    return worst


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_score_samples_against_the_float64_reference(n):
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    smp, logits, value, notes, ref = _pool()
    if n == 130:                                                     # the whole pool: every kind, every move count
        assert {(notes[k], int(smp[k]["n_moves"])) for k in range(POOL)} >= {(kind, m) for kind in ("late_temp", "gumbel", "spread80")
                                                                            for m in (2, 64, 65, 128)}
        assert {int(s["n_moves"]) for s in smp} == set(N_MOVES)
        inside = [k for k in range(POOL) if notes[k] == "nonfinite_inside" and smp[k]["n_moves"] > 0]
        behind = [k for k in range(POOL) if notes[k] == "nonfinite_behind" and 0 < smp[k]["n_moves"] < 128]
        assert len(inside) >= 3 and len(behind) >= 3 and not ref["valid"][inside].any() and ref["valid"][behind].all()
        assert any(notes[k] == "zero_visits" and (smp[k]["visits"][:smp[k]["n_moves"]] == 0).any() for k in range(POOL))
    for kind, idx in (("none", None), ("rows", {1: [3], 3: [3, 0, 12]}.get(n, _indices(n, "repeats")))):
        rows = np.arange(n) if idx is None else np.asarray(idx, dtype=np.int32)
        used = smp[:n] if idx is None else smp
        lg, vl = _t(logits[rows]), _t(value[rows])
        # write_back = 0: scores only, the records stay byte for byte
        store = _t(_raw(used))
        out = hip.score_samples(store, None if idx is None else _t(rows), lg, vl, 0.3, write_back=False)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(F.SCORE_DTYPE).reshape(-1)
        worst = _check_scores(got, ref, rows, value, (n, kind))
        print("n", n, kind, "largest error / bound:", worst)
        assert store.cpu().numpy().tobytes() == _raw(used).tobytes()
        # write_back = 1: the same scores, the eight bytes of every valid row's record, and nothing else
        out1 = hip.score_samples(store, None if idx is None else _t(rows), lg, vl, 0.3, write_back=True)
        torch.cuda.synchronize()
        assert out1.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
        after = store.cpu().numpy()
        want = _raw(used).copy()
        for j, r in enumerate(rows):
            if got[j]["valid"]:
                ps = np.zeros((), dtype=F.POLICY_STATS_DTYPE)
                ps["policy_kl"], ps["has_policy_stats"], ps["prior_top1"] = got[j]["policy_kl"], 1, got[j]["top1"]
                want[r if idx is not None else j, 120:128] = np.frombuffer(ps.tobytes(), np.uint8)
        assert after.tobytes() == want.tobytes()
        rec = after.view(F.SAMPLE_DTYPE).reshape(-1)
        assert (F.root_stats(rec)["has_root_stats"] == 1).all() and (after[:, 116] == 1).all()     # byte 116 and the root fields
        assert F.root_stats(rec)["root_q"].tobytes() == F.root_stats(used)["root_q"].tobytes()
        marks = F.policy_stats(rec)
        touched = np.zeros(len(used), bool)
        touched[[r if idx is not None else j for j, r in enumerate(rows) if got[j]["valid"]]] = True
        assert (marks["has_policy_stats"] == touched).all()
        if idx is None:
            written = want
    # scores may be NULL when writing back: the records end up as after the call above
    import ctypes as C
    store = _t(_raw(smp[:n]))
    opts = hip.ScoreOpts(0.3, 1, 0)
    lg, vl = _t(logits[:n]), _t(value[:n])
    hip.check(hip.lib().xq_score_samples(store.data_ptr(), None, n, lg.data_ptr(), vl.data_ptr(), C.byref(opts), None,
                                         hip.stream_ptr(store.device)), "xq_score_samples")
    torch.cuda.synchronize()
    assert store.cpu().numpy().tobytes() == written.tobytes()


def test_score_samples_late_temperature_is_the_argument():
    """Another T gives another target for the late_temp records only."""
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    smp, logits, value, notes, _ = _pool()
    ref = F.sample_scores(smp, logits, value, 1.0)
    out = hip.score_samples(_t(_raw(smp)), None, _t(logits), _t(value), 1.0)
    torch.cuda.synchronize()
    _check_scores(out.cpu().numpy().view(F.SCORE_DTYPE).reshape(-1), ref, np.arange(POOL), value, "T=1")


def test_score_samples_overflowing_total_is_invalid():
    """T = 0.01 takes a late record's powers past float64: valid = 0, zeros, and the record is not marked; the same record at
    T = 0.3, and a record that is not late, score as ever."""
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    smp = np.zeros(2, dtype=F.SAMPLE_DTYPE)
    smp["n_moves"], smp["late_temp"] = 3, (1, 0)
    smp["actions"][:, :3], smp["visits"][:, :3] = (100, 101, 102), (60000, 50000, 7)
    logits = np.zeros((2, 128), np.float32)
    logits[:, :3] = (0.5, -1.0, 2.0)
    value = np.array([0.25, -0.5], np.float32)
    for T in (0.01, 0.3):
        ref = F.sample_scores(smp, logits, value, T)
        assert ref["valid"].tolist() == ([0, 1] if T == 0.01 else [1, 1])
        store = _t(_raw(smp))
        out = hip.score_samples(store, None, _t(logits), _t(value), T, write_back=True)
        torch.cuda.synchronize()
        _check_scores(out.cpu().numpy().view(F.SCORE_DTYPE).reshape(-1), ref, np.arange(2), value, ("overflow", T))
        marks = F.policy_stats(store.cpu().numpy().view(F.SAMPLE_DTYPE).reshape(-1))["has_policy_stats"]
        assert marks.tolist() == ref["valid"].tolist()


# ---- 3. the counts ----------------------------------------------------------------------------------------------------------------
def _host_counts(smp, alpha, seed, epoch):
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    ps = F.policy_stats(smp)
    _, marked, M, S = F.surprise_weights(smp, alpha)
    return np.array([hip.surprise_count_host(ps["policy_kl"][i], marked[i], M, S, alpha, seed, epoch, smp["slot"][i],
                                             smp["game_seq"][i], smp["ply"][i]) for i in range(len(smp))], dtype=np.int32)


@pytest.mark.parametrize("n", [1, 3, 65, 130, SUM_BLOCK + 1])
def test_surprise_counts_equal_the_host_twin(n):
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    smp = surprise_records(n, 40 + n)
    if n == 1:
        set_policy_stats(smp, np.float32(0.75), 1)
    store = _t(_raw(smp))
    seen = {}
    for alpha in (0.0, 0.5, 1.0):
        for seed, epoch in ((1, 0), (0xFEDCBA9876543210, 0), (1, 3)):
            got = hip.surprise_counts(store, alpha, seed, epoch).cpu().numpy()
            want = _host_counts(smp, alpha, seed, epoch)
            assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (alpha, seed, epoch)
            assert want.tobytes() == F.surprise_counts(smp, alpha, seed, epoch).tobytes()
            seen[(alpha, seed, epoch)] = got
        if alpha == 0.0:
            assert all((c == 1).all() for c in seen.values())
    unmarked = F.policy_stats(smp)["has_policy_stats"] != 1
    assert all((c[unmarked] == 1).all() for c in seen.values())
    if n >= 65:                                                      # two seeds and two epochs differ
        assert (seen[(0.5, 1, 0)] != seen[(0.5, 0xFEDCBA9876543210, 0)]).any() and (seen[(0.5, 1, 0)] != seen[(0.5, 1, 3)]).any()
        assert unmarked.any() and (~unmarked).any()
    zero = surprise_records(n, 40 + n, zero_kl=True)                 # all-zero KL: S = 0, every count 1
    assert (hip.surprise_counts(_t(_raw(zero)), 1.0, 1, 0).cpu().numpy() == 1).all()
    torch.cuda.synchronize()
    assert store.cpu().numpy().tobytes() == _raw(smp).tobytes()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def test_score_samples_end_to_end_against_a_float64_forward():
    import torch
    from xiangqi_alphazero_amd import evaluator, hip, model, selfplay, weights
    from xiangqi_alphazero_amd import sample_format as F
    net = model.XiangqiNet(64, 2)
    net.load_state_dict(weights.make_state_dict(64, 2, policy_gain=4.0))
    cfg = types.SimpleNamespace(num_simulations=16, c_puct=1.5, temperature_threshold=6, max_game_length=12, random_opening_moves=2,
                                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
    samples, results, st, _ = selfplay.run_games(net, cfg, 8, n_slots=8, seed=3, device_records=True)
    n = samples.shape[0]
    assert 8 <= n <= 8 * 12 and results.shape[0] == 8
    before = samples.cpu().numpy().copy()
    rec = before.view(F.SAMPLE_DTYPE).reshape(-1)
    ev = evaluator.make_evaluator(net, "cuda", "hip")[0]
    # the evaluator is not code under test: its distance from a float64 forward of the same network is measured here
    x, moves, counts = hip.samples_to_requests(samples)
    ll, v = (t.clone() for t in ev.evaluate_legal(x, moves, counts))
    net64 = model.XiangqiNet(64, 2).double().cuda().eval()
    net64.load_state_dict({k: t.double() if t.is_floating_point() else t for k, t in net.state_dict().items()})
    with torch.no_grad():
        l64, v64 = net64(x.double())
    l64 = torch.gather(l64, 1, moves.view(torch.int16).to(torch.int64) & 0xFFFF).cpu().numpy()
    mask = np.arange(128)[None, :] < rec["n_moves"][:, None]
    d = float(np.abs(ll.cpu().numpy().astype(np.float64) - l64)[mask].max())
    print("samples", n, "max |logit_evaluator - logit_float64| over the legal moves:", d)
    assert d < 1e-3                                                  # a sanity line, not the bound: the fp32 evaluator is close
    ref = F.sample_scores(rec, l64, v64.cpu().numpy().reshape(-1), 0.3)
    assert ref["valid"].all()
    for chunk in (2048, 5):                                          # one chunk, and many with a short last one
        store = samples.clone()
        scores = selfplay.score_samples(ev, store, 0.3, write_back=True, chunk=chunk)
        torch.cuda.synchronize()
        assert scores.shape == (n, 16) and scores.dtype == torch.uint8 and scores.is_cuda
        got = scores.cpu().numpy().view(F.SCORE_DTYPE).reshape(-1)
        assert got["valid"].all()
        for f in ("policy_kl", "policy_ce"):
            err = np.abs(got[f].astype(np.float64) - ref[f])
            bound = 2.0 * d + 2.0 ** -23 * np.abs(ref[f])
            print(chunk, f, "largest error", err.max(), "bound there", bound[np.argmax(err)])
            assert (err <= bound).all(), (chunk, f)
        top2 = np.sort(np.where(mask, l64, -np.inf), axis=1)[:, -2:]
        clear = (rec["n_moves"] == 1) | (top2[:, 1] - top2[:, 0] > 2.0 * d)
        print(chunk, "top1 compared on", int(clear.sum()), "of", n)
        assert (~clear).sum() * 4 <= n and (got["top1"][clear] == ref["top1"][clear]).all()
        if chunk == 2048:                                            # the same rows in one launch as above: the evaluator's own value
            assert got["value"].tobytes() == v.cpu().numpy().tobytes()
        # the returned scores are the ones written back, and nothing else in the records moved
        after = store.cpu().numpy()
        marks = F.policy_stats(after.view(F.SAMPLE_DTYPE).reshape(-1))
        assert (marks["has_policy_stats"] == 1).all() and marks["policy_kl"].tobytes() == got["policy_kl"].tobytes()
        assert (marks["prior_top1"] == got["top1"]).all() and (marks["zero"] == 0).all()
        after[:, 120:128] = before[:, 120:128]
        assert after.tobytes() == before.tobytes()
    summary = selfplay.score_summary(scores, store)
    assert summary["scored_samples"] == n and abs(summary["mean_policy_kl"] - float(got["policy_kl"].astype(np.float64).mean())) < 1e-9
    assert abs(summary["value_mse_vs_z"] - float(((got["value"].astype(np.float64) - rec["z"]) ** 2).mean())) < 1e-9
    assert abs(summary["prior_top1_rate"] - float(got["top1"].mean())) < 1e-12
    # write_back = False leaves the records alone
    store = samples.clone()
    selfplay.score_samples(ev, store, write_back=False)
    assert store.cpu().numpy().tobytes() == before.tobytes()


# ---- 5. the train step ------------------------------------------------------------------------------------------------------------
def _net_and_optimizer():
    import torch
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(16, 1)
    net.load_state_dict(weights.make_state_dict(16, 1, seed=11))
    net = net.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4)
    return net, opt, torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.1)


def _training_records():
    smp = np.array(_pool()[0])                                       # a writable copy
    rng = np.random.default_rng(9)
    set_policy_stats(smp, rng.exponential(0.7, POOL).astype(np.float32), (rng.random(POOL) < 0.7).astype(np.uint8))
    return smp


def test_train_network_weight_zero_is_the_run_without_the_keyword():
    import torch
    from xiangqi_alphazero_amd import training
    cfg = types.SimpleNamespace(min_buffer_size=10, num_epochs=1, batch_size=32)
    buf = training.ReplayBuffer(50000)
    buf.extend(_training_records()[:32])
    end = []
    # the library's convolutions are held to their deterministic algorithms for the comparison, and one discarded run goes first:
    # the first convolution of a shape in a process may be served by another algorithm than every later one
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for kw in ({}, {}, dict(surprise_weight=0.0)):
            net, opt, sch = _net_and_optimizer()
            gen = torch.Generator().manual_seed(5)
            stats = [training.train_network(net, opt, sch, buf, cfg, generator=gen, **kw) for _ in range(2)]    # two steps
            assert all(s["policy_surprise_weight"] == 0.0 and s["policy_stats_coverage"] is None and s["epoch_samples"] == [64]
                       for s in stats)
            end.append((stats, {k: t.cpu().numpy().tobytes() for k, t in net.state_dict().items()}, gen.get_state().numpy().tobytes()))
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was
    for other in end[2:]:
        differing = [k for k in end[1][1] if end[1][1][k] != other[1][k]]
        print("weights that differ between the run without the keyword and the run at weight 0:", differing)
        assert not differing and end[1][0] == other[0] and end[1][2] == other[2]      # the generator was drawn from as often


def test_train_network_epoch_draws_the_reference_counts():
    import torch
    from xiangqi_alphazero_amd import training
    from xiangqi_alphazero_amd import sample_format as F
    smp = _training_records()
    buf = training.ReplayBuffer(200)                                 # 100 records: the ring wraps and its oldest record is row 30
    buf.extend(smp[:60].copy())
    buf.extend(smp[60:].copy())
    assert buf.count == 100 and buf.head == 30
    live = smp[30:]                                                  # oldest first
    assert buf.policy_stats_coverage() == float((F.policy_stats(live)["has_policy_stats"] == 1).mean())
    cfg = types.SimpleNamespace(min_buffer_size=10, num_epochs=2, batch_size=64, policy_surprise_weight=0.5)
    seen = []
    batch = buf.batch
    buf.batch = lambda logical, q_mix=0.0: (seen.append(logical.clone()), batch(logical, q_mix))[1]
    net, opt, sch = _net_and_optimizer()
    stats = training.train_network(net, opt, sch, buf, cfg, generator=torch.Generator().manual_seed(5))       # the config's key
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=torch.Generator().manual_seed(5)).item())
    want = [F.surprise_counts(live, 0.5, seed, e) for e in (0, 1)]
    assert (want[0] != want[1]).any() and (want[0] != 1).any()
    assert stats["policy_surprise_weight"] == 0.5 and stats["policy_stats_coverage"] == buf.policy_stats_coverage()
    assert stats["epoch_samples"] == [2 * int(w.sum()) for w in want]
    drawn = torch.cat(seen).numpy()
    first = drawn[:stats["epoch_samples"][0]]
    expansion = np.repeat(np.arange(200), np.repeat(want[0], 2))
    assert np.array_equal(np.sort(first), expansion)                 # the multiset of epoch 0
    assert np.array_equal(np.sort(drawn[stats["epoch_samples"][0]:]), np.repeat(np.arange(200), np.repeat(want[1], 2)))
    assert not np.array_equal(first, expansion)                      # ... permuted
    halves = np.bincount(first, minlength=200).reshape(100, 2)
    assert (halves[:, 0] == halves[:, 1]).all() and (halves[:, 0] == want[0]).all()    # both mirror halves equally often
    # logical sample 2 r is live record r: the ring's oldest record first
    idx, flip = buf._record_of(torch.tensor([0, 1, 199]))
    assert idx.tolist() == [30, 30, 29] and flip.tolist() == [0, 1, 1]
    assert buf.store[30].cpu().numpy().tobytes() == _raw(live[:1]).tobytes()
    order = buf.epoch_order(0.5, seed, 0, torch.Generator().manual_seed(1), shuffle=False)
    assert np.array_equal(order.numpy(), expansion)
