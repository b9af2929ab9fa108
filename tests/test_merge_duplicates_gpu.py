"""GPU checks of merging duplicate positions: the key kernel against the host twin bit for bit; the head kernel against the numpy
predecessor rule (made-up equal keys, equal boards with different sides, mirror pairs); groups of one byte-identical to
xq_samples_to_batch_ex; larger groups against sample_format.merged_targets; ReplayBuffer.position_groups / batch_groups on a
wrapped ring; and train_network end to end on engine games."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from golden_io import corpus
from merge_duplicates_records import group_buffer, key_records, make_group, mirror_board, records_of
from policy_surprise_records import score_records

pytestmark = pytest.mark.gpu

T = 0.3


def _dev(smp):
    import torch
    return torch.from_numpy(np.ascontiguousarray(smp).view(np.uint8).reshape(len(smp), 640).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _host_keys(mirror: bool):
    from xiangqi_alphazero_amd import hip
    smp = key_records()
    return [hip.position_key_host(s["board"], int(s["side"]), mirror) for s in smp]


# ---- 1. keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", (False, True))
@pytest.mark.parametrize("n", (0, 1, 3, 4, 5, 257))
def test_position_keys_equal_the_host_twin(n, mirror):
    import torch
    from xiangqi_alphazero_amd import hip
    smp = key_records()
    assert len(smp) == 257
    store = _dev(smp)
    host = _host_keys(mirror)
    # without an index: the first n records; with one: n records from the far end, out of order, one of them twice
    keys, mir = hip.position_keys(store[:n], None, mirror)
    rows = np.arange(n)
    if n:
        rows = (np.arange(n) * 101 + 256) % 257
        rows[-1] = rows[0]
    keys_i, mir_i = hip.position_keys(store, torch.from_numpy(rows.astype(np.int32)).cuda(), mirror)
    torch.cuda.synchronize()
    for got_k, got_m, which in ((keys, mir, np.arange(n)), (keys_i, mir_i, rows)):
        assert got_k.shape == (n,) and got_m.shape == (n,)
        assert got_k.cpu().numpy().view(np.uint64).tolist() == [host[r][0] for r in which]
        assert got_m.cpu().numpy().tolist() == [host[r][1] for r in which]


# ---- 2. heads -----------------------------------------------------------------------------------------------------------------------
def test_group_heads_equal_the_reference():
    import torch
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd import sample_format as F
    d = corpus()
    a, b, c = (d["board"][i].astype(np.int8) for i in (10, 2000, 3000))
    boards = [a, b, a, mirror_board(a), b, b, c, mirror_board(c), mirror_board(c), a, c]
    sides = [1, 1, 1, 1, -1, -1, 1, 1, -1, 1, 1]
    smp = records_of(np.array(boards), np.array(sides, dtype=np.int8))
    n = len(smp)
    store = _dev(smp)
    real, mir = hip.position_keys(store, None, True)
    made_up = torch.full((n,), 12345, dtype=torch.int64, device="cuda")
    half = made_up.clone()
    half[n // 2:] = -7                                                  # two runs of equal keys; a negative int64 is a large uint64
    mir_np = mir.cpu().numpy()
    assert mir_np.tolist() == [F.position_key(s["board"], int(s["side"]), True)[1] for s in smp]
    for keys in (made_up, half, real):
        keys_np = keys.cpu().numpy().view(np.uint64)
        for order_np in (np.argsort(keys_np, kind="stable"), np.arange(n)[::-1].copy()):     # the sorted order, and any other
            order = torch.from_numpy(order_np.astype(np.int32)).cuda()
            head = hip.position_group_heads(store, None, order, keys, mir)
            torch.cuda.synchronize()
            want = F.position_group_heads(smp, order_np, keys_np, mir_np)
            assert head.cpu().numpy().tolist() == want.tolist(), (keys_np[:2], order_np)
    # A, B, A under one key: three groups and more; under the real keys the four records of A are one group
    order = torch.arange(n, dtype=torch.int32, device="cuda")
    assert hip.position_group_heads(store, None, order, made_up, mir).cpu().numpy().tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1, 1, 1]
    # through an index: rows are records index[row]
    index = torch.from_numpy(np.arange(n)[::-1].astype(np.int32).copy()).cuda()
    k2, m2 = hip.position_keys(store, index, True)
    order_np = np.argsort(k2.cpu().numpy().view(np.uint64), kind="stable")
    head = hip.position_group_heads(store, index, torch.from_numpy(order_np.astype(np.int32)).cuda(), k2, m2)
    want = F.position_group_heads(smp[::-1], order_np, k2.cpu().numpy().view(np.uint64), m2.cpu().numpy())
    assert head.cpu().numpy().tolist() == want.tolist() and int(want.sum()) == 5      # A, B, B-, C, C-


# ---- 3. groups of one ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single_records():
    smp = score_records(63, 7)[0]                                       # every n_moves of N_MOVES with every kind
    smp.setflags(write=False)
    return smp


def _plain(store, idx, flip, q_mix):
    import torch
    from xiangqi_alphazero_amd import hip
    b = idx.shape[0]
    states = torch.empty((b, 15, 10, 9), dtype=torch.float32, device="cuda")
    pi = torch.empty((b, 8100), dtype=torch.float32, device="cuda")
    z = torch.empty((b, 1), dtype=torch.float32, device="cuda")
    opts = hip.BatchOpts(float(q_mix))
    hip.check(hip.lib().xq_samples_to_batch_ex(store.data_ptr(), idx.data_ptr(), flip.data_ptr(), b, T, C.byref(opts),
                                               states.data_ptr(), pi.data_ptr(), z.data_ptr(), hip.stream_ptr(store.device)),
              "xq_samples_to_batch_ex")
    return states, pi, z


@pytest.mark.parametrize("q_mix", (0.0, 0.25))
def test_groups_of_one_are_the_plain_kernel_byte_for_byte(q_mix):
    import torch
    from xiangqi_alphazero_amd import hip
    smp = _single_records()
    n = len(smp)
    store = _dev(smp)
    offsets = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    members = torch.arange(n, dtype=torch.int32, device="cuda").flip(0).contiguous()      # group g is record n - 1 - g
    for mirrored in (0, 1):
        mm = torch.full((n,), mirrored, dtype=torch.uint8, device="cuda")
        logical = torch.arange(2 * n, device="cuda")
        group, flip = (logical // 2).to(torch.int32), (logical % 2).to(torch.uint8)
        got = hip.groups_to_batch(store, offsets, members, mm, group, flip, T, q_mix)
        want = _plain(store, members[group.long()].contiguous(), flip ^ mirrored, q_mix)
        torch.cuda.synchronize()
        for name, g, w in zip(("planes", "pi", "z"), got, want):
            assert g.shape == w.shape and g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (name, mirrored)


# ---- 4. larger groups ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merged_reference(late: bool, q_mix: float):
    """The numpy reference of every group of the shared buffer under both flips, then the three rows that must be zeros."""
    from xiangqi_alphazero_amd import sample_format as F
    smp, groups, notes = group_buffer(late)
    n_groups = len(groups[0]) - 1
    group = np.array([g for g in range(n_groups) for _ in (0, 1)] + [-1, n_groups, n_groups + 5], dtype=np.int32)
    flip = (np.arange(len(group)) % 2).astype(np.uint8)
    return group, flip, F.merged_targets(smp, groups, group, flip, T, q_mix)


@pytest.mark.parametrize("q_mix", (0.0, 0.25))
@pytest.mark.parametrize("late", (False, True))
def test_larger_groups_equal_the_reference(late, q_mix):
    import torch
    from xiangqi_alphazero_amd import hip
    smp, (offsets, members, mirrored), notes = group_buffer(late)
    group, flip, (st, pi, z) = _merged_reference(late, q_mix)
    sizes = np.diff(offsets)
    assert {2, 3, 64, 65, 200, 5, 1} <= set(sizes.tolist())
    store = _dev(smp)
    dev = [torch.from_numpy(a).cuda() for a in (offsets, members, mirrored, group, flip)]
    got_st, got_pi, got_z = (t.cpu().numpy() for t in hip.groups_to_batch(store, *dev, T, q_mix))
    assert got_st.tobytes() == st.tobytes()
    got_z = got_z.reshape(-1)
    assert not got_st[-3:].any() and not got_pi[-3:].any() and not got_z[-3:].any()
    for j, g in enumerate(group[:-3]):
        mem = members[offsets[g]:offsets[g + 1]]
        has_late = bool(smp["late_temp"][mem].any())
        err = np.abs(got_pi[j].astype(np.float64) - pi[j].astype(np.float64))
        print("group", int(g), "size", len(mem), "flip", int(flip[j]), "late" if has_late else "T=1", "max |pi - ref|", err.max())
        if has_late:                                                  # pow: the tolerance tests/test_training.py grants the plain kernel
            np.testing.assert_allclose(got_pi[j], pi[j], rtol=2e-7, atol=0)
        else:
            assert got_pi[j].tobytes() == pi[j].tobytes(), (int(g), len(mem))
        assert got_z[j].tobytes() == z[j].tobytes(), (int(g), len(mem))
    # the group whose members are all invalid: zeros in pi, the mean in z; the one with some invalid: a distribution
    all_invalid = [j for j, g in enumerate(group[:-3]) if sizes[g] == 3 and not pi[j].any()]
    assert len(all_invalid) == 2 and not got_pi[all_invalid].any()
    # an empty group gives zeros and reads no record
    off_e = offsets.copy()
    off_e[1:] = off_e[0]
    out = hip.groups_to_batch(store, torch.from_numpy(off_e).cuda(), dev[1], dev[2], dev[3], dev[4], T, q_mix)
    assert all(not t.cpu().numpy().any() for t in out)


# ---- 5. the replay buffer -----------------------------------------------------------------------------------------------------------
def test_replay_buffer_groups_on_a_wrapped_ring():
    import torch
    from xiangqi_alphazero_amd import training
    from xiangqi_alphazero_amd import sample_format as F
    rng = np.random.default_rng(3)
    d = corpus()
    a, b, c = ((d["board"][i].astype(np.int8), int(d["side"][i])) for i in (40, 900, 2500))
    smp = np.concatenate([make_group(*a, 4, rng), make_group(*b, 2, rng), make_group(*c, 1, rng), make_group(*a, 2, rng),
                          make_group(*b, 2, rng, ("late_temp",))])
    smp = smp[rng.permutation(11)]
    buf = training.ReplayBuffer(16)                                      # 8 records
    buf.extend(smp[:5])
    buf.extend(smp[5:])                                                  # 11 extended: the ring has wrapped
    assert buf.count == 8 and buf.head == 3
    live = smp[3:]                                                       # oldest first
    for mirror in (True, False):
        groups = buf.position_groups(mirror)
        offsets, members, mirrored = F.position_groups(live, mirror)
        assert groups.n_groups == len(offsets) - 1 and groups.n_records == 8
        assert groups.offsets.cpu().numpy().tolist() == offsets.tolist()
        assert groups.members.cpu().numpy().tolist() == ((members + 3) % 8).tolist()          # ring indices
        assert groups.member_mirrored.cpu().numpy().tolist() == mirrored.tolist()
        assert groups.sizes.cpu().numpy().tolist() == np.diff(offsets).tolist()
        logical = torch.randperm(2 * groups.n_groups, generator=torch.Generator().manual_seed(1))
        st, pi, z = (t.cpu().numpy() for t in buf.batch_groups(groups, logical.cuda(), 0.25))
        lg = logical.numpy()
        rst, rpi, rz = F.merged_targets(live, (offsets, members, mirrored), lg // 2, lg % 2, buf.late_temperature, 0.25)
        assert st.tobytes() == rst.tobytes() and z.shape == (len(lg), 1) and z.reshape(-1).tobytes() == rz.tobytes()
        np.testing.assert_allclose(pi, rpi, rtol=2e-7, atol=0)
    assert buf.position_groups(True).n_groups < buf.position_groups(False).n_groups <= 8
    assert training.ReplayBuffer(16).position_groups().n_groups == 0


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
def _net_and_optimizer():
    import torch
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(16, 1)
    net.load_state_dict(weights.make_state_dict(16, 1, seed=11))
    net = net.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4)
    return net, opt, torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.1)


def test_train_network_on_engine_games():
    """Most of this test's time is the process' first train step of the 16x1 network at batch 32 (the convolution library's
    algorithm search: about 5 s measured, against 0.01 s for the second call); the later train tests of the suite use the same
    shapes and no longer pay it."""
    import torch
    from xiangqi_alphazero_amd import model, selfplay, training, weights
    from xiangqi_alphazero_amd import sample_format as F
    player = model.XiangqiNet(64, 2)
    player.load_state_dict(weights.make_state_dict(64, 2, policy_gain=4.0))
    cfg = types.SimpleNamespace(num_simulations=16, c_puct=1.5, temperature_threshold=6, max_game_length=10, random_opening_moves=0,
                                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
    samples, results, _, _ = selfplay.run_games(player, cfg, 4, n_slots=4, seed=3, device_records=True)
    rec = samples.cpu().numpy().view(F.SAMPLE_DTYPE).reshape(-1)
    # the shortest prefix of the records with 16 distinct positions: every batch of the merged epochs is then a full batch of 32,
    # the one batch shape the other train tests use (a new shape costs the convolution library seconds of algorithm search)
    k = next(k for k in range(16, len(rec) + 1) if len(F.position_groups(rec[:k], True)[0]) - 1 == 16)
    rec = rec[:k]
    buf = training.ReplayBuffer(50000)
    buf.extend(samples[:k])
    offsets, members, _ = F.position_groups(rec, True)
    n_groups = len(offsets) - 1
    tcfg = dict(min_buffer_size=10, num_epochs=2, batch_size=32)
    net, opt, sch = _net_and_optimizer()
    on = training.train_network(net, opt, sch, buf, types.SimpleNamespace(merge_duplicate_positions=True, **tcfg),
                                generator=torch.Generator().manual_seed(5))
    print("records", len(rec), "distinct positions", on["distinct_positions"], "largest group", on["largest_group"])
    assert on["merge_duplicate_positions"] is True and on["distinct_positions"] == n_groups < len(rec)
    assert on["epoch_samples"] == [2 * on["distinct_positions"]] * 2
    assert on["largest_group"] == int(np.diff(offsets).max()) >= 2       # the initial position is in every game
    assert on["merged_records"] == len(rec) - n_groups
    assert all(np.isfinite(on[k]) for k in ("policy_loss", "value_loss", "total_loss"))
    assert buf.position_groups(False).n_groups == len(F.position_groups(rec, False)[0]) - 1 >= n_groups
    # off: the stats and the trained weights of a run with the keys absent (16 records: full batches of 32 again)
    rec = rec[:16]
    buf = training.ReplayBuffer(50000)
    buf.extend(samples[:16])
    end = []
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        # one discarded run goes first: the first convolution of a shape in a process may be served by another algorithm
        for extra, kw in (({}, {}), ({}, {}), (dict(merge_duplicate_positions=False, merge_mirror_positions=True), {})):
            net, opt, sch = _net_and_optimizer()
            gen = torch.Generator().manual_seed(5)
            stats = [training.train_network(net, opt, sch, buf, types.SimpleNamespace(**tcfg, **extra), generator=gen, **kw)]
            assert all(s["merge_duplicate_positions"] is False and s["distinct_positions"] is None and s["merged_records"] is None
                       and s["largest_group"] is None and s["epoch_samples"] == [2 * len(rec)] * 2 for s in stats)
            end.append((stats, {k: t.cpu().numpy().tobytes() for k, t in net.state_dict().items()}, gen.get_state().numpy().tobytes()))
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was
    for other in end[2:]:
        differing = [k for k in end[1][1] if end[1][1][k] != other[1][k]]
        print("weights that differ between the run with the keys absent and the run with the option off:", differing)
        assert not differing and end[1][0] == other[0] and end[1][2] == other[2]
