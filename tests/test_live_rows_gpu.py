"""The packed self-play step on the GPU: every *_live evaluator kernel computes a live row bit-identically to its full-width
twin wherever the row sits in the batch and touches nothing past the live count; the engine's packed step (select ->
compact -> evaluator over n_live rows -> scatter -> expand) gives byte-identical games to the full-width stage loop; and
the evaluated row count follows the slots that asked for an evaluation."""
import numpy as np
import pytest

CAP = 1024
COUNTS = (0, 1, 2, 37, CAP - 1, CAP)
SENTINEL = np.float32(-12345.5)


def _perm_case(n, seed):
    """Row permutation: live row r of the packed batch holds source row perm[r] (shuffled, so rows move position)."""
    rng = np.random.default_rng(seed)
    return rng.permutation(CAP)[:n]


def _live_inputs(src, perm, n):
    """Packed copy of `src` rows perm[:n] at the front, NaN in every row past n."""
    import torch
    out = torch.full_like(src, float("nan"))
    if n:
        out[:n] = src[torch.from_numpy(perm).to(src.device)]
    return out


def _check(ref, got, perm, n):
    """Live rows: the bytes of the full-width result at the source row; rows past n: the sentinel, untouched."""
    r, g = ref.cpu().numpy(), got.cpu().numpy()
    assert g[:n].tobytes() == r[perm].tobytes()
    assert (g[n:].view(np.uint32) == np.full(g[n:].shape, SENTINEL, np.float32).view(np.uint32)).all()


def _n(n):
    import torch
    return torch.tensor([n], dtype=torch.int32, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["narrow", "wide", "narrow_rev", "wide_rev", "bf16", "bf16_rev"])
def test_conv_live_rows_bitwise(variant):
    import torch
    from xiangqi_alphazero_amd import hip
    torch.manual_seed(3)
    c = 128
    w = torch.randn(c, c, 3, 3) * 0.05
    if variant.startswith("bf16"):
        u, launch = hip.wino_transform_weights_bf16(w.cuda()), hip.wino_conv3x3_bf16
    else:
        u, launch = hip.wino_transform_weights(w, 128 if variant.startswith("wide") else 64).cuda(), hip.wino_conv3x3
    rev = variant.endswith("_rev")
    bias = (torch.randn(c) * 0.1).cuda()
    x = torch.randn(CAP, 90, c, device="cuda")
    res = torch.randn(CAP, 90, c, device="cuda")
    ref = torch.empty_like(x)
    launch(x, u, bias, ref, res, True, rev)
    for i, n in enumerate(COUNTS):
        perm = _perm_case(n, i)
        xl, rl = _live_inputs(x, perm, n), _live_inputs(res, perm, n)
        out = torch.full_like(x, float(SENTINEL))
        launch(xl, u, bias, out, rl, True, rev, n_live=_n(n))
        _check(ref, out, perm, n)


@pytest.mark.gpu
def test_stem_heads_policy_value_live_rows_bitwise():
    import torch
    from xiangqi_alphazero_amd import hip
    torch.manual_seed(4)
    c = 128
    planes = (torch.rand(CAP, 15, 10, 9, device="cuda") < 0.08).float()
    planes[:, 14] = (torch.rand(CAP, device="cuda") < 0.5).float()[:, None, None]
    wt = (torch.randn(135, c) * 0.2).cuda()
    b_in = (torch.randn(c) * 0.1).cuda()
    h = torch.randn(CAP * 90, c, device="cuda").relu()
    w_pv = (torch.randn(36, c) * 0.1).cuda()
    b_pv = (torch.randn(36) * 0.1).cuda()
    feat = torch.randn(CAP, 2880, device="cuda").relu()
    fc_w = (torch.randn(8100, 2880) * 0.02).cuda()
    fc_b = (torch.randn(8100) * 0.1).cuda()
    moves = torch.randint(0, 8100, (CAP, 128), dtype=torch.int32, device="cuda").to(torch.int16)
    counts = torch.randint(0, 70, (CAP,), dtype=torch.int32, device="cuda")
    vfeat = torch.randn(CAP, 360, device="cuda").relu()
    w1t = (torch.randn(360, 128) * 0.05).cuda()
    b1 = (torch.randn(128) * 0.1).cuda()
    w2 = (torch.randn(128) * 0.1).cuda()
    b2 = (torch.randn(1) * 0.1).cuda()

    stem_ref = torch.empty(CAP, 90, c, device="cuda")
    hip.stem_conv(planes, wt, b_in, stem_ref)
    p_ref, v_ref = hip.heads_1x1(h, w_pv, b_pv)
    pol_ref = torch.full((CAP, 128), float(SENTINEL), device="cuda")
    hip.policy_head_legal(feat, fc_w, fc_b, moves, counts, pol_ref)
    val_ref = hip.value_head(vfeat, w1t, b1, w2, b2)
    for i, n in enumerate(COUNTS):
        perm = _perm_case(n, 10 + i)
        tp = torch.from_numpy(perm).cuda()
        nl = _n(n)
        out = torch.full((CAP, 90, c), float(SENTINEL), device="cuda")
        hip.stem_conv(_live_inputs(planes, perm, n), wt, b_in, out, nl)
        _check(stem_ref, out, perm, n)

        hl = _live_inputs(h.view(CAP, 90, c), perm, n).view(CAP * 90, c)
        p = torch.full((CAP * 90, 32), float(SENTINEL), device="cuda")
        v = torch.full((CAP * 90, 4), float(SENTINEL), device="cuda")
        hip.heads_1x1(hl, w_pv, b_pv, nl, out=(p, v))
        _check(p_ref.view(CAP, 90, 32), p.view(CAP, 90, 32), perm, n)
        _check(v_ref.view(CAP, 90, 4), v.view(CAP, 90, 4), perm, n)

        ml = torch.full_like(moves, -1)                 # past n: out-of-range action ids and counts
        cl = torch.full_like(counts, 128)
        if n:
            ml[:n], cl[:n] = moves[tp], counts[tp]
        pol = torch.full((CAP, 128), float(SENTINEL), device="cuda")
        hip.policy_head_legal(_live_inputs(feat, perm, n), fc_w, fc_b, ml, cl, pol, nl)
        _check(pol_ref, pol, perm, n)

        val = torch.full((CAP,), float(SENTINEL), device="cuda")
        hip.value_head(_live_inputs(vfeat, perm, n), w1t, b1, w2, b2, nl, out=val)
        _check(val_ref, val, perm, n)


@pytest.mark.gpu
@pytest.mark.parametrize("channels,blocks", [(64, 2), (128, 6)])
def test_evaluator_live_rows_bitwise(channels, blocks):
    import torch
    from xiangqi_alphazero_amd import hip_net, model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=4.0))
    ev = hip_net.HipResNetEvaluator(net, "cuda", engine_policy=True)
    assert ev.live_rows
    cap = 256
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(cap, 15, 10, 9, generator=g) < 0.06).float().cuda()
    moves = torch.randint(0, 8100, (cap, 128), dtype=torch.int32, generator=g).to(torch.int16).cuda()
    counts = torch.randint(1, 60, (cap,), dtype=torch.int32, generator=g).cuda()
    ll_ref, v_ref = ev.evaluate_legal(x, moves, counts)
    ll_ref, v_ref = ll_ref.clone(), v_ref.clone()
    keep = torch.arange(128, device="cuda")[None, :] < counts[:, None]
    for i, n in enumerate((0, 1, 37, cap - 1, cap)):
        perm = np.random.default_rng(20 + i).permutation(cap)[:n]
        tp = torch.from_numpy(perm).cuda()
        xl = torch.full_like(x, float("nan"))
        ml, cl = torch.full_like(moves, -1), torch.full_like(counts, 128)
        if n:
            xl[:n], ml[:n], cl[:n] = x[tp], moves[tp], counts[tp]
        ll, v = ev.evaluate_legal(xl, ml, cl, n_live=_n(n))
        got_ll = torch.where(keep[tp], ll[:n], 0.0).cpu().numpy()
        want_ll = torch.where(keep[tp], ll_ref[tp], 0.0).cpu().numpy()
        assert got_ll.tobytes() == want_ll.tobytes()
        assert v[:n].cpu().numpy().tobytes() == v_ref[tp].cpu().numpy().tobytes()


# ---- the engine step ---------------------------------------------------------------------------------------------------

def _sorted_records(eng):
    smp, res = eng.drain()
    return (np.sort(smp, order=["slot", "game_seq", "ply"]).tobytes(), np.sort(res, order=["slot", "game_seq"]).tobytes(),
            len(smp), len(res))


def _make(kind, channels, blocks, slots, sims, **cfg):
    from xiangqi_alphazero_amd import engine, evaluator, model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=4.0))
    ev, _ = evaluator.make_evaluator(net, "cuda", kind)
    return engine.SelfPlayEngine(engine.make_config(slots, sims, seed=9, **cfg), "cuda", evaluator=ev), ev


def _full_width_run(kind, channels, blocks, slots, sims, steps=None, until_done=None, **cfg):
    """The explicit full-width stage loop (as bench.py's headline region drives it)."""
    eng, ev = _make(kind, channels, blocks, slots, sims, **cfg)
    n = 0
    while True:
        x = eng.select()
        ll, v = ev.evaluate_legal(x, eng.req_moves, eng.req_counts)
        eng.expand_legal(ll, v)
        n += 1
        if steps is not None and n >= steps:
            break
        if until_done is not None and n % 32 == 0 and eng.stats()["games_finished"] >= until_done:
            break
    st = eng.stats()
    return n, st, _sorted_records(eng)


def _packed_run(kind, channels, blocks, slots, sims, steps, graph, **cfg):
    eng, _ = _make(kind, channels, blocks, slots, sims, **cfg)
    assert eng.path == "packed"
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while eng.steps < steps:
        eng.step()
    st = eng.stats()
    return eng, st, _sorted_records(eng)


def _same(st_full, rec_full, st_packed, rec_packed):
    a = {k: v for k, v in st_full.items() if k != "rows_evaluated"}
    b = {k: v for k, v in st_packed.items() if k != "rows_evaluated"}
    assert a == b
    assert st_full["rows_evaluated"] == 0
    assert rec_full == rec_packed


@pytest.mark.gpu
def test_packed_step_equals_full_width_with_a_tail():
    """(a) 64x3, 256 slots, games_target = 256: the run ends in a tail where slots go idle."""
    cfg = dict(games_target=256, max_game_length=60)
    k, st_f, rec_f = _full_width_run("hip", 64, 3, 256, 8, until_done=256, **cfg)
    assert st_f["games_finished"] == 256 and st_f["overflow"] == 0
    for graph in (False, True):
        eng, st_p, rec_p = _packed_run("hip", 64, 3, 256, 8, k, graph, **cfg)
        _same(st_f, rec_f, st_p, rec_p)
        assert 0 < st_p["rows_evaluated"] < k * 256


@pytest.mark.gpu
def test_packed_step_equals_full_width_refill_staggered():
    """(b) refilling slots with start_stagger: idle slots at the start instead of the end."""
    cfg = dict(start_stagger=True, max_game_length=60)
    _, st_f, rec_f = _full_width_run("hip", 64, 3, 256, 8, steps=160, **cfg)
    for graph in (False, True):
        _, st_p, rec_p = _packed_run("hip", 64, 3, 256, 8, 160, graph, **cfg)
        _same(st_f, rec_f, st_p, rec_p)


@pytest.mark.gpu
def test_packed_step_equals_full_width_bf16():
    """(c) the bf16 evaluator (k_wino_conv_bf16) at 128x2."""
    cfg = dict(games_target=256, max_game_length=40)
    k, st_f, rec_f = _full_width_run("bf16", 128, 2, 256, 8, until_done=256, **cfg)
    for graph in (False, True):
        _, st_p, rec_p = _packed_run("bf16", 128, 2, 256, 8, k, graph, **cfg)
        _same(st_f, rec_f, st_p, rec_p)


@pytest.mark.gpu
def test_mcts_search_many_packed_equals_full_width():
    """(d) MCTS.search_many on 64 positions: step() takes the packed path; the control hides `live_rows`."""
    import types
    from oracle import xq_oracle as O
    from xiangqi_alphazero_amd import evaluator, mcts, model, weights
    net = model.XiangqiNet(64, 2)
    net.load_state_dict(weights.make_state_dict(64, 2, policy_gain=4.0))
    ev, _ = evaluator.make_evaluator(net, "cuda", "hip")

    class FullWidth:                                   # the same evaluator without the live-row capability
        def __init__(self, inner):
            self.inner = inner

        def __call__(self, x):
            return self.inner(x)

        def evaluate_legal(self, x, moves, counts):
            return self.inner.evaluate_legal(x, moves, counts)

    rng = np.random.default_rng(7)
    games = []
    for i in range(64):
        g = O.Game()
        for _ in range(int(rng.integers(0, 24))):
            la = g.legal_actions()
            if len(la) == 0 or g.is_game_over()[0]:
                break
            g.make_action(int(la[rng.integers(len(la))]))
        games.append(types.SimpleNamespace(board=g.board.copy(), current_player=g.current_player, move_count=g.move_count,
                                           no_capture_count=g.no_capture_count, history=[bytes(h) for h in g.history()]))
    packed = mcts.MCTS(ev, num_simulations=24, seed=3)
    full = mcts.MCTS(FullWidth(ev), num_simulations=24, seed=3)
    for noise in (False, True):
        a = packed.search_many(games, 1.0, noise)
        b = full.search_many(games, 1.0, noise)
        assert packed._engine(64, noise).path == "packed" and full._engine(64, noise).path == "full"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        sp, sf = packed._engine(64, noise).stats(), full._engine(64, noise).stats()
        assert {k: v for k, v in sp.items() if k != "rows_evaluated"} == {k: v for k, v in sf.items() if k != "rows_evaluated"}


@pytest.mark.gpu
def test_live_count_follows_the_waiting_slots():
    """Case (a) stepped by hand: after every compaction n_live equals the number of slots in a WAIT phase (slot_ints[:, 3]
    in {2, 4}), the row map lists exactly those slots in order, rows_evaluated is the sum of the counts, and the count
    falls to 0 once every game is over -- where graph replays of the packed step still run and change nothing."""
    import torch
    eng, ev = _make("hip", 64, 3, 256, 8, games_target=256, max_game_length=60)
    total, seen, zero_at = 0, [], None
    for k in range(1200):
        eng.select()
        eng.compact()
        torch.cuda.synchronize()
        phase = eng.slot_ints[:, 3].cpu().numpy()
        waiting = np.flatnonzero((phase == 2) | (phase == 4))
        n = int(eng.n_live.item())
        assert n == len(waiting)
        assert (eng.packed_rows[:n].cpu().numpy() == waiting).all()
        total += n
        seen.append(n)
        ll, v = ev.evaluate_legal(eng.packed_x, eng.packed_moves, eng.packed_counts, n_live=eng.n_live)
        eng.expand_packed(ll, v)
        if n == 0:
            zero_at = k
            break
    assert zero_at is not None, "games never finished"
    st = eng.stats()
    assert st["games_finished"] == 256 and st["rows_evaluated"] == total < len(seen) * 256
    assert max(seen) == 256 and min(seen) == 0
    assert eng.capture_step(warmup=1)
    for _ in range(4):
        eng.step()
    torch.cuda.synchronize()
    assert int(eng.n_live.item()) == 0
    st2 = eng.stats()
    assert st2 == st
