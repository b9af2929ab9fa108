"""The evaluation mirror (xq_engine_init_em) on the GPU, 64x2 networks throughout.

1. the row kernel (hip.mirror_requests) bit for bit against torch (x.flip(-1), the golden permutation), n = 1, 3, 65, 130, counts
   from {0, 1, 2, 127, 128}, mixed flags, pieces on columns 0, 4 and 8; one call of 64 rows x 128 moves covers all 8100 action ids;
   rows at or past n stay untouched;
2. on 512 corpus positions the mirrored request is the mirrored board's own request: planes byte for byte, moves as a set;
3. the evaluator un-mirrors by construction: the logit of move i of the mirrored request is, as float32 bits, the logit the
   mirrored position's own request holds for flip(a_i), and the values are equal;
4. an engine with the option against a hand-driven control (an engine without it, stepped through select -> compact -> flags from
   hip.eval_mirror_bit over slot_ints, torch flip and the golden permutation -> evaluate_legal -> expand_packed): drained samples,
   results and stats byte for byte; 37 slots, 8 simulations; plain, leaves_per_step = 4 and tree reuse; eager and replayed; and at
   least one game differs from the option-off engine;
5. off is the parent: eval_mirror=False and an engine set up through xq_engine_init_rs, eager and replayed;
6. serving: MCTS(..., eval_mirror=True).search_many on 16 positions equals the same hand-driven control, twice;
7. xq_engine_compact_misses on a mirror engine is refused; the constructor refuses the cache and an evaluator without live_rows.
"""
import ctypes as C
import types

import numpy as np
import pytest

import golden_io as G
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

SEED = 11


@pytest.fixture(scope="module")
def ev():
    return _hip_evaluator(64, 2, 4.0)[1]


@pytest.fixture(scope="module")
def perm():
    import torch
    return torch.from_numpy(G.flip_perm().astype(np.int64)).cuda()


def _mirror_moves_torch(moves, counts, perm):
    """Words below the count that are action ids go through the permutation, every other word stays (int16 bits of uint16)."""
    import torch
    m = moves.to(torch.int64) & 0xFFFF
    col = torch.arange(m.shape[1], device=m.device)[None, :]
    act = (col < counts[:, None].to(torch.int64)) & (m < 8100)
    out = torch.where(act, perm[torch.where(act, m, torch.zeros_like(m))], m)
    return torch.where(out >= 32768, out - 65536, out).to(torch.int16)


def _mirror_torch(x, moves, counts, flags, perm):
    import torch
    f = flags.bool()
    xo = torch.where(f[:, None, None, None], x.flip(-1), x)
    mo = torch.where(f[:, None], _mirror_moves_torch(moves, counts, perm), moves)
    return xo, mo


# ---- 1. the row kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_row_kernel_bit_for_bit(n, perm):
    import torch
    from xiangqi_alphazero_amd import hip
    g = torch.Generator().manual_seed(100 + n)
    x = torch.randint(0, 2, (n, 15, 10, 9), generator=g).float()
    x[:, :, :, 0] = torch.randint(0, 2, (n, 15, 10), generator=g).float() * 3.0 + 1.0      # columns 0, 4 and 8 are never all alike
    x[:, :, :, 4] = 5.0 + torch.arange(10).float()[None, None, :]
    x[:, :, :, 8] = -2.0
    moves = torch.randint(0, 8100, (n, 128), generator=g)
    moves[:, 100:] = torch.randint(8100, 65536, (n, 28), generator=g)                       # words that are no action ids
    moves = torch.where(moves >= 32768, moves - 65536, moves).to(torch.int16)
    counts = torch.tensor([0, 1, 2, 127, 128], dtype=torch.int32)[torch.randint(0, 5, (n,), generator=g)]
    flags = torch.randint(0, 2, (n,), generator=g).to(torch.uint8) * torch.randint(1, 256, (n,), generator=g).to(torch.uint8)
    if n >= 3:
        flags[0], flags[1], counts[0], counts[1] = 1, 0, 128, 128
    x, moves, counts, flags = x.cuda(), moves.cuda(), counts.cuda(), flags.cuda()
    pad = 3                                                                                  # sentinel rows past n
    xo = torch.full((n + pad, 15, 10, 9), -7.5, device="cuda")
    mo = torch.full((n + pad, 128), -12345, dtype=torch.int16, device="cuda")
    got_x, got_m = hip.mirror_requests(x, moves, counts, flags, out=(xo, mo))
    want_x, want_m = _mirror_torch(x, moves, counts, flags, perm)
    assert torch.equal(got_x[:n].view(torch.int32), want_x.view(torch.int32)) and torch.equal(got_m[:n], want_m)
    assert (xo[n:] == -7.5).all() and (mo[n:] == -12345).all()
    if n >= 3:
        assert not torch.equal(got_x[0], x[0]) and torch.equal(got_x[1], x[1]) and torch.equal(got_m[1], moves[1])
    fresh_x, fresh_m = hip.mirror_requests(x, moves, counts, flags)                          # allocating form
    assert torch.equal(fresh_x, got_x[:n]) and torch.equal(fresh_m, got_m[:n])
    # twice is the identity on the action ids below the count
    back_x, back_m = hip.mirror_requests(got_x[:n].contiguous(), got_m[:n].contiguous(), counts, flags)
    assert torch.equal(back_x, x) and torch.equal(back_m, moves)


def test_row_kernel_covers_every_action_id(perm):
    import torch
    from xiangqi_alphazero_amd import hip
    ids = torch.arange(64 * 128) % 8100                                                      # 8192 words: every id at least once
    moves = torch.where(ids >= 32768, ids - 65536, ids).to(torch.int16).view(64, 128).cuda()
    x = torch.zeros((64, 15, 10, 9), device="cuda")
    counts = torch.full((64,), 128, dtype=torch.int32, device="cuda")
    _, got = hip.mirror_requests(x, moves, counts, torch.ones(64, dtype=torch.uint8, device="cuda"))
    got = (got.to(torch.int64) & 0xFFFF).view(-1)
    assert len(set(ids.tolist())) == 8100 and torch.equal(got, perm[ids.cuda()])
    assert sorted(set(got.tolist())) == list(range(8100))


# ---- 2. and 3. fixture positions ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def positions():
    """512 corpus positions that are not over, and their mirror images: boards, sides, requests of both.  Computed once, shared."""
    import torch
    from xiangqi_alphazero_amd import hip
    d = G.corpus()
    picks = [i for i in range(0, len(d["board"]), 9) if not d["done"][i]][:512]
    assert len(picks) == 512
    boards = torch.from_numpy(d["board"][picks].copy()).cuda()
    sides = torch.from_numpy(d["side"][picks].copy()).cuda()
    mboards = boards.view(-1, 10, 9).flip(-1).contiguous().view(-1, 90)
    out = {}
    for name, b in (("orig", boards), ("mirr", mboards)):
        moves, counts, _, _ = hip.movegen(b, sides)
        out[name] = (hip.encode(b, sides), moves, counts.to(torch.int32))
    return out


def test_mirrored_request_is_the_mirrored_boards_request(positions, perm):
    import torch
    from xiangqi_alphazero_amd import hip
    x, moves, counts = positions["orig"]
    mx, mmoves, mcounts = positions["mirr"]
    ones = torch.ones(len(x), dtype=torch.uint8, device="cuda")
    got_x, got_m = hip.mirror_requests(x, moves, counts, ones)
    assert torch.equal(got_x.view(torch.int32), mx.view(torch.int32))                        # planes byte for byte
    assert torch.equal(counts, mcounts) and int(counts.min()) > 0
    a, b, c = (got_m.cpu().numpy().view(np.uint16), mmoves.cpu().numpy().view(np.uint16), counts.cpu().numpy())
    same_order = 0
    for i in range(len(c)):
        assert sorted(a[i, :c[i]].tolist()) == sorted(b[i, :c[i]].tolist()), i               # the same moves as a set
        same_order += a[i, :c[i]].tolist() == b[i, :c[i]].tolist()
    assert same_order < len(c)                                                              # not in the same order: mirrored in place
    zeros = torch.zeros(len(x), dtype=torch.uint8, device="cuda")
    cp_x, cp_m = hip.mirror_requests(x, moves, counts, zeros)
    assert torch.equal(cp_x, x) and torch.equal(cp_m, moves)


def test_evaluator_unmirrors_by_construction(positions, ev):
    import torch
    from xiangqi_alphazero_amd import hip
    x, moves, counts = positions["orig"]
    mx, mmoves, mcounts = positions["mirr"]
    ones = torch.ones(len(x), dtype=torch.uint8, device="cuda")
    got_x, got_m = hip.mirror_requests(x, moves, counts, ones)
    ll, v = (t.clone() for t in ev.evaluate_legal(got_x, got_m, counts))
    own_ll, own_v = (t.clone() for t in ev.evaluate_legal(mx, mmoves, mcounts))
    assert torch.equal(v.view(torch.int32), own_v.view(torch.int32))
    a, b, c = got_m.cpu().numpy().view(np.uint16), mmoves.cpu().numpy().view(np.uint16), counts.cpu().numpy()
    ll, own_ll = ll.cpu().numpy().view(np.uint32), own_ll.cpu().numpy().view(np.uint32)
    for i in range(len(c)):
        where = {int(m): k for k, m in enumerate(b[i, :c[i]])}
        idx = [where[int(m)] for m in a[i, :c[i]]]                                           # where flip(a_i) sits in the own list
        assert (ll[i, :c[i]] == own_ll[i, idx]).all(), i
    plain_ll, plain_v = ev.evaluate_legal(x, moves, counts)
    assert not torch.equal(plain_v, v)                                                       # the network is not symmetric


# ---- 4. the engine against a hand-driven control ----------------------------------------------------------------------------------
def _flags_of(eng, n, rows, gi):
    """The bits of the packed rows [0, n) of a stepped engine, on the host, from its state words after select."""
    from xiangqi_alphazero_amd import hip
    cfg, K = eng.cfg, eng.K
    flags = np.zeros(len(eng.packed_rows), dtype=np.uint8)
    for r in range(n):
        slot, j = divmod(int(rows[r]), K)
        root = int(gi[slot, hip.GI_PHASE]) == 2                                              # PH_WAIT_ROOT
        flags[r] = hip.eval_mirror_bit(int(cfg.seed), int(cfg.rank), slot, int(gi[slot, hip.GI_GSEQ]) & 0xFFFFFFFF,
                                       int(gi[slot, hip.GI_MC]), root, 0 if root else int(gi[slot, hip.GI_SIMS]), j)
    return flags


def _hand_step(eng, ev, perm, seen):
    """One step of the control: the engine's own select, compact and expand_packed; the mirroring by torch on the host's flags."""
    import torch
    eng.select()
    eng.compact()
    torch.cuda.synchronize()
    n = int(eng.n_live.item())
    flags = _flags_of(eng, n, eng.packed_rows.cpu().numpy(), eng.slot_ints.cpu().numpy())
    seen[0] += n
    seen[1] += int(flags.sum())
    x, m = _mirror_torch(eng.packed_x, eng.packed_moves, eng.packed_counts, torch.from_numpy(flags).cuda(), perm)
    ll, v = ev.evaluate_legal(x.contiguous(), m.contiguous(), eng.packed_counts, n_live=eng.n_live)
    eng.expand_packed(ll, v)
    eng.steps += 1


def _play(eng, n_games, step):
    while True:
        step()
        if eng.steps % 16 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 4000, "games did not finish"
    st = eng.stats()
    assert st["overflow"] == 0
    smp, res = eng.drain()
    return (np.sort(smp, order=["slot", "game_seq", "ply"]).tobytes(), np.sort(res, order=["slot", "game_seq"]).tobytes(), st)


ENGINE_CASES = [("plain", {}), ("leaves4", dict(leaves_per_step=4)), ("tree_reuse", dict(tree_reuse=True))]


@pytest.mark.parametrize("name,kw", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_equals_hand_driven_control(name, kw, ev, perm):
    from xiangqi_alphazero_amd import engine
    n = 37
    cfg = engine.make_config(n, 8, seed=SEED, games_target=n, max_game_length=40)
    control = engine.SelfPlayEngine(cfg, evaluator=ev, **kw)
    assert not control.eval_mirror and control.h.pad0 >= 0
    seen = [0, 0]
    want = _play(control, n, lambda: _hand_step(control, ev, perm, seen))
    print(name, "rows", seen[0], "mirrored", seen[1])
    assert 0.4 * seen[0] < seen[1] < 0.6 * seen[0]                                          # about half of the requests
    got = {}
    for graph in (False, True):
        a = engine.SelfPlayEngine(cfg, evaluator=ev, eval_mirror=True, **kw)
        assert a.eval_mirror and a.path == "packed" and a.h.pad0 < 0 and a.workspace_bytes == control.workspace_bytes
        if graph:
            assert a.capture_step() and a.launch_mode == "graph"
        got[graph] = _play(a, n, a.step)
        assert got[graph][0] == want[0] and got[graph][1] == want[1], (name, graph)
        assert got[graph][2] == want[2], (name, graph)
    off = engine.SelfPlayEngine(cfg, evaluator=ev, **kw)
    plain = _play(off, n, off.step)
    assert plain[1] != want[1] or plain[0] != want[0]                                       # the bits are not all zero


# ---- 5. off is the parent ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4], ids=["sequential", "leaves4"])
def test_off_is_the_engine_of_init_rs(K, ev):
    import torch
    from xiangqi_alphazero_amd import engine, hip
    n = 8
    cfg = engine.make_config(n, 8, seed=SEED, games_target=n, max_game_length=30)
    for graph in (False, True):
        out = []
        for through_rs in (True, False):
            eng = engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=K, eval_mirror=False)
            assert not eng.eval_mirror
            if through_rs:
                before = bytes(eng.h)
                base = (eng.ws.data_ptr() + 255) & ~255
                hip.check(eng.lib.xq_engine_init_rs(C.byref(eng.h), C.byref(cfg), K, 0, None, None, None, None, None, None, None, base,
                                                    eng.workspace_bytes, None, hip.stream_ptr(eng.device)), "xq_engine_init_rs")
                torch.cuda.synchronize()
                assert bytes(eng.h) == before                                               # the same handle
            if graph:
                assert eng.capture_step()
            out.append(_play(eng, n, eng.step))
        assert out[0] == out[1]


# ---- 6. serving ---------------------------------------------------------------------------------------------------------------------
def test_mcts_serving_equals_control_and_repeats(ev, perm):
    import torch
    from xiangqi_alphazero_amd import engine, mcts
    from xiangqi_alphazero_amd.sample_format import dense_pi
    d = G.corpus()
    picks = [i for i in range(5, len(d["board"]), 70) if not d["done"][i]][:16]
    games = [types.SimpleNamespace(board=d["board"][i].reshape(10, 9), current_player=int(d["side"][i]), move_count=int(d["move_count"][i]),
                                   no_capture_count=int(d["no_capture"][i]), history=[h.tobytes() for h in G.history_tail(d, i)])
             for i in picks]
    sims = 24
    m = mcts.MCTS(ev, sims, seed=3, eval_mirror=True)
    first, v1 = m.search_many(games, add_noise=False, return_values=True)
    assert m._engine(16, False).eval_mirror
    second, v2 = m.search_many(games, add_noise=False, return_values=True)
    assert all((a == b).all() for a, b in zip(first, second)) and v1.tobytes() == v2.tobytes()
    cfg = engine.make_config(16, sims, c_puct=1.5, add_noise=False, manual_moves=1, seed=3)
    control = engine.SelfPlayEngine(cfg, evaluator=ev)
    for slot, g in enumerate(games):
        hist = [np.frombuffer(h, dtype=np.int8) for h in g.history]
        control.set_position(slot, np.asarray(g.board, dtype=np.int8), g.current_player, g.move_count, g.no_capture_count,
                             np.stack(hist) if hist else None)
    seen = [0, 0]
    while not control.held():
        _hand_step(control, ev, perm, seen)
        assert control.steps < 8 * sims
    assert 0 < seen[1] < seen[0]
    for slot in range(16):
        r = control.read_root(slot)
        assert (dense_pi(r["actions"], r["visits"].astype(np.float64), 1.0) == first[slot]).all(), slot
        assert mcts.root_value(r["visits"], r["total_value"]) == v1[slot]
    plain = mcts.MCTS(ev, sims, seed=3).search_many(games, add_noise=False)
    assert any((a != b).any() for a, b in zip(first, plain))


# ---- 7. refusals that need a device ------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(ev):
    from xiangqi_alphazero_amd import engine, hip
    cfg = engine.make_config(4, 8, seed=1)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, eval_mirror=True)
    eng.select()
    import torch
    no_hit = torch.zeros(4, dtype=torch.int32, device="cuda")
    sp = hip.stream_ptr(eng.device)
    assert eng.lib.xq_engine_compact_misses(C.byref(eng.h), eng.nn_input.data_ptr(), no_hit.data_ptr(), sp) == -1
    off = engine.SelfPlayEngine(cfg, evaluator=ev)
    off.select()
    assert off.lib.xq_engine_compact_misses(C.byref(off.h), off.nn_input.data_ptr(), no_hit.data_ptr(), sp) == 0   # the call itself is fine
    torch.cuda.synchronize()
    with pytest.raises(hip.XqError, match="eval_mirror"):
        engine.SelfPlayEngine(cfg, evaluator=ev, eval_mirror=True, eval_cache_entries=64)
    with pytest.raises(hip.XqError, match="live_rows"):
        engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), eval_mirror=True)
    eng.evaluator = _TorchStub()                                                             # swapped afterwards: the step refuses too
    with pytest.raises(hip.XqError, match="eval_mirror"):
        eng.step()
