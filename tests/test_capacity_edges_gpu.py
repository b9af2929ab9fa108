"""The engine's capacity edges on the GPU: what the suite's other engine tests step around by asserting overflow == 0 and
samples_dropped == 0.

1. Sample and result rings at capacity: a drain hands out only rows written since the last drain, whole games, each equal to the
   row an engine with roomy rings produced for the same (slot, game_seq, ply); samples_written counts exactly the rows handed out.
2. Move lists past XQ_MAXM = 128: a truncated list is the head of the true list, flagged, and the waves beside it in the
   workgroup (the kernels carve LDS per wave, no barrier) are untouched.
3. An engine slot in overflow does not disturb the slots beside it in the tree arenas.
4. Injected draws running out: flagged (overflow bit 2), every missing draw reads as 0, the engine keeps stepping.

Every scenario stays inside clamped, documented behaviour; none uses a fault as its signal.  The crafted boards and their move
counts are tests/capacity_boards.py, refereed on the CPU in tests/test_capacity_edges.py.
"""
import ctypes as C

import numpy as np
import pytest

import capacity_boards as CB
import golden_io as G
from oracle import xq_oracle as O
from stub_eval import StubEvaluator, predict_from_key, state_key

pytestmark = pytest.mark.gpu

POISON = 0xEE          # no record holds it: as a board byte it is piece -18, as a slot 0xEEEEEEEE, as a winner -18


@pytest.fixture(scope="module")
def mods():
    import torch
    from xiangqi_alphazero_amd import engine, hip
    hip.lib()
    assert torch.cuda.is_available()
    return engine, hip


# ---- 1. rings at capacity ---------------------------------------------------------------------------------------------

RING_STEPS, RING_SAMPLES, RING_RESULTS = 300, 100, 8


def _ring_engine(engine, net, **rings):
    from xiangqi_alphazero_amd import evaluator
    ev, _ = evaluator.make_evaluator(net, "cuda", "hip")
    cfg = engine.make_config(96, 4, max_game_length=20, random_opening_moves=4, temperature_threshold=8, seed=21, **rings)
    return engine.SelfPlayEngine(cfg, "cuda", evaluator=ev)


@pytest.fixture(scope="module")
def ring_reference(mods):
    """300 eager steps with the default rings (nothing dropped), one drain: every sample by (slot, game_seq, ply), every result
    by (slot, game_seq).  Computed once, read-only."""
    engine, _ = mods
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(64, 3)
    net.load_state_dict(weights.make_state_dict(64, 3, policy_gain=4.0))
    eng = _ring_engine(engine, net)
    for _ in range(RING_STEPS):
        eng.step()
    st = eng.stats()
    smp, res = eng.drain()
    assert st["overflow"] == 0 and st["samples_dropped"] == 0 and len(smp) == st["samples_written"]
    assert len(res) == st["games_finished"] > 20
    samples = {(int(s["slot"]), int(s["game_seq"]), int(s["ply"])): s.tobytes() for s in smp}
    results = {(int(r["slot"]), int(r["game_seq"])): r.tobytes() for r in res}
    assert len(samples) == len(smp) and len(results) == len(res)
    n_samples = {k: int(r["n_samples"]) for k, r in zip(((int(r["slot"]), int(r["game_seq"])) for r in res), res)}
    assert max(n_samples.values()) <= 20 and sum(n_samples.values()) == len(smp)
    return dict(net=net, stats=st, samples=samples, results=results, n_samples=n_samples)


def _fill(eng, hip, idx, nbytes, byte):
    off = int(eng.h.p[idx]) - int(eng.ws.data_ptr())
    eng.ws[off:off + nbytes].fill_(byte)


def _poison_rings(eng, hip):
    _fill(eng, hip, hip.P_OUTS, eng.cfg.max_out_samples * hip.SAMPLE_BYTES, POISON)
    _fill(eng, hip, hip.P_OUTR, eng.cfg.max_out_results * hip.RESULT_BYTES, POISON)


def _pending(eng, hip):
    """xq_engine_drain_device's size query (both buffers NULL): the pending sizes; consumes nothing."""
    ns, nr = C.c_int(-1), C.c_int(-1)
    rc = eng.lib.xq_engine_drain_device(C.byref(eng.h), None, 0, C.byref(ns), None, 0, C.byref(nr), hip.stream_ptr(eng.device))
    assert rc == 0
    return ns.value, nr.value


def _drain(eng, hip, mode):
    from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE, SAMPLE_DTYPE
    if mode == "host":
        return eng.drain()
    smp, res = eng.drain_device()
    assert smp.is_cuda and res.is_cuda
    return (smp.cpu().numpy().reshape(-1).view(SAMPLE_DTYPE).copy(), res.cpu().numpy().reshape(-1).view(RESULT_DTYPE).copy())


def _short_drain_consumes_nothing(eng, hip):
    """The raw ABI with a sample buffer one row too small: XQ_ERR_ARG, the pending sizes reported, nothing consumed."""
    from xiangqi_alphazero_amd.sample_format import RESULT_DTYPE, SAMPLE_DTYPE
    ns, nr = _pending(eng, hip)
    assert ns > 0 and nr > 0
    assert _pending(eng, hip) == (ns, nr)                             # the size query itself consumed nothing
    smp = np.full(ns, POISON, dtype=np.uint8).repeat(hip.SAMPLE_BYTES).view(SAMPLE_DTYPE)
    res = np.full(nr, POISON, dtype=np.uint8).repeat(hip.RESULT_BYTES).view(RESULT_DTYPE)
    gs, gr = C.c_int(-1), C.c_int(-1)
    rc = eng.lib.xq_engine_drain(C.byref(eng.h), smp.ctypes.data, ns - 1, C.byref(gs), res.ctypes.data, nr, C.byref(gr),
                                 hip.stream_ptr(eng.device))
    assert rc == -1 and (gs.value, gr.value) == (ns, nr)               # XQ_ERR_ARG
    assert (smp.view(np.uint8) == POISON).all() and (res.view(np.uint8) == POISON).all()     # and nothing was copied
    assert _pending(eng, hip) == (ns, nr)
    return ns, nr


@pytest.mark.parametrize("mode", ["host", "device"])
def test_full_rings_hand_out_only_whole_fresh_games(mods, ring_reference, mode):
    """max_out_samples = 100 and max_out_results = 8 where 300 steps finish some 290 games of up to 20 samples: the rings are
    full long before each drain.  Which games find room depends on the order workgroups reach the cursor, so everything is
    compared by key against the roomy run of the same seed, never by position.
    Before the cursor moved only for a game that fits (compare-and-swap), a rejected game had already pushed it past the
    capacity and the drains returned min(cursor, 100) rows: the rows behind the last accepted game came back as they lay in
    the ring, here the poison bytes, in production the samples of games drained earlier."""
    import torch
    engine, hip = mods
    ref = ring_reference
    eng = _ring_engine(engine, ref["net"], max_out_samples=RING_SAMPLES, max_out_results=RING_RESULTS)
    assert eng.cfg.max_out_samples == RING_SAMPLES and eng.cfg.max_out_results == RING_RESULTS
    _poison_rings(eng, hip)
    seen_samples, seen_results, rows_total = set(), set(), 0
    finished_before, gseq_before = 0, None
    drains = []
    for part in range(2):
        for _ in range(RING_STEPS // 2):
            eng.step()
        st = eng.stats()
        assert st["overflow"] == 0                                  # a full ring is not a capacity error
        assert st["samples_dropped"] > 0                            # ... and it is full: the test cannot pass vacuously
        gseq = eng.slot_ints[:, hip.GI_GSEQ].cpu().numpy().copy()
        if part == 0:
            pend = _short_drain_consumes_nothing(eng, hip)
        smp, res = _drain(eng, hip, mode)
        if part == 0:
            assert (len(smp), len(res)) == pend                       # the full-size drain after it returns exactly those
        assert _pending(eng, hip) == (0, 0)
        print(f"{mode} drain {part}: {len(smp)} rows, {len(res)} results, written {st['samples_written']}, "
              f"dropped {st['samples_dropped']}, finished {st['games_finished']}")
        # -- samples: fresh, equal to the roomy run's, whole games, none twice
        assert 0 < len(smp) <= RING_SAMPLES
        raw = smp.view(np.uint8).reshape(len(smp), hip.SAMPLE_BYTES)
        assert not (raw == POISON).all(axis=1).any(), "a row the engine never wrote came back"
        per_game = {}
        for s in smp:
            key = (int(s["slot"]), int(s["game_seq"]), int(s["ply"]))
            assert key in ref["samples"], key
            assert s.tobytes() == ref["samples"][key], key
            assert key not in seen_samples, key
            seen_samples.add(key)
            per_game[key[:2]] = per_game.get(key[:2], 0) + 1
            # flushed since the last drain: a flush is followed by the slot's next game in the same launch
            assert int(s["game_seq"]) <= int(gseq[key[0]]) - 1
            if gseq_before is not None:
                assert int(s["game_seq"]) >= int(gseq_before[key[0]]), "a row of an earlier drain came back"
        for gk, n in per_game.items():
            assert n == ref["n_samples"][gk], gk                    # wholly present
        rows_total += len(smp)
        assert rows_total == st["samples_written"]
        # -- results: the first min(finished since the last drain, 8), each the roomy run's record
        assert len(res) == min(st["games_finished"] - finished_before, RING_RESULTS)
        for r in res:
            key = (int(r["slot"]), int(r["game_seq"]))
            assert r.tobytes() == ref["results"][key], key
            assert key not in seen_results, key
            seen_results.add(key)
            if gseq_before is not None:
                assert key[1] >= int(gseq_before[key[0]])
        finished_before, gseq_before = st["games_finished"], gseq
        drains.append(per_game)
        _poison_rings(eng, hip)
        torch.cuda.synchronize()
    assert drains[1] and not set(drains[0]) & set(drains[1])          # the second drain holds games of its own
    st = eng.stats()
    for k in ("games_finished", "sims", "moves_played", "games_started", "plies_finished"):
        assert st[k] == ref["stats"][k], k                          # the games themselves are unchanged
    assert st["samples_written"] + st["samples_dropped"] == sum(ref["n_samples"].values())
    assert st["samples_written"] == rows_total and st["overflow"] == 0


# ---- 2. move lists past XQ_MAXM ---------------------------------------------------------------------------------------

SENTINEL = 0xA5


def _edge_batch():
    """99 positions = 24 workgroups of four and one of three: edge board b (six of them) stands at wave position w of workgroup
    4 b + w, among three corpus positions; the last, partial workgroup is corpus positions only."""
    d = G.corpus()
    n = 4 * 6 * 4 + 3
    n_plain = n - 4 * len(CB.ALL_COUNTS)
    over = [int(j) for j in np.nonzero(d["done"])[0][::4][:8]]          # eight finished games' last positions among them
    plain = list(range(7, len(d["board"]), 41))[:n_plain - len(over)] + over
    assert len(plain) == n_plain and len(over) == 8
    pool = iter(plain[(k * 37) % n_plain] for k in range(n_plain))      # 37 and 75 are coprime: a fixed shuffle
    boards = np.zeros((n, 90), dtype=np.int8)
    side = np.zeros(n, dtype=np.int8)
    mc = np.zeros(n, dtype=np.int32)
    nocap = np.zeros(n, dtype=np.int32)
    hist = np.zeros((n, 12, 90), dtype=np.int8)
    src = np.full(n, -1, dtype=np.int64)           # corpus index, or -1 for an edge board
    want = [None] * n                               # edge boards: their move count
    for b, count in enumerate(CB.ALL_COUNTS):
        for w in range(4):
            i = 4 * (4 * b + w) + w
            boards[i], side[i], want[i] = CB.edge_board(count).reshape(90), 1, count
    for i in range(n):
        if want[i] is None:
            j = next(pool)
            src[i] = j
            boards[i], side[i], mc[i], nocap[i] = d["board"][j], d["side"][j], d["move_count"][j], d["no_capture"][j]
            h = G.history_tail(d, j)
            hist[i, :len(h)] = h
    for g in range(24):                             # every edge board shares its workgroup with three ordinary positions
        assert sorted(x is None for x in want[4 * g:4 * g + 4]) == [False, True, True, True]
    assert n % 4 != 0 and {i % 4 for i in range(n) if want[i] == 152} == {0, 1, 2, 3}
    return dict(n=n, boards=boards, side=side, mc=mc, nocap=nocap, hist=hist, src=src, want=want, corpus=d)


def test_movegen_truncates_at_128_and_leaves_its_neighbours_alone(mods):
    """xq_movegen_batch over edge boards with 121 .. 152 legal moves, each beside three ordinary positions of its workgroup, in
    every wave position.  Would catch: a truncated list that is not the head of the true one, a miscounted or unflagged
    truncation (127 / 128 / 129 sit on both sides of the comparison), a write past a row's count, and an LDS overrun into the
    neighbouring wave's board, candidates or output row, which would change a neighbour's list, count or check flag."""
    import torch
    _, hip = mods
    t = _edge_batch()
    n = t["n"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    boards, side = dev(t["boards"]), dev(t["side"])
    moves = torch.full((n + 1, hip.MAXM), -1, dtype=torch.int16, device="cuda")          # 0xFFFF; one guard row behind the batch
    counts = torch.full((n + 1,), -1, dtype=torch.int16, device="cuda")
    chk = torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
    hip.check(hip.lib().xq_movegen_batch(boards.data_ptr(), side.data_ptr(), n, moves.data_ptr(), counts.data_ptr(),
                                         chk.data_ptr(), status.data_ptr(), hip.stream_ptr()), "xq_movegen_batch")
    mv = moves.cpu().numpy().view(np.uint16)
    ct = counts.cpu().numpy().view(np.uint16)
    ck, stt = chk.cpu().numpy(), status.cpu().numpy()
    assert (mv[n] == 0xFFFF).all() and ct[n] == 0xFFFF and ck[n] == SENTINEL and stt[n] == SENTINEL   # nothing behind the batch
    for i in range(n):
        full = O.legal_actions(t["boards"][i], int(t["side"][i]))
        tag = (i, t["want"][i])
        if t["want"][i] is not None:
            assert len(full) == t["want"][i], tag
        over = len(full) > CB.MAXM
        assert t["want"][i] is not None or not over
        assert int(stt[i]) == (1 if over else 0), tag
        assert int(ct[i]) == min(len(full), CB.MAXM), tag
        np.testing.assert_array_equal(mv[i, :ct[i]], full[:CB.MAXM], err_msg=str(tag))      # the head of the true list
        assert (mv[i, ct[i]:] == 0xFFFF).all(), tag                                         # nothing written past the count
        assert int(ck[i]) == int(O.is_in_check(t["boards"][i], int(t["side"][i]))), tag
    assert sorted(int(c) for c, w in zip(ct[:n], t["want"]) if w is not None) == sorted(min(c, 128) for c in CB.ALL_COUNTS * 4)
    # the same batch through xq_game_over_batch (it generates the moves too): edge boards not over, the others as recorded
    out = hip.game_over(boards, side, dev(t["mc"]), dev(t["nocap"]), dev(t["hist"])).cpu().numpy()
    d = t["corpus"]
    for i in range(n):
        if t["want"][i] is not None:
            assert out[i, 0] == 0, i
        else:
            assert (int(out[i, 0]), int(out[i, 1])) == (int(d["done"][t["src"][i]]), int(d["winner"][t["src"][i]])), i


# ---- 3. an engine slot in overflow ------------------------------------------------------------------------------------

def _stub_steps(eng, n_steps, peaked=True):
    import torch
    cache = {}
    for _ in range(n_steps):
        x = eng.select().cpu().numpy()
        probs = np.empty((x.shape[0], 8100), dtype=np.float32)
        vals = np.empty(x.shape[0], dtype=np.float32)
        for i in range(x.shape[0]):
            key = state_key(x[i])
            if key not in cache:
                cache[key] = predict_from_key(key, peaked)
            probs[i], vals[i] = cache[key]
        eng.expand(torch.from_numpy(probs).cuda(), torch.from_numpy(vals).cuda(), is_probs=True)


def _corpus_games(count):
    d = G.corpus()
    games = []
    for i in [i for i in range(5, len(d["board"]), 70) if not d["done"][i]][:count]:
        g = O.Game()
        for a in d["taken"][i - d["ply"][i]:i]:
            g.make_action(int(a))
        np.testing.assert_array_equal(g.board.reshape(90), d["board"][i])
        games.append(g)
    return games


def _set_game(eng, slot, g):
    eng.set_position(slot, g.board, g.current_player, g.move_count, g.no_capture_count, g.history()[-12:])


def _assert_roots_equal(a, b, tag):
    assert list(a["actions"]) == list(b["actions"]), tag
    assert list(a["visits"]) == list(b["visits"]), tag
    assert a["total_value"].tobytes() == b["total_value"].tobytes(), tag
    assert a["prior"].tobytes() == b["prior"].tobytes() and a["prior_kind"] == b["prior_kind"], tag
    assert (a["root_visits"], a["sims_done"]) == (b["root_visits"], b["sims_done"]), tag


def _assert_root_is_oracle(r, g, sims, tag):
    want = O.mcts_search(g, sims, StubEvaluator(peaked=True).predict)
    n = want.n_children
    assert list(r["actions"]) == list(want.actions[:n]), tag
    assert list(r["visits"]) == list(want.visits[:n]), tag
    np.testing.assert_array_equal(r["total_value"], np.array(want.total_value[:n]), err_msg=str(tag))
    assert r["sims_done"] == sims, tag


def test_engine_slot_in_overflow_does_not_disturb_its_neighbours(mods):
    """Search-only engine, 64 simulations: slots 1, 3, 5 hold the 139-, 152- and 128-move boards, slots 0, 2, 4, 6 ordinary
    positions.  The overflow is reported (bit 1 << 8, code -4 from a checked read), the truncated roots are the head of the
    true move list, and the even slots' searches are, bit for bit, those of an engine that holds only them, and the oracle's:
    an arena write of a slot in overflow that left its own [node_cap] range would show there."""
    engine, hip = mods
    sims = 64
    games = _corpus_games(4)
    edge = {1: 139, 3: 152, 5: 128}
    eng = engine.SelfPlayEngine(engine.make_config(7, sims, add_noise=False, manual_moves=True))
    for k, g in enumerate(games):
        _set_game(eng, 2 * k, g)
    for slot, count in edge.items():
        eng.set_position(slot, CB.edge_board(count), 1)
    _stub_steps(eng, sims + 1)
    st = eng.stats(check=False)
    assert st["overflow"] & (1 << 8), hex(st["overflow"])
    assert st["overflow"] == 1 << 8, hex(st["overflow"])            # the move list, and no other capacity
    with pytest.raises(hip.XqError, match="code -4"):
        eng.stats()
    alone = engine.SelfPlayEngine(engine.make_config(4, sims, add_noise=False, manual_moves=True))
    for k, g in enumerate(games):
        _set_game(alone, k, g)
    _stub_steps(alone, sims + 1)
    assert alone.stats()["overflow"] == 0
    for k, g in enumerate(games):
        r = eng.read_root(2 * k)
        _assert_roots_equal(r, alone.read_root(k), k)
        _assert_root_is_oracle(r, g, sims, k)
    for slot, count in edge.items():
        r = eng.read_root(slot)
        full = O.legal_actions(CB.edge_board(count), 1)
        assert len(full) == count
        assert list(r["actions"]) == list(full[:CB.MAXM]), slot
        assert r["sims_done"] == sims and int(np.sum(r["visits"])) == sims, slot


def test_128_move_root_is_no_overflow(mods):
    """Exactly XQ_MAXM legal moves is inside the capacity: overflow stays 0 and the search is the oracle's
    (tests/test_capacity_edges.py shows that this search meets no longer list further down)."""
    engine, _ = mods
    sims = 64
    eng = engine.SelfPlayEngine(engine.make_config(1, sims, add_noise=False, manual_moves=True))
    eng.set_position(0, CB.edge_board(128), 1)
    _stub_steps(eng, sims + 1)
    assert eng.stats()["overflow"] == 0
    g = O.Game()
    g.set_board(CB.edge_board(128), 1)
    r = eng.read_root(0)
    assert len(r["actions"]) == 128
    _assert_root_is_oracle(r, g, sims, 128)


# ---- 4. injected draws running out ------------------------------------------------------------------------------------

def test_injected_draws_running_out_is_flagged_and_reads_as_zero(mods):
    """Self-play from injected draws with inject_len = 8: the first noisy root alone needs 44 Dirichlet draws, so the streams
    run out at once.  The engine flags it (overflow bit 2), takes 0 for every missing draw (there is no rejection loop on the
    injected path: a zero draw is the Dirichlet weight 1) and keeps stepping; an engine given the same eight draws followed by
    explicit zeros, 16384 in all, never runs out and must play the same game."""
    engine, hip = mods
    from draws import Stream
    S, n_slots, steps = 4, 2, 40
    short = np.zeros((n_slots, 4, 8), dtype=np.uint64)
    for kind in range(4):
        s = Stream(5, kind + 1)
        short[:, kind, :] = np.array([s.next_u64() for _ in range(8)], dtype=np.uint64)[None, :]
    long_ = np.zeros((n_slots, 4, 16384), dtype=np.uint64)
    long_[:, :, :8] = short
    engs = []
    for inj in (short, long_):
        cfg = engine.make_config(n_slots, S, add_noise=True, inject_len=inj.shape[2], seed=3)
        engs.append(engine.SelfPlayEngine(cfg, inject=inj))
    e8, e16k = engs
    for e in engs:
        _stub_steps(e, 1 + S, peaked=False)                            # the root's evaluation and the first move's S simulations
    for slot in range(n_slots):
        r8, r16k = e8.read_root(slot), e16k.read_root(slot)
        assert r8["sims_done"] == S and r8["prior_kind"] == 1 and len(r8["actions"]) > 8
        _assert_roots_equal(r8, r16k, slot)
    assert e8.stats(check=False)["overflow"] == 2                      # bit 2, nothing else
    assert e16k.stats()["overflow"] == 0
    sims = [e8.stats(check=False)["sims"]]
    assert sims[0] == n_slots * S
    for _ in range(steps - 1 - S):
        _stub_steps(e8, 1, peaked=False)
        sims.append(e8.stats(check=False)["sims"])
    # a slot's step is a simulation, or the one root evaluation between two moves: over two steps the count always grows
    assert all(b >= a for a, b in zip(sims, sims[1:])) and all(sims[i + 2] > sims[i] for i in range(len(sims) - 2)), sims
    _stub_steps(e16k, steps - 1 - S, peaked=False)
    s8, s16k = e8.stats(check=False), e16k.stats()
    assert s8["overflow"] == 2 and s16k["overflow"] == 0
    for k in ("sims", "moves_played", "root_evals", "leaf_evals", "nodes_created", "games_started"):
        assert s8[k] == s16k[k], k
    assert s8["moves_played"] >= n_slots * 6
    with pytest.raises(hip.XqError, match="code -4"):
        e8.stats()
