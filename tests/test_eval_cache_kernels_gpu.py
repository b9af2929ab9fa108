"""The evaluation cache's kernels (csrc/xq_evcache.hip: k_evcache_probe with wave_evkey, k_compact_misses, k_evcache_commit,
k_evcache_invalidate) held to the host twin of tests/eval_cache_model.py probe by probe: hit flags, the bits of every row handed
back, the packed misses and the five counters.  The first three tests drive the C entry points directly on slots that wait for
an evaluation nobody delivers, with planes and evaluated rows of the test's own; the last watches the cached step of a real
self-play engine.  Every comparison is exact.  tests/test_eval_cache_model.py shows what the streams used here can tell apart."""
import ctypes as C
import os

import numpy as np
import pytest

import eval_cache_model as M

pytestmark = pytest.mark.gpu

PH_WAIT_ROOT = 2                                          # enum Phase of csrc/xq_engine_state.cuh
SENT_LOGIT, SENT_VALUE = 0x7FA5A5A5, 0x7FB6B6B6           # int32 patterns no step's rows hold
SPECIALS = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x00000001, 0x807FFFFF, 0x00000000], np.uint32)
#                    -0.0        +inf        -inf        quiet NaN + payload, signalling NaN, two denormals, +0.0


def _bits(tag: int, n: int):
    """The evaluated rows of step `tag` as bit patterns: int32 [n, 128] logits and int32 [n] values, random bits with the
    special values sprinkled in, so that a copy through the table is shown to be bitwise and a row names the step it is from."""
    rng = np.random.default_rng([77, tag])
    rows = rng.integers(0, 2 ** 32, (n, M.MAXM), dtype=np.uint64).astype(np.uint32)
    rows[np.arange(n)[:, None], rng.integers(0, M.MAXM, (n, len(SPECIALS)))] = SPECIALS[None, :]
    vals = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    vals[::3] = SPECIALS[(np.arange(len(vals[::3])) + tag) % len(SPECIALS)]
    return rows.view(np.int32), vals.view(np.int32)


class _NeverCalled:
    live_rows = True                                      # what the engine asks of a cached step's evaluator


class Rig:
    """A search-only engine with an evaluation cache whose `waiting` slots sit in PH_WAIT_ROOT for good, the entry points of one
    cached step minus the evaluator and the expansion, and the model fed the same probes and commits."""

    def __init__(self, n_slots: int, entries: int, positions: dict):
        import torch
        from xiangqi_alphazero_amd import engine, hip
        self.torch, self.hip = torch, hip
        self.G, self.K = n_slots, entries
        cfg = engine.make_config(n_slots, 4, add_noise=False, manual_moves=True)
        self.eng = e = engine.SelfPlayEngine(cfg, "cuda", evaluator=_NeverCalled(), eval_cache_entries=entries)
        assert (e.cache.ways, e.cache.sets) == M.geometry(entries)
        off = e._cache_hit_ptr - e.cache_ws.data_ptr()
        self.hit = e.cache_ws[off:off + 4 * n_slots].view(torch.int32)
        self.rows = torch.zeros((n_slots, M.MAXM), dtype=torch.int32, device="cuda")
        self.values = torch.zeros(n_slots, dtype=torch.int32, device="cuda")
        self.model = M.EvCacheModel(n_slots, entries)
        self.waiting = []
        self.set_positions(positions)

    def set_positions(self, positions: dict):
        e = self.eng
        for slot, (board, side) in positions.items():
            e.set_position(slot, board, int(side))
        e.select()
        self.torch.cuda.synchronize()
        self.waiting = sorted(set(self.waiting) | set(positions))
        self.idle = [s for s in range(self.G) if s not in self.waiting]
        self.counts = e.req_counts.cpu().numpy().copy()
        phase = e.slot_ints[:, self.hip.GI_PHASE].cpu().numpy()
        assert (phase[self.waiting] == PH_WAIT_ROOT).all() and (phase[self.idle] == self.hip.PH_HOLD).all()
        assert (self.counts[self.waiting] > 0).all() and (self.counts[self.idle] == 0).all()

    def invalidate(self):
        e = self.eng
        self.hip.check(e.lib.xq_evcache_invalidate(C.byref(e.cache), self.hip.stream_ptr(e.device)), "xq_evcache_invalidate")
        self.model.invalidate()

    def stats(self) -> dict:
        e = self.eng
        cs = self.hip.EvCacheStats()
        self.hip.check(e.lib.xq_evcache_stats_read(C.byref(e.cache), C.byref(cs), self.hip.stream_ptr(e.device)), "stats_read")
        return cs.as_dict()

    def step(self, planes, keys, *commits):
        """One step: probe `planes` (device float32 [G, 15, 10, 9]; `keys[slot]` is the model's key of a waiting slot's planes),
        compact the misses, commit `commits` = (rows int32 [G, 128], values int32 [G]) indexed by SLOT, one after the other.
        Asserts everything the kernels leave behind against the model; returns (flags, slot_logits bits, slot_value bits)."""
        torch, hip, e = self.torch, self.hip, self.eng
        lib, sp = e.lib, hip.stream_ptr(e.device)
        assert planes.is_contiguous() and planes.dtype == torch.float32 and tuple(planes.shape) == (self.G, 15, 10, 9)
        before = self.hit.cpu().numpy().copy()
        e.slot_logits.view(torch.int32).fill_(SENT_LOGIT)
        e.slot_value.view(torch.int32).fill_(SENT_VALUE)
        hip.check(lib.xq_evcache_probe(C.byref(e.cache), C.byref(e.h), planes.data_ptr(), sp), "xq_evcache_probe")
        hip.check(lib.xq_engine_compact_misses(C.byref(e.h), planes.data_ptr(), e._cache_hit_ptr, sp), "xq_engine_compact_misses")
        torch.cuda.synchronize()
        flags = self.hit.cpu().numpy().copy()
        logits = e.slot_logits.view(torch.int32).cpu().numpy()
        value = e.slot_value.view(torch.int32).cpu().numpy()
        n_live = int(e.n_live.cpu().numpy()[0])
        want_flags, misses = before.copy(), []                      # an idle slot's flag keeps its previous value
        want_logits = np.full((self.G, M.MAXM), SENT_LOGIT, np.int32)   # a missed or idle slot's rows keep the sentinel
        want_value = np.full(self.G, SENT_VALUE, np.int32)
        for slot in self.waiting:
            hit, row, val = self.model.probe_key(slot, keys[slot], int(self.counts[slot]))
            want_flags[slot] = int(hit)
            if hit:
                want_logits[slot], want_value[slot] = np.frombuffer(row, np.int32), val
            else:
                misses.append(slot)
        assert flags.tolist() == want_flags.tolist()
        assert (logits == want_logits).all(), f"rows differ at slots {np.flatnonzero((logits != want_logits).any(1)).tolist()}"
        assert (value == want_value).all()
        assert n_live == len(misses)
        assert e.packed_rows.cpu().numpy()[:n_live].tolist() == misses
        if n_live:
            idx = torch.tensor(misses, device="cuda")
            assert torch.equal(e.packed_x[:n_live].view(torch.int32), planes[idx].view(torch.int32))
            assert e.packed_counts.cpu().numpy()[:n_live].tolist() == self.counts[misses].tolist()
        for rows, values in commits:
            packed_rows, packed_values = np.zeros((self.G, M.MAXM), np.int32), np.zeros(self.G, np.int32)
            packed_rows[:n_live], packed_values[:n_live] = rows[misses], values[misses]
            self.rows.copy_(torch.from_numpy(packed_rows))
            self.values.copy_(torch.from_numpy(packed_values))
            hip.check(lib.xq_evcache_commit(C.byref(e.cache), C.byref(e.h), self.rows.data_ptr(), self.values.data_ptr(), sp),
                      "xq_evcache_commit")
            torch.cuda.synchronize()
            for slot in misses:
                self.model.commit(slot, rows[slot].tobytes(), int(values[slot]), int(self.counts[slot]))
        return flags, logits, value


@pytest.fixture(scope="module")
def fixtures():
    """The distinct fixture positions, their keys from the board, and their planes as the device encodes them."""
    import torch
    from xiangqi_alphazero_amd import hip
    boards, sides, keys = M.distinct_positions()
    planes = hip.encode(torch.from_numpy(boards).cuda(), torch.from_numpy(sides.astype(np.int8)).cuda())
    torch.cuda.synchronize()
    assert (M.key_from_planes(planes.cpu().numpy()) == keys).all()
    return boards, sides, keys, planes


def _initial():
    from oracle import xq_oracle as O
    g = O.Game()
    return g.board.reshape(90).copy(), int(g.current_player)


def _oracle_planes(board, side):
    from oracle import xq_oracle as O
    return np.ascontiguousarray(O.encode_state(np.asarray(board, np.int8).reshape(10, 9), int(side)), np.float32)


def _playable(boards, sides, i: int):
    """The first corpus position from index i on that has a legal move: a slot set to it waits with a count above 0."""
    from oracle import xq_oracle as O
    while not len(O.legal_actions(boards[i], int(sides[i]))):
        i += 1
    return boards[i], sides[i]


# ---- 3a: the streams ----------------------------------------------------------------------------------------------------------
STREAM_G = 67                                             # 17 workgroups of 4 waves, the last one ragged
STREAM_IDLE = (5, 6, 66)


@pytest.mark.parametrize("entries", M.STREAM_KS)
def test_streams_probe_by_probe(fixtures, entries):
    import torch
    boards, sides, keys, planes_all = fixtures
    active = [s for s in range(STREAM_G) if s not in STREAM_IDLE]
    assert len(active) == M.STREAM_SLOTS
    streams = M.make_streams(entries, keys)
    # every slot waits on a position of its own (they differ in their legal count); the probed planes are the stream's
    rig = Rig(STREAM_G, entries, {s: _playable(boards, sides, s * 61) for s in active})
    assert rig.idle == list(STREAM_IDLE) and len(set(rig.counts[active].tolist())) > 4
    index = np.zeros((M.T_STEPS, STREAM_G), np.int64)
    index[:, active] = streams.T
    index[:, list(STREAM_IDLE)] = streams[:3].T             # an idle slot's planes are some position too: they must not matter
    index_dev = torch.from_numpy(index).cuda()
    key_bytes = [k.tobytes() for k in keys]
    all_flags = np.zeros((M.T_STEPS, STREAM_G), np.int32)
    for t in range(M.T_STEPS):
        if t in M.INVALIDATE_BEFORE:
            rig.invalidate()
        planes = planes_all[index_dev[t]].contiguous()
        step_keys = {s: key_bytes[index[t, s]] for s in active}
        commits = [_bits(t, STREAM_G)] + ([_bits(1000 + t, STREAM_G)] if t in M.REPEAT_COMMIT else [])
        all_flags[t] = rig.step(planes, step_keys, *commits)[0]
    assert rig.stats() == rig.model.stats
    assert (all_flags[:, list(STREAM_IDLE)] == 0).all()
    st = rig.model.stats
    assert st["probes"] == M.STREAM_SLOTS * M.T_STEPS and st["hits"] >= 0.10 * st["probes"] and st["evictions"] >= 0.05 * st["probes"]


# ---- 3b: the device key -------------------------------------------------------------------------------------------------------
KEY_G, KEY_K, KEY_SLOTS = 96, 16, 91


def _base_nibbles(which: str):
    boards, sides = M.fixture_positions()
    n_corpus = len(np.load(os.path.join(M.ROOT, "tests", "golden", "corpus.npz"))["side"])
    if which == "initial":
        board, side = _initial()
    elif which == "sparse":
        board, side = boards[n_corpus], sides[n_corpus]                     # crafted.npz's first position: two pieces
        assert 0 < np.count_nonzero(board) <= 4
    else:
        board, side = boards[45], sides[45]                                 # a corpus position well into a game
        assert 16 < np.count_nonzero(board) < 32
    planes = _oracle_planes(board, side)
    nib = M.nibbles_from_planes(planes)[0]
    assert (M.planes_from_nibbles(nib) == planes).all() and (M.pack_nibbles(nib) == M.key_numpy(board, side)).all()
    return nib


def _variant(nib, i: int):
    """Variant i of a position's nibbles: square i holds something else (i < 90), or the other side is to move (i = 90)."""
    out = nib.copy()
    if i == 90:
        out[90] ^= 1
    elif nib[i] == 0:
        out[i] = 1 + i % 14                                                 # an empty square is filled
    elif i % 2:
        out[i] = 0                                                          # an occupied square is emptied ...
    else:
        out[i] = nib[i] % 14 + 1                                            # ... or holds another plane's piece
    assert out[i] != nib[i]
    return out


@pytest.mark.parametrize("which", ["initial", "sparse", "midgame"])
def test_device_key_sees_every_square_and_the_side(which):
    import torch
    base = _base_nibbles(which)
    variants = [_variant(base, i) for i in range(KEY_SLOTS)]
    assert len({M.pack_nibbles(v).tobytes() for v in variants} | {M.pack_nibbles(base).tobytes()}) == KEY_SLOTS + 1
    rig = Rig(KEY_G, KEY_K, {s: _initial() for s in range(KEY_SLOTS)})
    slots = list(range(KEY_SLOTS))
    base_np = np.broadcast_to(M.planes_from_nibbles(base), (KEY_G, 15, 10, 9)).copy()
    var_np = base_np.copy()
    for i in slots:
        var_np[i] = M.planes_from_nibbles(variants[i])
    base_dev, var_dev = torch.from_numpy(base_np).cuda(), torch.from_numpy(var_np).cuda()
    base_keys = {s: M.key_from_planes(base_np[s])[0].tobytes() for s in slots}
    var_keys = {s: M.key_from_planes(var_np[s])[0].tobytes() for s in slots}
    A, B = _bits(1, KEY_G), _bits(3, KEY_G)

    def check(out, want_hit, rows):
        flags, logits, value = out
        assert flags[slots].tolist() == [want_hit] * KEY_SLOTS
        if want_hit:
            assert (logits[slots] == rows[0][slots]).all() and (value[slots] == rows[1][slots]).all()

    check(rig.step(base_dev, base_keys, A), 0, None)           # 1: the base, all miss, commit A_i
    check(rig.step(base_dev, base_keys), 1, A)                 # 2: all hit with A_i
    check(rig.step(var_dev, var_keys, B), 0, None)             # 3: slot i probes variant i: 91 misses, commit B_i
    check(rig.step(base_dev, base_keys), 1, A)                 # 4: the base still answers with A_i
    check(rig.step(var_dev, var_keys), 1, B)                   # 5: the variants with B_i
    assert rig.stats() == rig.model.stats == dict(probes=5 * KEY_SLOTS, hits=3 * KEY_SLOTS, inserts=2 * KEY_SLOTS, evictions=0,
                                                  mismatches=0)


def _decode_case():
    """A base and a square whose 15 contents (empty, or a piece of each plane) spread over the K = 16 table's four sets with at
    most four keys each, found with the hash twin: nothing is evicted, so every one of them must still be there."""
    for which in ("sparse", "midgame", "initial"):
        base = _base_nibbles(which)
        for sq in range(90):
            sets = []
            for v in range(15):
                nib = base.copy()
                nib[sq] = v
                sets.append(M.evkey_hash(M.pack_nibbles(nib)) & (M.geometry(KEY_K)[1] - 1))
            if max(np.bincount(sets)) <= 4:
                return base, sq
    raise AssertionError("no square spreads its 15 keys over the sets")


def test_device_key_decodes_every_plane():
    import torch
    base, sq = _decode_case()
    G, slot = 4, 2
    rig = Rig(G, KEY_K, {slot: _initial()})
    planes, keys = [], []
    for v in range(15):
        nib = base.copy()
        nib[sq] = v
        x = np.broadcast_to(M.planes_from_nibbles(nib), (G, 15, 10, 9)).copy()
        planes.append(torch.from_numpy(x).cuda())
        keys.append({slot: M.pack_nibbles(nib).tobytes()})
    assert len({k[slot] for k in keys}) == 15
    for v in range(15):
        flags, _, _ = rig.step(planes[v], keys[v], _bits(100 + v, G))
        assert flags[slot] == 0
    for v in np.random.default_rng(4).permutation(15).tolist():
        flags, logits, value = rig.step(planes[v], keys[v])
        rows, values = _bits(100 + v, G)
        assert flags[slot] == 1 and (logits[slot] == rows[slot]).all() and value[slot] == values[slot]
    assert rig.stats() == rig.model.stats == dict(probes=30, hits=15, inserts=15, evictions=0, mismatches=0)


# ---- 3c: the count mismatch ---------------------------------------------------------------------------------------------------
def test_count_mismatch_picks_the_way_whose_count_matches(fixtures):
    from oracle import xq_oracle as O
    boards, sides, keys, planes_all = fixtures
    X = _initial()
    n_x = len(O.legal_actions(X[0], X[1]))
    other = next(i for i in range(40, 400) if len(O.legal_actions(boards[i], int(sides[i]))) not in (0, n_x))
    Y = (boards[other], sides[other])
    rig = Rig(1, 4, {0: X})
    c1 = int(rig.counts[0])
    P, key = planes_all[45:46].contiguous(), {0: keys[45].tobytes()}
    R1, R2, unused = _bits(1, 1), _bits(2, 1), _bits(3, 1)
    flags, _, _ = rig.step(P, key, R1)
    assert flags[0] == 0
    rig.set_positions({0: Y})
    c2 = int(rig.counts[0])
    assert c1 == n_x and c2 == len(O.legal_actions(Y[0], int(Y[1]))) != c1
    flags, _, _ = rig.step(P, key, R2)                                       # key and generation match, the count does not
    assert flags[0] == 0 and rig.stats()["mismatches"] == 1
    flags, logits, value = rig.step(P, key, unused)                          # ways 0 and 1 hold the key: way 1's count matches
    assert flags[0] == 1 and (logits[0] == R2[0][0]).all() and value[0] == R2[1][0]
    rig.set_positions({0: X})
    assert int(rig.counts[0]) == c1
    flags, logits, value = rig.step(P, key, unused)
    assert flags[0] == 1 and (logits[0] == R1[0][0]).all() and value[0] == R1[1][0]
    assert rig.stats() == rig.model.stats == dict(probes=4, hits=2, inserts=2, evictions=0, mismatches=1)


# ---- 3d: the product path under watch -----------------------------------------------------------------------------------------
def _net(seed):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(64, 2)
    net.load_state_dict(weights.make_state_dict(64, 2, seed=seed, policy_gain=8.0))
    return net


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_cached_step_of_a_self_play_engine(graph):
    """eng.step() itself, eager and replayed: after every step the model is fed what the step probed (the planes and counts of
    the slots that asked) and what it evaluated (the evaluator's packed outputs), and must have predicted the hit flags and the
    rows handed back.  A weight update after step 150 keeps the model's generation in step with the device's."""
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    G, S, K, STEPS, UPDATE_AFTER = 16, 32, 8, 400, 150
    ev, _ = evaluator.make_evaluator(_net(0), "cuda", "hip")
    eng = engine.SelfPlayEngine(engine.make_config(G, S, max_game_length=24, seed=11), "cuda", evaluator=ev, eval_cache_entries=K)
    assert eng.path == "cached"
    off = eng._cache_hit_ptr - eng.cache_ws.data_ptr()
    hit_view = eng.cache_ws[off:off + 4 * G].view(torch.int32)
    model = M.EvCacheModel(G, K)
    for step in range(STEPS):
        if graph and step == 2:                                             # two eager steps first, as capture_step's own warm-up
            assert eng.capture_step(warmup=0)
        if step == UPDATE_AFTER:
            ev.update(_net(5))
            model.invalidate()                                              # the engine bumps the device's word before its next step
        eng.step()
        torch.cuda.synchronize()
        x = eng.nn_input.cpu().numpy().reshape(G, -1)
        counts = eng.req_counts.cpu().numpy()
        flags = hit_view.cpu().numpy()
        n_live = int(eng.n_live.cpu().numpy()[0])
        packed_rows = eng.packed_rows.cpu().numpy()[:n_live].tolist()
        logits = eng.slot_logits.view(torch.int32).cpu().numpy()
        value = eng.slot_value.view(torch.int32).cpu().numpy()
        ev_logits = eng._keep_packed[0].view(torch.int32).cpu().numpy()
        ev_value = eng._keep_packed[1].view(torch.int32).cpu().numpy()
        # Every slot of a refilling engine (no games_target, no staggered start) leaves select waiting, the root of a game the
        # rules have ended included -- and such a root may ask with a count of 0, so the count cannot name the waiting slots.
        waiting = list(range(G))
        keys = M.key_from_planes(x)
        misses = []
        for slot in waiting:
            hit, row, val = model.probe_key(slot, keys[slot], int(counts[slot]))
            assert flags[slot] == int(hit), f"step {step} slot {slot}"
            if hit:
                assert (logits[slot] == np.frombuffer(row, np.int32)).all() and value[slot] == val, f"step {step} slot {slot}"
            else:
                misses.append(slot)
        assert n_live == len(misses) and packed_rows == misses, f"step {step}"
        for r, slot in enumerate(misses):
            assert (logits[slot] == ev_logits[r]).all() and value[slot] == ev_value[r]      # the scatter back to slot order
            model.commit(slot, ev_logits[r].tobytes(), int(ev_value[r]), int(counts[slot]))
    assert eng.launch_mode == ("graph" if graph else "eager")
    st = eng.stats()
    assert {k: st["eval_cache_" + k] for k in M.COUNTERS} == model.stats
    assert model.stats["probes"] == G * STEPS
    print(f"{eng.launch_mode}: {model.stats}")
    assert model.stats["hits"] > 0 and model.stats["evictions"] > 0 and model.gen == 2
