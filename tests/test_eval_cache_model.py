"""The evaluation cache's host twin (tests/eval_cache_model.py) on the CPU: its key against the library's host key, its
geometry and bookkeeping on a scenario written out by hand, and the power of the streams the GPU test
(tests/test_eval_cache_kernels_gpu.py) puts through the kernels -- every wrong cache below answers at least one probe of them
differently from the right one, so kernels that agree with the model probe by probe have none of these defects."""
import numpy as np
import pytest

import eval_cache_model as M


# ---- the wrong caches ---------------------------------------------------------------------------------------------------------
class Fifo(M.EvCacheModel):
    def on_hit(self, e, clock):                       # no stamp refresh on a hit
        pass


class TieHigh(M.EvCacheModel):
    def victim(self, ways):                           # highest way on stamp ties
        for w, e in enumerate(ways):
            if e.gen != self.gen:
                return w
        return min(range(len(ways)), key=lambda w: (ways[w].stamp, -w))


class SetFromOtherBits(M.EvCacheModel):
    def set_index(self, h):
        return (h >> 16) & (self.sets - 1)


class GenerationIgnored(M.EvCacheModel):
    def matches(self, e, key, count):
        return e.key == key and e.count == count


class CountIgnored(M.EvCacheModel):
    def matches(self, e, key, count):
        return e.key == key and e.gen == self.gen


class NoOlderGenerationFirst(M.EvCacheModel):
    def victim(self, ways):                           # the oldest stamp, whatever its generation
        return min(range(len(ways)), key=lambda w: (ways[w].stamp, w))


class HighestMatchingWay(M.EvCacheModel):
    def pick_hit(self, ways):
        return ways[-1]


def _mutants(entries):
    """The mutants that are meaningful at this table size (the count mutant has its own scenario below)."""
    ways, sets = M.geometry(entries)
    out = [GenerationIgnored]
    if ways > 1:
        out += [Fifo, TieHigh, NoOlderGenerationFirst, HighestMatchingWay]
    if sets > 1:
        out += [SetFromOtherBits]
    return out


def _row_of(t, slot, again):
    return (t, slot, again), (t, again)               # a token of the inserting step for the row and for the value


def _run(cls, entries):
    _, _, keys = M.distinct_positions()
    streams = M.make_streams(entries, keys)
    model = cls(M.STREAM_SLOTS, entries)
    counts = [20 + s % 30 for s in range(M.STREAM_SLOTS)]
    key_bytes = [k.tobytes() for k in keys]
    flags, returned = M.run_streams(model, streams, key_bytes, counts, _row_of)
    return model, flags, returned


@pytest.fixture(scope="module")
def right():
    return {K: _run(M.EvCacheModel, K) for K in M.STREAM_KS}


@pytest.mark.parametrize("entries", M.STREAM_KS)
def test_every_mutant_diverges_on_the_streams(right, entries):
    _, flags, returned = right[entries]
    for cls in _mutants(entries):
        _, f2, r2 = _run(cls, entries)
        differ = [s for s in range(M.STREAM_SLOTS) if (f2[s] != flags[s]).any() or r2[s] != returned[s]]
        print(f"K {entries} {cls.__name__}: diverges on {len(differ)} of {M.STREAM_SLOTS} slots")
        assert differ, f"{cls.__name__} is not told from the model at K = {entries}"


@pytest.mark.parametrize("entries", M.STREAM_KS)
def test_stream_conditions(right, entries):
    model, flags, _ = right[entries]
    st = model.stats
    assert st["probes"] == M.STREAM_SLOTS * M.T_STEPS and st["hits"] == int(flags.sum())
    print(f"K {entries}: hit rate {st['hits'] / st['probes']:.3f}, evictions {st['evictions']}, inserts {st['inserts']}, "
          f"generation-decided inserts {model.generation_decided}")
    assert st["hits"] >= 0.10 * st["probes"]
    assert st["evictions"] >= 0.05 * st["probes"]
    assert st["mismatches"] == 0
    # After each invalidation an insert that the generation rule alone places: it lands on the first older-generation way
    # while another way holds an older stamp, so a search by stamp would have gone elsewhere.  (A way of the CURRENT generation
    # can never hold the older stamp: the clock only grows and every current stamp is from after the invalidation.)
    assert len(model.generation_decided) == 1 + len(M.INVALIDATE_BEFORE)
    if model.W > 1:
        assert all(n > 0 for n in model.generation_decided[1:])


def test_count_mutant_diverges_on_the_mismatch_scenario():
    _, _, keys = M.distinct_positions()
    r1, r2 = ("row1", "value1"), ("row2", "value2")
    good = M.EvCacheModel(1, 4)
    out = M.run_mismatch_scenario(good, keys[0], 44, 31, r1, r2)
    assert out == [(False, None, None), (False, None, None), (True,) + r2, (True,) + r1]
    assert good.stats == dict(probes=4, hits=2, inserts=2, evictions=0, mismatches=1)
    bad = CountIgnored(1, 4)
    assert M.run_mismatch_scenario(bad, keys[0], 44, 31, r1, r2) != out


# ---- the twin's own checks ----------------------------------------------------------------------------------------------------
def test_geometry():
    assert [M.geometry(k) for k in (1, 2, 4, 8, 16, 64)] == [(1, 1), (2, 1), (4, 1), (4, 2), (4, 4), (4, 16)]
    for k in (1, 2, 4, 8):
        m = M.EvCacheModel(3, k)
        assert (m.W, m.sets, m.W * m.sets) == (min(4, k), k // min(4, k), k)
        assert all(0 <= m.set_index(h) < m.sets for h in (0, 1, 0xFFFFFFFF, 0x12345678))


def test_hash_twin_on_written_out_values():
    # FNV-1a of twelve zero words is the offset basis times the prime twelve times; the finisher is checked on it by hand
    h = 0x811C9DC5
    for _ in range(12):
        h = (h * 0x01000193) % 2 ** 32
    h ^= h >> 16
    h = (h * 0x7FEB352D) % 2 ** 32
    h ^= h >> 15
    assert M.evkey_hash(np.zeros(12, np.uint32)) == h
    one = np.zeros(12, np.uint32)
    one[11] = 1
    assert M.evkey_hash(one) != h and 0 <= M.evkey_hash(np.full(12, 0xFFFFFFFF, np.uint32)) < 2 ** 32


def test_planes_key_matches_the_board_key_and_the_library():
    """Three derivations of the key agree on every fixture position: from the board, from the planes (what the model's probe
    uses) and the library's host key."""
    import ctypes as C  # noqa: F401
    from oracle import xq_oracle as O
    from xiangqi_alphazero_amd import hip
    hip.build()
    lib = hip.lib()
    boards, sides, keys = M.distinct_positions()
    planes = np.stack([np.ascontiguousarray(O.encode_state(b.reshape(10, 9), int(s)), np.float32) for b, s in zip(boards, sides)])
    assert (M.key_from_planes(planes) == keys).all()
    out = np.zeros(12, np.uint32)
    for i in range(0, len(keys), 7):
        assert lib.xq_evcache_key_host(np.ascontiguousarray(planes[i]).ctypes.data, out.ctypes.data) == 0
        assert (out == keys[i]).all()
    # hand-made planes decode to the nibbles they were made of
    rng = np.random.default_rng(1)
    nib = rng.integers(0, 15, 91)
    nib[90] = 1
    assert (M.nibbles_from_planes(M.planes_from_nibbles(nib))[0] == nib).all()


def test_clock_and_stamps_on_a_hand_written_scenario():
    """K = 2: one set of two ways.  Ten probes of one slot, keys A B C, an invalidation before the eighth."""
    A, B, C_ = (np.full(12, v, np.uint32).tobytes() for v in (1, 2, 3))
    m = M.EvCacheModel(2, 2)
    script = [A, B, A, C_, B, A, B, "invalidate", B, A, B]
    flags, rows, t = [], [], 0
    for k in script:
        if k == "invalidate":
            m.invalidate()
            continue
        t += 1
        hit, row, _ = m.probe_key(1, k, 5)
        flags.append(int(hit))
        rows.append(row)
        if not hit:
            m.commit(1, t, None, 5)
    #                1  2  3  4  5  6  7  8  9  10
    assert flags == [0, 0, 1, 0, 0, 0, 1, 0, 0, 1]
    # 3: A from probe 1.  4: C evicts B (stamp 2 < A's refreshed 3).  5: B evicts A.  6: A evicts C.  7: B from probe 5.
    # 8, 9: the older generation's ways are refilled in way order, nothing is evicted.  10: B from probe 8.
    assert rows == [None, None, 1, None, None, None, 5, None, None, 8]
    assert m.clock == [0, 10]
    way0, way1 = m.table[1]
    assert (way0.key, way0.stamp, way0.gen, way1.key, way1.stamp, way1.gen) == (B, 10, 2, A, 9, 2)
    assert m.stats == dict(probes=10, hits=3, inserts=7, evictions=3, mismatches=0)
    assert all(e.gen == 0 for e in m.table[0])                    # the other slot's table is its own
