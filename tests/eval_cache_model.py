"""Host twin of the evaluation cache (csrc/xq_evcache.hip, include/xq_hip.h), written from the rules at the top of the source and
not from its kernels: the 12-word key, its hash, the W-way sets, the probe clock, the stamp refresh, the victim order, the
generation and the five counters.  tests/test_eval_cache_model.py shows that the streams below tell this model from the wrong
ones; tests/test_eval_cache_kernels_gpu.py holds the kernels to it probe by probe.  Test infrastructure only.

A row and a value are stored as the caller hands them in (the GPU tests hand in the int32 bit patterns of 128 logits and of the
value; the CPU tests a token of the inserting step) and come back unchanged on a hit."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYW, MAXM, STATE_FLOATS = 12, 128, 1350
COUNTERS = ("probes", "hits", "inserts", "evictions", "mismatches")


# ---- key ---------------------------------------------------------------------------------------------------------------------
def pack_nibbles(nib):
    """nibbles [..., n <= 96] -> uint32 [..., 12]: nibble i sits at bits 4 (i mod 8) of word i / 8."""
    nib = np.asarray(nib, np.uint64)
    full = np.zeros(nib.shape[:-1] + (96,), np.uint64)
    full[..., :nib.shape[-1]] = nib
    full = full.reshape(nib.shape[:-1] + (12, 8))
    return (full << (4 * np.arange(8, dtype=np.uint64))).sum(-1).astype(np.uint32)


def key_numpy(board, side):
    """Independent re-derivation from the board: nibble = |piece| for the side to move's pieces, |piece| + 7 for the
    opponent's, 0 when empty (the planes' order, game.py:618-640); nibble 90 = red to move."""
    b = np.asarray(board, np.int64).reshape(90)
    nib = np.where(b == 0, 0, np.where(b * side > 0, np.abs(b), np.abs(b) + 7))
    nib = np.concatenate([nib, [1 if side == 1 else 0], np.zeros(5, np.int64)])
    return np.array([sum(int(nib[8 * w + j]) << (4 * j) for j in range(8)) for w in range(12)], np.uint32)


def nibbles_from_planes(planes):
    """planes float32 [..., 15 * 90] (any shape with 1350 trailing elements per position) -> nibbles [..., 91]: 1 + the highest
    piece plane that is non-zero at the square, 0 when none is; nibble 90 from the first element of plane 14."""
    p = np.asarray(planes, np.float32)
    p = p.reshape(-1, 15, 90)
    occ = p[:, :14, :] != 0
    nib = (occ * np.arange(1, 15)[None, :, None]).max(1)
    return np.concatenate([nib, (p[:, 14, :1] != 0).astype(nib.dtype)], axis=1)


def key_from_planes(planes):
    """The 12 key words of every position in `planes`: uint32 [n, 12]."""
    return pack_nibbles(nibbles_from_planes(planes))


def planes_from_nibbles(nib):
    """Hand-made planes of 91 nibbles (the inverse of nibbles_from_planes): float32 [15, 10, 9]."""
    nib = np.asarray(nib, np.int64).reshape(91)
    x = np.zeros((15, 90), np.float32)
    for sq in range(90):
        if nib[sq]:
            x[nib[sq] - 1, sq] = 1.0
    x[14, :] = float(nib[90] != 0)
    return x.reshape(15, 10, 9)


def evkey_hash(key) -> int:
    """FNV-1a over the 12 words, then one xorshift-multiply round; all mod 2^32."""
    h = 0x811C9DC5
    for w in np.asarray(key, np.uint32).reshape(KEYW).tolist():
        h = ((h ^ w) * 0x01000193) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    return h


def geometry(entries: int):
    """-> (ways, sets) of a table with `entries` entries per slot."""
    ways = min(4, entries)
    return ways, entries // ways


# ---- the model ---------------------------------------------------------------------------------------------------------------
class Entry:
    __slots__ = ("gen", "stamp", "count", "value", "row", "key")

    def __init__(self):
        self.gen, self.stamp, self.count, self.value, self.row, self.key = 0, 0, 0, None, None, None


class EvCacheModel:
    """One cache: `n_slots` private tables of `entries` entries.  The rules a wrong cache would get wrong are methods of their
    own (`set_index`, `matches`, `pick_hit`, `on_hit`, `victim`) so that the mutants of the CPU test override one each."""

    def __init__(self, n_slots: int, entries: int):
        assert n_slots > 0 and entries > 0 and entries & (entries - 1) == 0
        self.G, self.K = n_slots, entries
        self.W, self.sets = geometry(entries)
        self.gen = 1                                                   # entries start in generation 0: never a hit
        self.clock = [0] * n_slots
        self.last_key = [None] * n_slots
        self.table = [[Entry() for _ in range(entries)] for _ in range(n_slots)]
        self.stats = dict.fromkeys(COUNTERS, 0)
        self.generation_decided = [0]      # per generation so far: inserts that only the generation rule places (see commit)
        self._hashes = {}

    # -- the rules
    def hash_of(self, key: bytes) -> int:
        h = self._hashes.get(key)
        if h is None:
            h = self._hashes[key] = evkey_hash(np.frombuffer(key, np.uint32))
        return h

    def set_index(self, h: int) -> int:
        return h & (self.sets - 1)

    def matches(self, e: Entry, key: bytes, count: int) -> bool:
        return e.key == key and e.gen == self.gen and e.count == count

    def pick_hit(self, ways):
        return ways[0]                                                 # the lowest way that matches

    def on_hit(self, e: Entry, clock: int):
        e.stamp = clock

    def victim(self, ways) -> int:
        for w, e in enumerate(ways):
            if e.gen != self.gen:
                return w                                               # the first way of an older generation
        return min(range(len(ways)), key=lambda w: (ways[w].stamp, w))     # else the oldest stamp, lowest way on ties

    # -- the operations
    def _set(self, slot: int, key: bytes):
        s = self.set_index(self.hash_of(key))
        return self.table[slot][s * self.W:(s + 1) * self.W]

    def probe_key(self, slot: int, key, count: int):
        """-> (hit, row, value); row and value are None on a miss."""
        key = np.ascontiguousarray(key, np.uint32).tobytes() if not isinstance(key, bytes) else key
        assert len(key) == 4 * KEYW
        self.clock[slot] += 1
        self.last_key[slot] = key
        ways = self._set(slot, key)
        self.stats["probes"] += 1
        same = [e for e in ways if self.matches(e, key, count)]
        if same:
            e = self.pick_hit(same)
            self.on_hit(e, self.clock[slot])
            self.stats["hits"] += 1
            return True, e.row, e.value
        if any(e.key == key and e.gen == self.gen for e in ways):
            self.stats["mismatches"] += 1                              # key and generation match, no way matches the count too
        return False, None, None

    def probe(self, slot: int, planes, count: int):
        return self.probe_key(slot, key_from_planes(planes)[0], count)

    def commit(self, slot: int, row, value, count: int):
        """Insert under the key `slot` probed last."""
        key = self.last_key[slot]
        assert key is not None, "commit before any probe of the slot"
        ways = self._set(slot, key)
        w = self.victim(ways)
        e = ways[w]
        self.stats["inserts"] += 1
        if all(x.gen == self.gen for x in ways):
            self.stats["evictions"] += 1                               # a live entry of the current generation is replaced
        elif e.gen != self.gen and any(x.stamp < e.stamp for x in ways):
            self.generation_decided[-1] += 1                           # the generation rule chose: the oldest stamp is elsewhere
        e.gen, e.stamp, e.count, e.value, e.row, e.key = self.gen, self.clock[slot], int(count), value, row, key
        return w

    def invalidate(self):
        self.gen += 1
        self.generation_decided.append(0)


# ---- fixtures and the streams shared by the CPU and the GPU test -------------------------------------------------------------
T_STEPS = 256
INVALIDATE_BEFORE = (100, 180)
# On these steps the commit is issued twice (the second time with another row): the entry points accept it -- the probed key,
# the packed rows and their count stand -- and it is the only way to two entries of one set with equal stamps and equal keys,
# without which "lowest way on ties" and "the lowest matching way" would decide nothing.
REPEAT_COMMIT = frozenset(range(2, T_STEPS, 5))
STREAM_SLOTS = 64
STREAM_KS = (1, 2, 4, 8, 16, 64)


def fixture_positions():
    """Every position of corpus.npz and crafted.npz: (boards int8 [n, 90], sides int64 [n])."""
    corpus = np.load(os.path.join(ROOT, "tests", "golden", "corpus.npz"))
    crafted = np.load(os.path.join(ROOT, "tests", "golden", "crafted.npz"))
    boards = np.concatenate([corpus["board"], crafted["board"]])
    sides = np.concatenate([corpus["side"], crafted["side"]]).astype(np.int64)
    return boards, sides


_distinct = None


def distinct_positions():
    """The fixture positions with every key once, in fixture order: (boards, sides, keys uint32 [n, 12])."""
    global _distinct
    if _distinct is None:
        boards, sides = fixture_positions()
        keys = np.stack([key_numpy(b, s) for b, s in zip(boards, sides)])
        _, first = np.unique(keys, axis=0, return_index=True)
        first.sort()
        _distinct = (boards[first], sides[first], keys[first])
    return _distinct


def make_streams(entries: int, keys, seed: int = 20, hot: float = 0.5):
    """int [STREAM_SLOTS, T_STEPS], indices into `keys`: per slot a pool of 3 K + 4 distinct positions and T draws, each with
    probability 0.6 one of the 6 most recently used positions and otherwise uniform over the pool.  With four sets or more, the
    share `hot` of a pool comes from the positions of the lowest quarter of the sets, so that some sets fill up and evict
    between two invalidations however large the table is."""
    rng = np.random.default_rng([seed, entries])
    P = 3 * entries + 4
    _, sets = geometry(entries)
    everything = np.arange(len(keys))
    crowded = everything
    if sets >= 4:
        crowded = np.array([i for i in everything if (evkey_hash(keys[i]) & (sets - 1)) < sets // 4])
    n_hot = int(P * hot) if sets >= 4 else 0
    assert P <= len(keys) and n_hot <= len(crowded)
    out = np.zeros((STREAM_SLOTS, T_STEPS), np.int64)
    for s in range(STREAM_SLOTS):
        pool = rng.choice(crowded, n_hot, replace=False)
        rest = np.setdiff1d(everything, pool)
        pool = np.concatenate([pool, rng.choice(rest, P - n_hot, replace=False)])
        recent = []
        for t in range(T_STEPS):
            if recent and rng.random() < 0.6:
                pos = recent[int(rng.integers(len(recent)))]
            else:
                pos = int(pool[int(rng.integers(P))])
            if pos in recent:
                recent.remove(pos)
            recent.insert(0, pos)
            del recent[6:]
            out[s, t] = pos
    return out


def run_streams(model, streams, keys, counts, row_of, slots=None):
    """Drive `model` through `streams` the way the GPU test drives the kernels: per step an invalidation where the recipe has
    one, a probe of every slot, a commit of every miss, a second commit on the steps of REPEAT_COMMIT.  `row_of(t, slot, again)`
    -> (row, value).  Returns (flags bool [slots, T], returned: per slot and step the (row, value) handed back on a hit)."""
    n, T = streams.shape
    slots = list(range(n)) if slots is None else list(slots)
    flags = np.zeros((n, T), bool)
    returned = [[None] * T for _ in range(n)]
    for t in range(T):
        if t in INVALIDATE_BEFORE:
            model.invalidate()
        for i, slot in enumerate(slots):
            hit, row, value = model.probe_key(slot, keys[streams[i, t]], counts[i])
            flags[i, t] = hit
            if hit:
                returned[i][t] = (row, value)
        for again in ((False, True) if t in REPEAT_COMMIT else (False,)):
            for i, slot in enumerate(slots):
                if not flags[i, t]:
                    model.commit(slot, *row_of(t, slot, again), counts[i])
    return flags, returned


def run_mismatch_scenario(model, key, c1: int, c2: int, r1, r2, slot: int = 0):
    """The count-mismatch script of the GPU test on the model: the same planes probed under two legal counts.  `r1`, `r2` are
    (row, value).  Returns the four probes' (hit, row, value)."""
    out = [model.probe_key(slot, key, c1)]
    model.commit(slot, *r1, c1)
    out.append(model.probe_key(slot, key, c2))           # key and generation match, the count does not: a mismatch
    model.commit(slot, *r2, c2)
    out.append(model.probe_key(slot, key, c2))           # two ways hold the key: the one whose count matches answers
    out.append(model.probe_key(slot, key, c1))
    return out
