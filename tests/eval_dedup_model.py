"""Host twin of the request dedup's resolve rule (csrc/xq_evdedup.hip, include/xq_hip.h), written from the rules in the header and
not from the kernels: from the keys, the legal-move counts, the live flags and the table size it gives rep[], the packed rows[]
and the four counters.  The bucket of a key is the library's own host function (xq_evdedup_bucket_host), which
tests/test_eval_dedup_abi.py holds to a numpy re-derivation.  tests/test_eval_dedup_model.py shows that the crafted streams
below tell this twin from the wrong ones; tests/test_eval_dedup_kernels_gpu.py holds the kernels to it.  Test infrastructure only."""
import numpy as np

import eval_cache_model as EC

ROOT = EC.ROOT
COUNTERS = ("requests", "merged", "collisions", "mismatches")
EMPTY = 2 ** 31 - 1
SIZES = (1, 3, 4, 5, 1030)            # a ragged last workgroup of four waves; more than one row per compaction thread


def table_size(n_slots: int) -> int:
    """The smallest power of two >= max(16, 4 n_slots)."""
    t = 16
    while t < 4 * n_slots:
        t *= 2
    return t


def lib_bucket(key, T: int) -> int:
    from xiangqi_alphazero_amd import hip
    return hip.dedup_bucket(np.frombuffer(key, np.uint32) if isinstance(key, bytes) else key, T)


class DedupModel:
    """The rules a wrong dedup would get wrong are methods of their own, so that the mutants of the CPU test override one each."""

    def __init__(self, bucket_of=lib_bucket):
        self.bucket_of = bucket_of

    def enters_table(self, live: bool) -> bool:
        return live                                               # only a row that asks may represent anything

    def pick(self, members):
        return min(members)                                       # atomicMin: the lowest row of the bucket

    def same_key(self, a: bytes, b: bytes) -> bool:
        return a == b                                             # all 12 words

    def same_count(self, a: int, b: int) -> bool:
        return a == b

    def resolve(self, keys, counts, live, T: int):
        """keys: n entries of 48 bytes (or uint32 [n, 12]); counts, live: n ints -> (rep dict {live row: its representative},
        rows list, counters dict)."""
        keys = [k if isinstance(k, bytes) else np.ascontiguousarray(k, np.uint32).tobytes() for k in keys]
        n = len(keys)
        assert len(counts) == n and len(live) == n and T >= 16 and T & (T - 1) == 0
        bucket = [self.bucket_of(k, T) for k in keys]
        table = {}
        for r in range(n):
            if self.enters_table(bool(live[r])):
                table.setdefault(bucket[r], []).append(r)
        rep, st = {}, dict.fromkeys(COUNTERS, 0)
        for s in range(n):
            if not live[s]:
                continue
            st["requests"] += 1
            m = self.pick(table[bucket[s]]) if bucket[s] in table else s
            if m == s:
                rep[s] = s
            elif self.same_key(keys[m], keys[s]) and self.same_count(int(counts[m]), int(counts[s])):
                rep[s] = m
                st["merged"] += 1
            else:
                rep[s] = s
                if keys[m] != keys[s]:
                    st["collisions"] += 1
                else:
                    st["mismatches"] += 1
        rows = [s for s in range(n) if live[s] and rep[s] == s]
        return rep, rows, st


# ---- the crafted streams shared by the CPU and the GPU test ------------------------------------------------------------------
def nibbles_of(board, side):
    """The 91 nibbles of a position (eval_cache_model.key_numpy's, unpacked)."""
    b = np.asarray(board, np.int64).reshape(90)
    nib = np.where(b == 0, 0, np.where(b * side > 0, np.abs(b), np.abs(b) + 7))
    return np.concatenate([nib, [1 if side == 1 else 0]]).astype(np.uint8)


def corpus_nibbles():
    """The nibbles and keys of the distinct fixture positions: (uint8 [n, 91], uint32 [n, 12])."""
    boards, sides, keys = EC.distinct_positions()
    nib = np.stack([nibbles_of(b, s) for b, s in zip(boards, sides)])
    assert (EC.pack_nibbles(nib) == keys).all()
    return nib, keys


def numbered(base, i: int):
    """Request i of a family of distinct requests: `base` with i + 1 written, in base 14 with digits 1..14, into its first empty squares."""
    out = np.array(base, np.uint8)
    empty = np.flatnonzero(out[:90] == 0)
    v, j = i + 1, 0
    while v:
        out[empty[j]] = 1 + (v % 14)          # the next empty square stays empty: it ends the number
        v //= 14
        j += 1
    return out


def one_nibble_variant(nib, i: int):
    """Variant i of a position's nibbles: square i holds something else (i < 90), or the other side is to move (i = 90)."""
    out = nib.copy()
    if i == 90:
        out[90] ^= 1
    elif nib[i] == 0:
        out[i] = 1 + i % 14
    elif i % 2:
        out[i] = 0
    else:
        out[i] = nib[i] % 14 + 1
    assert out[i] != nib[i]
    return out


def find_collision(keys, T: int, bucket_of=lib_bucket):
    """-> (a, b, d): the first two distinct fixture positions a < b that share a bucket of a T-bucket table, and the first
    position d of another bucket.  A search on the CPU."""
    seen = {}
    for i, k in enumerate(keys):
        b = bucket_of(k, T)
        if b in seen:
            a = seen[b]
            d = next(j for j, kj in enumerate(keys) if bucket_of(kj, T) != b)
            return a, i, d
        seen[b] = i
    raise AssertionError("no two fixture positions share a bucket")


def cases(bucket_of=lib_bucket):
    """name -> (nibbles uint8 [n, 91], counts int32 [n], live int32 [n]).  A case's table has table_size(n) buckets."""
    nib, keys = corpus_nibbles()
    base = nib[0]
    out = {}
    for n in SIZES:
        out[f"identical_{n}"] = (np.repeat(base[None], n, 0), np.full(n, 44, np.int32), np.ones(n, np.int32))
        out[f"distinct_{n}"] = (np.stack([numbered(base, i) for i in range(n)]), np.full(n, 44, np.int32), np.ones(n, np.int32))
        rng = np.random.default_rng([28, n])
        ids = rng.integers(0, max(1, n // 3), n)
        live = (rng.random(n) < 0.8).astype(np.int32)
        out[f"mixed_{n}"] = (np.stack([numbered(base, int(i)) for i in ids]), np.full(n, 30, np.int32), live)
    P, Q = nib[45], nib[46]
    # idle rows whose planes equal a live row's, below and above it: the representative of rows 1 and 3 is row 1, never row 0
    out["idle_twins"] = (np.stack([P, P, Q, P, P, Q]), np.full(6, 37, np.int32), np.array([0, 1, 1, 1, 0, 0], np.int32))
    out["nibble_variants"] = (np.stack([P] + [one_nibble_variant(P, i) for i in range(91)]), np.full(92, 37, np.int32),
                              np.ones(92, np.int32))
    out["count_mismatch"] = (np.stack([P, P, P]), np.array([30, 31, 30], np.int32), np.ones(3, np.int32))
    a, b, d = find_collision(keys, table_size(4), bucket_of)
    out["bucket_collision"] = (np.stack([nib[a], nib[b], nib[b], nib[d]]), np.full(4, 41, np.int32), np.ones(4, np.int32))
    return out


def keys_of(nib):
    return [k.tobytes() for k in EC.pack_nibbles(nib)]


def planes_of(nib):
    """float32 [n, 15, 10, 9] hand-made planes of the nibbles."""
    return np.stack([EC.planes_from_nibbles(x) for x in nib])
