"""CPU-side checks of the evaluation cache's C ABI (xq_evcache_*, xq_engine_compact_misses; include/xq_hip.h): the exports,
argument errors before any launch, the documented table layout, and the key -- an exact, injective packing of the planes
the engine hands to the network -- against a numpy re-derivation over every fixture position."""
import ctypes as C
import os

import numpy as np
import pytest

from eval_cache_model import fixture_positions as _fixture_positions, key_numpy as _key_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["xq_evcache_bytes", "xq_evcache_init", "xq_evcache_hit_flags", "xq_evcache_probe", "xq_engine_compact_misses",
       "xq_evcache_commit", "xq_evcache_invalidate", "xq_evcache_stats_read", "xq_evcache_key_host"]


@pytest.fixture(scope="module")
def lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


def test_new_symbols_are_declared_and_exported(lib):
    from xiangqi_alphazero_amd import hip
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)


def _align(x):
    return (x + 255) & ~255


def _layout_bytes(G, K):
    GK = G * K
    parts = [4, G * 4, G * 4, G * 48, G * 64,                      # generation, clocks, hit flags, probe keys, counters
             GK * 4, GK * 4, GK * 4, GK * 4, GK * 48, GK * 512]    # entry generation, stamp, count, value, key, logits
    return sum(_align(p) for p in parts)


def test_bytes_match_the_documented_layout(lib):
    from xiangqi_alphazero_amd import engine
    for G, K in ((1, 1), (3, 2), (128, 4), (1024, 1024), (8192, 2048)):
        assert lib.xq_evcache_bytes(G, K) == _layout_bytes(G, K) == engine.eval_cache_bytes(G, K)
    # 576 B per entry: BASELINE configs[2] with the recommended K is ~9.7 GB
    assert 9.6e9 < lib.xq_evcache_bytes(8192, 2048) < 9.7e9
    for G, K in ((0, 4), (-1, 4), (8, 0), (8, -4), (8, 3), (8, 12)):
        assert lib.xq_evcache_bytes(G, K) == 0


def test_recommended_entries():
    from xiangqi_alphazero_amd import engine
    assert [engine.recommended_cache_entries(s) for s in (1, 8, 64, 100, 400, 800)] == [2, 16, 128, 256, 1024, 2048]


def _fake_cache(n_slots=8, entries=4):
    from xiangqi_alphazero_amd import hip
    c = hip.EvCache()
    c.n_slots, c.entries = n_slots, entries
    c.ways = min(4, entries) if entries > 0 else 0
    c.sets = entries // c.ways if c.ways else 0
    for i in range(16):
        c.p[i] = 0x100000 + 0x1000 * i                             # never dereferenced: every call below fails first
    return c


def _fake_engine(n_games=8):
    from xiangqi_alphazero_amd import hip
    e = hip.Engine()
    e.cfg.n_games = n_games
    for i in range(32):
        e.p[i] = 0x200000 + 0x1000 * i
    return e


def test_argument_errors_without_gpu(lib):
    ARG, WS = -1, -3
    B = C.byref
    c, e = _fake_cache(), _fake_engine()
    x, buf = 0x300000, 0x400000                                    # aligned stand-ins for device addresses
    # init: bad geometry, null / misaligned memory, short buffer -- all before any HIP call
    assert lib.xq_evcache_init(None, 8, 4, buf, 1 << 20, None) == ARG
    assert lib.xq_evcache_init(B(c), 8, 3, buf, 1 << 20, None) == ARG
    assert lib.xq_evcache_init(B(c), 8, 0, buf, 1 << 20, None) == ARG
    assert lib.xq_evcache_init(B(c), 0, 4, buf, 1 << 20, None) == ARG
    assert lib.xq_evcache_init(B(c), 8, 4, None, 1 << 20, None) == ARG
    assert lib.xq_evcache_init(B(c), 8, 4, buf + 16, 1 << 20, None) == ARG
    assert lib.xq_evcache_init(B(c), 8, 4, buf, lib.xq_evcache_bytes(8, 4) - 1, None) == WS
    # probe: null pointers, slot count differing from the engine's, a broken geometry
    assert lib.xq_evcache_probe(None, B(e), x, None) == ARG
    assert lib.xq_evcache_probe(B(c), None, x, None) == ARG
    assert lib.xq_evcache_probe(B(c), B(e), None, None) == ARG
    assert lib.xq_evcache_probe(B(c), B(_fake_engine(16)), x, None) == ARG
    assert lib.xq_evcache_probe(B(_fake_cache(8, 3)), B(e), x, None) == ARG
    nulled = _fake_cache()
    nulled.p[0] = None
    assert lib.xq_evcache_probe(B(nulled), B(e), x, None) == ARG
    # compaction of the misses
    assert lib.xq_engine_compact_misses(None, x, x, None) == ARG
    assert lib.xq_engine_compact_misses(B(e), None, x, None) == ARG
    assert lib.xq_engine_compact_misses(B(e), x, None, None) == ARG
    assert lib.xq_engine_compact_misses(B(_fake_engine(0)), x, x, None) == ARG
    # commit: misaligned logits, nulls, slot count
    assert lib.xq_evcache_commit(B(c), B(e), x + 4, x, None) == ARG
    assert lib.xq_evcache_commit(B(c), B(e), None, x, None) == ARG
    assert lib.xq_evcache_commit(B(c), B(e), x, None, None) == ARG
    assert lib.xq_evcache_commit(B(c), B(_fake_engine(4)), x, x, None) == ARG
    assert lib.xq_evcache_commit(None, B(e), x, x, None) == ARG
    # the rest
    assert lib.xq_evcache_invalidate(None, None) == ARG
    assert lib.xq_evcache_invalidate(B(_fake_cache(8, 0)), None) == ARG
    assert lib.xq_evcache_stats_read(None, None, None) == ARG
    assert lib.xq_evcache_stats_read(B(c), None, None) == ARG
    assert lib.xq_evcache_hit_flags(B(c), None) == ARG
    assert lib.xq_evcache_hit_flags(None, B(C.c_void_p())) == ARG
    hp = C.c_void_p()
    assert lib.xq_evcache_hit_flags(B(c), B(hp)) == 0 and hp.value == c.p[2]
    assert lib.xq_evcache_key_host(None, None) == ARG


def _planes(board, side):
    from oracle import xq_oracle as O
    return np.ascontiguousarray(O.encode_state(np.asarray(board, np.int8).reshape(10, 9), int(side)), np.float32).reshape(15, 90)


def _key_host(lib, planes):
    out = np.zeros(12, np.uint32)
    assert lib.xq_evcache_key_host(np.ascontiguousarray(planes, np.float32).ctypes.data, out.ctypes.data) == 0
    return out


def test_key_matches_numpy_and_is_injective_over_the_fixtures(lib):
    boards, sides = _fixture_positions()
    keys, seen = {}, {}
    for b, s in zip(boards, sides):
        k = _key_host(lib, _planes(b, s))
        assert (k == _key_numpy(b, s)).all()
        keys.setdefault(k.tobytes(), set()).add((b.tobytes(), int(s)))
        seen[(b.tobytes(), int(s))] = k.tobytes()
    assert all(len(v) == 1 for v in keys.values()), "two different positions share a key"
    assert len(keys) == len(seen) > 1000


def test_one_square_or_the_side_changes_the_key(lib):
    boards, sides = _fixture_positions()
    rng = np.random.default_rng(5)
    for i in rng.choice(len(boards), 200, replace=False):
        b, s = boards[i].copy(), int(sides[i])
        k = _key_host(lib, _planes(b, s)).tobytes()
        assert _key_host(lib, _planes(b, -s)).tobytes() != k                 # only the side to move differs
        sq = int(rng.integers(90))
        for v in (0, 1, -1, 5, -7):
            if v == b[sq]:
                continue
            b2 = b.copy()
            b2[sq] = v
            assert _key_host(lib, _planes(b2, s)).tobytes() != k              # one square differs
