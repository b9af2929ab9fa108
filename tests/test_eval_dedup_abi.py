"""CPU-side checks of the request dedup's C ABI (xq_evdedup_*, xq_engine_compact_unique / _expand_dedup, xq_dedup_rows_batch;
include/xq_hip.h): the exports, the argument rules before any launch, the bucket function against a numpy re-derivation over
every fixture position of corpus.npz, and every refusal of the option, in Python and in C."""
import ctypes as C
import os

import numpy as np
import pytest

import eval_cache_model as EC
import eval_dedup_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["xq_evdedup_bytes", "xq_evdedup_init", "xq_engine_compact_unique", "xq_engine_expand_dedup", "xq_evdedup_stats_read",
       "xq_evdedup_bucket_host", "xq_dedup_rows_batch"]
ARG, WS = -1, -3


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
    assert C.sizeof(hip.EvDedup) == 16 + 8 * 8 and C.sizeof(hip.EvDedupStats) == 64


def _align(x):
    return (x + 255) & ~255


def test_bytes_argument_rules_and_layout(lib):
    for G in (1, 3, 4, 5, 8, 1024, 1030, 8192, 1 << 24):
        T = M.table_size(G)
        parts = [T * 4, G * 48, G * 4, G * 4, G * 4, G * 32, 32 * 8]     # table, keys, bucket, rep, packed row, counters, sink
        assert lib.xq_evdedup_bytes(G) == sum(_align(p) for p in parts)
    for G in (0, -1, -(1 << 31), (1 << 24) + 1, (1 << 31) - 1):
        assert lib.xq_evdedup_bytes(G) == 0
    assert lib.xq_evdedup_bytes(1024) < 128 * 1024                        # configs[1]: 16 KiB of buckets, 92 B per slot


def _fake_dedup(n_slots=8):
    from xiangqi_alphazero_amd import hip
    d = hip.EvDedup()
    d.n_slots, d.table_size = n_slots, M.table_size(max(n_slots, 1))
    for i in range(8):
        d.p[i] = 0x100000 + 0x1000 * i                                    # never dereferenced: every call below fails first
    return d


def _fake_engine(n_games=8, pad0=0, manual_moves=0):
    from xiangqi_alphazero_amd import hip
    e = hip.Engine()
    e.cfg.n_games, e.cfg.manual_moves, e.pad0 = n_games, manual_moves, pad0
    for i in range(32):
        e.p[i] = 0x200000 + 0x1000 * i
    return e


def test_argument_errors_without_gpu(lib):
    B = C.byref
    d, e = _fake_dedup(), _fake_engine()
    x, buf = 0x300000, 0x400000                                           # aligned stand-ins for device addresses
    assert lib.xq_evdedup_init(None, 8, buf, 1 << 20, None) == ARG
    assert lib.xq_evdedup_init(B(d), 0, buf, 1 << 20, None) == ARG
    assert lib.xq_evdedup_init(B(d), (1 << 24) + 1, buf, 1 << 40, None) == ARG
    assert lib.xq_evdedup_init(B(d), 8, None, 1 << 20, None) == ARG
    assert lib.xq_evdedup_init(B(d), 8, buf + 16, 1 << 20, None) == ARG
    assert lib.xq_evdedup_init(B(d), 8, buf, lib.xq_evdedup_bytes(8) - 1, None) == WS
    d = _fake_dedup()
    for fn in (lib.xq_engine_compact_unique,):
        assert fn(None, B(e), x, None) == ARG
        assert fn(B(d), None, x, None) == ARG
        assert fn(B(d), B(e), None, None) == ARG
        assert fn(B(d), B(_fake_engine(16)), x, None) == ARG              # the slot counts differ
        assert fn(B(d), B(_fake_engine(0)), x, None) == ARG
    broken = _fake_dedup()
    broken.table_size = 24
    assert lib.xq_engine_compact_unique(B(broken), B(e), x, None) == ARG
    nulled = _fake_dedup()
    nulled.p[0] = None
    assert lib.xq_engine_compact_unique(B(nulled), B(e), x, None) == ARG
    assert lib.xq_engine_expand_dedup(None, B(e), x, x, None) == ARG
    assert lib.xq_engine_expand_dedup(B(d), None, x, x, None) == ARG
    assert lib.xq_engine_expand_dedup(B(d), B(e), None, x, None) == ARG
    assert lib.xq_engine_expand_dedup(B(d), B(e), x, None, None) == ARG
    assert lib.xq_engine_expand_dedup(B(d), B(e), x + 4, x, None) == ARG  # logits not 8-byte aligned
    assert lib.xq_engine_expand_dedup(B(d), B(_fake_engine(4)), x, x, None) == ARG
    assert lib.xq_evdedup_stats_read(None, None, None) == ARG
    assert lib.xq_evdedup_stats_read(B(d), None, None) == ARG
    assert lib.xq_dedup_rows_batch(x, x, x, -1, B(d), x, x, x, None) == ARG
    assert lib.xq_dedup_rows_batch(x, x, x, 9, B(d), x, x, x, None) == ARG    # more rows than the table was made for
    assert lib.xq_dedup_rows_batch(x, x, x, 4, None, x, x, x, None) == ARG
    assert lib.xq_dedup_rows_batch(x, x, x, 4, B(d), x, x, None, None) == ARG
    for hole in range(3):
        args = [x, x, x]
        args[hole] = None
        assert lib.xq_dedup_rows_batch(*args, 4, B(d), x, x, x, None) == ARG
    assert lib.xq_dedup_rows_batch(x, x, x, 4, B(d), None, x, x, None) == ARG
    assert lib.xq_dedup_rows_batch(x, x, x, 4, B(d), x, None, x, None) == ARG
    key = np.arange(12, dtype=np.uint32)
    assert lib.xq_evdedup_bucket_host(None, 16) == ARG
    for T in (0, -16, 24, 3):
        assert lib.xq_evdedup_bucket_host(key.ctypes.data, T) == ARG


def test_the_engines_the_dedup_refuses_in_c(lib):
    """Leaf batching (pad0's low 16 bits > 1), the evaluation mirror (pad0 bit 31) and arena games (manual_moves = 2) return
    XQ_ERR_ARG from both entry points before any launch; the pointers of these handles are stand-ins nothing may follow."""
    B = C.byref
    d, x = _fake_dedup(), 0x300000
    for e in (_fake_engine(pad0=4), _fake_engine(pad0=-(1 << 31)), _fake_engine(manual_moves=2)):
        assert lib.xq_engine_compact_unique(B(d), B(e), x, None) == ARG
        assert lib.xq_engine_expand_dedup(B(d), B(e), x, x, None) == ARG


def _hash_numpy(key):
    """FNV-1a over the 12 words and one xorshift-multiply round, in uint64 arithmetic masked to 32 bits."""
    h = np.uint64(0x811C9DC5)
    mask = np.uint64(0xFFFFFFFF)
    for w in np.asarray(key, np.uint64):
        h = ((h ^ w) * np.uint64(0x01000193)) & mask
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & mask
    h ^= h >> np.uint64(15)
    return int(h)


def test_bucket_matches_numpy_over_the_corpus(lib):
    from xiangqi_alphazero_amd import hip
    corpus = np.load(os.path.join(ROOT, "tests", "golden", "corpus.npz"))
    boards, sides = corpus["board"], corpus["side"].astype(np.int64)
    assert len(boards) > 500
    used = {16: set(), 4096: set()}
    for b, s in zip(boards, sides):
        key = EC.key_numpy(b, s)
        h = _hash_numpy(key)
        assert h == EC.evkey_hash(key)
        for T in (16, 32, 4096, 1 << 26):
            assert lib.xq_evdedup_bucket_host(key.ctypes.data, T) == h & (T - 1) == hip.dedup_bucket(key, T)
        used[16].add(h & 15)
        used[4096].add(h & 4095)
    assert len(used[16]) == 16 and len(used[4096]) > 400                  # the low bits spread
    with pytest.raises(hip.XqError):
        hip.dedup_bucket(np.zeros(12, np.uint32), 24)
    with pytest.raises(hip.XqError):
        hip.dedup_bucket(np.zeros(11, np.uint32), 16)


class _Live:
    live_rows = True


REFUSED = [
    (dict(eval_cache_entries=8), {}, "evaluation cache"),
    (dict(leaves_per_step=4), {}, "leaves_per_step"),
    (dict(eval_mirror=True), {}, "eval_mirror"),
    (dict(), dict(manual_moves=2), "arena"),
]


@pytest.mark.parametrize("opts, cfg_kw, word", REFUSED, ids=[r[2] for r in REFUSED])
def test_refusals_name_the_option(lib, opts, cfg_kw, word):
    from xiangqi_alphazero_amd import engine, hip
    cfg = engine.make_config(8, 16, **cfg_kw)
    assert engine.parse_engine_options(cfg, **opts).eval_dedup is False                     # fine without the dedup
    with pytest.raises(hip.XqError, match="eval_dedup") as ei:
        engine.parse_engine_options(cfg, eval_dedup=True, **opts)
    assert word in str(ei.value)
    with pytest.raises(hip.XqError, match="eval_dedup"):                                     # the engine refuses before it needs a GPU
        engine.SelfPlayEngine(cfg, "cuda", evaluator=_Live(), eval_dedup=True, **opts)


def test_an_evaluator_without_live_rows_is_refused(lib):
    from xiangqi_alphazero_amd import engine, hip
    cfg = engine.make_config(8, 16)
    for ev in (None, lambda x: x):
        with pytest.raises(hip.XqError, match="eval_dedup.*live_rows"):
            engine.SelfPlayEngine(cfg, "cuda", evaluator=ev, eval_dedup=True)
    with pytest.raises(hip.XqError, match="eval_dedup must be a bool"):
        engine.parse_engine_options(cfg, eval_dedup=2)


def test_the_option_is_off_by_default_and_goes_with_the_rest():
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(8, 16)
    assert engine.parse_engine_options(cfg).eval_dedup is False
    for kw in (dict(tree_reuse=True), dict(playout_cap=(0.25, 4)), dict(forced_playouts=2.0), dict(gumbel=(4, 50.0, 1.0)),
               dict(solver=True), dict(root_stats=True), dict(record_games=True), dict(perpetual_check=True)):
        assert engine.parse_engine_options(cfg, eval_dedup=True, **kw).eval_dedup is True
    assert engine.parse_engine_options(engine.make_config(8, 16, manual_moves=1), eval_dedup=True).eval_dedup is True


def test_the_config_key_reaches_the_engine(monkeypatch):
    """run_games reads config.eval_dedup (absent: off) and hands it to the engine; parallel_self_play and MCTS pass theirs on."""
    import inspect
    from xiangqi_alphazero_amd import mcts, selfplay
    assert inspect.signature(selfplay.run_games).parameters["eval_dedup"].default is None
    assert inspect.signature(selfplay.parallel_self_play).parameters["eval_dedup"].default is None
    assert inspect.signature(mcts.MCTS.__init__).parameters["eval_dedup"].default is False
    seen = {}

    class Stop(Exception):
        pass

    def fake_engine(cfg, device, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(selfplay.evaluator, "make_evaluator", lambda *a, **k: (_Live(), "hip"))
    monkeypatch.setattr(selfplay.engine, "SelfPlayEngine", fake_engine)

    class Cfg:
        num_simulations, c_puct, temperature_threshold, max_game_length, random_opening_moves = 16, 1.5, 20, 30, 0
        enable_resign, resign_threshold, resign_check_steps = False, -0.9, 5

    for value, want in ((None, False), (True, True), (False, False)):
        cfg = Cfg()
        if value is not None:
            cfg.eval_dedup = value
        with pytest.raises(Stop):
            selfplay.run_games(None, cfg, 4)
        assert seen["eval_dedup"] is want
    with pytest.raises(Stop):
        selfplay.run_games(None, Cfg(), 4, eval_dedup=True)
    assert seen["eval_dedup"] is True
