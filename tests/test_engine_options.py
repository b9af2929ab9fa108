"""The two validators of the engine's options side by side, without a GPU: `engine.parse_engine_options` (Python, refuses with a
message that names the option) and opts_ok behind every xq_engine_workspace_bytes_* (C, returns 0).

A case is (name, make_config keywords, option keywords).  The option keywords go to the parser as they are; for the C call the
same values become raw structs with no check in between (`raw`).  The tables are literal: nothing is skipped or filtered."""
import ctypes as C
import types

import pytest

from xiangqi_alphazero_amd import engine, hip

NAN, INF = float("nan"), float("inf")
CAP, FP, GZ, AR = dict(playout_cap=(0.25, 8)), dict(forced_playouts=2.0), dict(gumbel=(16, 50.0, 1.0)), dict(arena_opts=(4, 10))
CACHE = dict(eval_cache_entries=64)

ACCEPTED = [
    ("plain", {}, {}),
    ("K = 4", {}, dict(leaves_per_step=4)),
    ("tree reuse", {}, dict(tree_reuse=True)),
    ("cap", {}, CAP),
    ("forced", {}, FP),
    ("reuse + cap + forced", {}, dict(tree_reuse=True, **CAP, **FP)),
    ("gumbel, self-play", {}, GZ),
    ("gumbel, search only", dict(manual_moves=1), GZ),
    ("arena options", dict(manual_moves=2), AR),
    ("cache, plain", {}, CACHE),
    ("cache + reuse", {}, dict(tree_reuse=True, **CACHE)),
    ("cache + cap", {}, dict(**CAP, **CACHE)),
    ("cache + forced", {}, dict(**FP, **CACHE)),
    ("cache + gumbel", {}, dict(**GZ, **CACHE)),
]

# one case per rule of the refusal lists of include/xq_hip.h; the last field is the option the parser's message must name
REFUSED = [
    ("K < 1", {}, dict(leaves_per_step=0), "leaves_per_step"),
    ("K > 64", {}, dict(leaves_per_step=65), "leaves_per_step"),
    ("K > 1 in the arena", dict(manual_moves=2), dict(leaves_per_step=2), "leaves_per_step"),
    ("reuse, search only", dict(manual_moves=1), dict(tree_reuse=True), "tree_reuse"),
    ("reuse, arena", dict(manual_moves=2), dict(tree_reuse=True), "tree_reuse"),
    ("reuse, K > 1", {}, dict(tree_reuse=True, leaves_per_step=2), "tree_reuse"),
    ("reuse, S > 1600", dict(num_simulations=1601), dict(tree_reuse=True), "tree_reuse"),
    ("cap, search only", dict(manual_moves=1), CAP, "playout_cap"),
    ("cap, arena", dict(manual_moves=2), CAP, "playout_cap"),
    ("cap, K > 1", {}, dict(leaves_per_step=2, **CAP), "playout_cap"),
    ("cap, S_fast < 1", {}, dict(playout_cap=(0.25, 0)), "playout_cap"),
    ("cap, S_fast = S", {}, dict(playout_cap=(0.25, 32)), "playout_cap"),
    ("cap, p = 0", {}, dict(playout_cap=(0.0, 8)), "playout_cap"),
    ("cap, p > 1", {}, dict(playout_cap=(1.5, 8)), "playout_cap"),
    ("cap, p NaN", {}, dict(playout_cap=(NAN, 8)), "playout_cap"),
    ("forced, search only", dict(manual_moves=1), FP, "forced_playouts"),
    ("forced, arena", dict(manual_moves=2), FP, "forced_playouts"),
    ("forced, no noise", dict(add_noise=False), FP, "forced_playouts"),
    ("forced, K > 1", {}, dict(leaves_per_step=2, **FP), "forced_playouts"),
    ("forced, k NaN", {}, dict(forced_playouts=NAN), "forced_playouts"),
    ("forced, k inf", {}, dict(forced_playouts=INF), "forced_playouts"),
    ("forced, k = 0", {}, dict(forced_playouts=0.0), "forced_playouts"),
    ("forced, k > 16", {}, dict(forced_playouts=16.5), "forced_playouts"),
    ("gumbel, arena", dict(manual_moves=2), GZ, "gumbel"),
    ("gumbel + reuse", {}, dict(tree_reuse=True, **GZ), "gumbel"),
    ("gumbel + cap", {}, dict(**CAP, **GZ), "gumbel"),
    ("gumbel + forced", {}, dict(**FP, **GZ), "gumbel"),
    ("gumbel, K > 1", {}, dict(leaves_per_step=2, **GZ), "gumbel"),
    ("gumbel, m = 0", {}, dict(gumbel=(0, 50.0, 1.0)), "gumbel"),
    ("gumbel, m = 129", {}, dict(gumbel=(129, 50.0, 1.0)), "gumbel"),
    ("gumbel, c_visit NaN", {}, dict(gumbel=(16, NAN, 1.0)), "gumbel"),
    ("gumbel, c_visit beyond float32", {}, dict(gumbel=(16, 1e39, 1.0)), "gumbel"),
    ("gumbel, c_visit < 0", {}, dict(gumbel=(16, -1.0, 1.0)), "gumbel"),
    ("gumbel, c_scale = 0", {}, dict(gumbel=(16, 50.0, 0.0)), "gumbel"),
    ("gumbel, c_scale inf", {}, dict(gumbel=(16, 50.0, INF)), "gumbel"),
    ("gumbel, c_scale 0 as float32", {}, dict(gumbel=(16, 50.0, 1e-60)), "gumbel"),
    ("arena options, self-play", {}, AR, "arena_opts"),
    ("arena options, search only", dict(manual_moves=1), AR, "arena_opts"),
    ("arena options, plies < 0", dict(manual_moves=2), dict(arena_opts=(-1, 0)), "arena_opts"),
    ("arena options, plies > 16", dict(manual_moves=2), dict(arena_opts=(17, 0)), "arena_opts"),
    ("arena options, first_game < 0", dict(manual_moves=2), dict(arena_opts=(4, -2)), "arena_opts"),
    ("arena options, first_game + G beyond int32", dict(manual_moves=2), dict(arena_opts=(4, 2 ** 31 - 2)), "arena_opts"),
    ("arena options, K > 1", dict(manual_moves=2), dict(leaves_per_step=2, **AR), "arena_opts"),
    # xq_engine_init_gz refuses these on an arena engine by the option's own rule, which is the one the parser names
    ("arena options + reuse", dict(manual_moves=2), dict(tree_reuse=True, **AR), "tree_reuse"),
    ("arena options + cap", dict(manual_moves=2), dict(**CAP, **AR), "playout_cap"),
    ("arena options + forced", dict(manual_moves=2), dict(**FP, **AR), "forced_playouts"),
    ("arena options + gumbel", dict(manual_moves=2), dict(**GZ, **AR), "gumbel"),
]

# Rules only the C side can meet: the parser fills the structs itself, so a caller of it cannot set an unknown flag or a
# reserved word.  (name, K, flags, cap, forced, gumbel, arena, manual_moves)
C_ONLY = [
    ("unknown flag", 1, 2, None, None, None, None, 0),
    ("cap, reserved", 1, 0, hip.PlayoutCap(8, 1, 0.25), None, None, None, 0),
    ("forced, reserved[0]", 1, 0, None, hip.ForcedPlayouts(2.0, (1, 0)), None, None, 0),
    ("forced, reserved[1]", 1, 0, None, hip.ForcedPlayouts(2.0, (0, 1)), None, None, 0),
    ("gumbel, reserved", 1, 0, None, None, hip.Gumbel(16, 1, 50.0, 1.0), None, 0),
    ("arena options, reserved[0]", 1, 0, None, None, None, hip.ArenaOpts(4, 10, (1, 0)), 2),
    ("arena options, reserved[1]", 1, 0, None, None, None, hip.ArenaOpts(4, 10, (0, 1)), 2),
]


def _cfg(kw):
    return engine.make_config(**{**dict(n_games=4, num_simulations=32), **kw})


def raw(kw):
    """The option keywords as the C arguments (K, flags, cap, forced, gumbel, arena): raw structs, nothing checked."""
    cap, fp, gz, ar = kw.get("playout_cap"), kw.get("forced_playouts"), kw.get("gumbel"), kw.get("arena_opts")
    return (kw.get("leaves_per_step", 1), hip.ENGINE_TREE_REUSE if kw.get("tree_reuse") else 0,
            None if cap is None else hip.PlayoutCap(cap[1], 0, cap[0]), None if fp is None else hip.ForcedPlayouts(fp),
            None if gz is None else hip.Gumbel(gz[0], 0, gz[1], gz[2]), None if ar is None else hip.ArenaOpts(ar[0], ar[1]))


def _bytes_ar(lib, cfg, K, flags, *structs):
    return lib.xq_engine_workspace_bytes_ar(C.byref(cfg), K, flags, *(None if s is None else C.byref(s) for s in structs))


def _narrowest(lib, cfg, K, flags, cap, fp, gz, ar):
    """What the narrowest legacy entry point that takes these arguments returns."""
    ref = [None if s is None else C.byref(s) for s in (cap, fp, gz, ar)]
    if ar is not None:
        return lib.xq_engine_workspace_bytes_ar(C.byref(cfg), K, flags, *ref)
    if gz is not None:
        return lib.xq_engine_workspace_bytes_gz(C.byref(cfg), K, flags, *ref[:3])
    if fp is not None:
        return lib.xq_engine_workspace_bytes_fp(C.byref(cfg), K, flags, *ref[:2])
    if cap is not None:
        return lib.xq_engine_workspace_bytes_cap(C.byref(cfg), K, flags, ref[0])
    if flags:
        return lib.xq_engine_workspace_bytes_ex(C.byref(cfg), K, flags)
    if K != 1:
        return lib.xq_engine_workspace_bytes_leaves(C.byref(cfg), K)
    return lib.xq_engine_workspace_bytes(C.byref(cfg))


@pytest.fixture(scope="module")
def lib():
    hip.build()
    return hip.lib()


@pytest.mark.parametrize("name,cfg_kw,kw", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted_by_both(lib, name, cfg_kw, kw):
    cfg = _cfg(cfg_kw)
    rec = engine.parse_engine_options(cfg, **kw)
    assert isinstance(rec, engine.EngineOptions)
    want = raw(kw)
    assert (rec.K, rec.flags) == want[:2]
    for got, exp in zip(rec[2:], want[2:]):
        assert (got is None) == (exp is None) and (got is None or bytes(got) == bytes(exp))
    n = _bytes_ar(lib, cfg, *rec)
    assert n > 0
    assert n == _narrowest(lib, cfg, *want)


@pytest.mark.parametrize("name,cfg_kw,kw,option", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_both(lib, name, cfg_kw, kw, option):
    cfg = _cfg(cfg_kw)
    with pytest.raises(hip.XqError, match=option):
        engine.parse_engine_options(cfg, **kw)
    assert _bytes_ar(lib, cfg, *raw(kw)) == 0
    assert _narrowest(lib, cfg, *raw(kw)) == 0


@pytest.mark.parametrize("name,K,flags,cap,fp,gz,ar,manual", C_ONLY, ids=[c[0] for c in C_ONLY])
def test_refused_by_c_only(lib, name, K, flags, cap, fp, gz, ar, manual):
    cfg = _cfg(dict(manual_moves=manual))
    assert _bytes_ar(lib, cfg, K, flags, cap, fp, gz, ar) == 0
    zeroed = [None if s is None else type(s).from_buffer_copy(bytes(s)) for s in (cap, fp, gz, ar)]
    for s in zeroed:
        if s is not None:
            C.memset(C.byref(s, type(s).reserved.offset), 0, type(s).reserved.size)
    assert _bytes_ar(lib, cfg, K, flags & 1, *zeroed) > 0          # the same arguments without the offending word pass


def test_python_only_rules():
    """Three rules have no C counterpart in the options check, because the evaluation cache is not an argument of
    xq_engine_init_*: the cache has its own handle (xq_evcache_init), and the C side refuses the pairing where it is used
    (xq_evcache_probe on an engine with K > 1; an arena-options engine is never stepped through the cached step)."""
    with pytest.raises(hip.XqError, match="evaluation cache"):
        engine.parse_engine_options(_cfg({}), leaves_per_step=2, **CACHE)
    with pytest.raises(hip.XqError, match="arena_opts"):
        engine.parse_engine_options(_cfg(dict(manual_moves=2)), **AR, **CACHE)
    # the cached step evaluates the packed misses: an evaluator without live_rows is refused by _init_cache itself
    with pytest.raises(hip.XqError, match="live_rows"):
        engine.SelfPlayEngine._init_cache(types.SimpleNamespace(evaluator=None), 64)
