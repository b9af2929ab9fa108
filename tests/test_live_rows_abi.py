"""CPU-side checks of the packed step's C ABI (include/xq_hip.h: xq_engine_compact / xq_engine_packed /
xq_engine_expand_packed and the *_live evaluator kernels): argument conventions, the stats struct, header <-> EXPORTS."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = ["xq_stem_conv_live", "xq_heads_1x1_live", "xq_wino_conv3x3_live", "xq_wino_conv3x3_bf16_live",
        "xq_policy_head_legal_live", "xq_value_head_live"]
ENGINE = ["xq_engine_compact", "xq_engine_packed", "xq_engine_expand_packed"]


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


def _live_call(lib, name, capacity, dev_n, ptr=None):
    """One call of a *_live entry point with every other pointer = `ptr` (None: null), stream null."""
    if name == "xq_stem_conv_live":
        return lib.xq_stem_conv_live(ptr, ptr, ptr, ptr, capacity, dev_n, 128, None)
    if name == "xq_heads_1x1_live":
        return lib.xq_heads_1x1_live(ptr, ptr, ptr, ptr, ptr, capacity * 90, dev_n, 128, None)
    if name == "xq_wino_conv3x3_live":
        return lib.xq_wino_conv3x3_live(ptr, ptr, ptr, None, ptr, capacity, dev_n, 128, 1, None)
    if name == "xq_wino_conv3x3_bf16_live":
        return lib.xq_wino_conv3x3_bf16_live(ptr, ptr, ptr, None, ptr, capacity, dev_n, 128, 1, None)
    if name == "xq_policy_head_legal_live":
        return lib.xq_policy_head_legal_live(ptr, ptr, ptr, ptr, ptr, capacity, dev_n, ptr, None)
    if name == "xq_value_head_live":
        return lib.xq_value_head_live(ptr, ptr, ptr, ptr, ptr, capacity, dev_n, ptr, None)
    raise AssertionError(name)


def test_live_entry_points_argument_conventions():
    lib = _lib()
    n = ctypes.c_int32(3)                       # never dereferenced: every call below returns before any launch
    np_ = ctypes.addressof(n)
    for name in LIVE:
        assert _live_call(lib, name, 4, None) == -1, name             # null pointers (dev_n included)
        assert _live_call(lib, name, 4, np_) == -1, name               # null data pointers, count present
        assert _live_call(lib, name, -1, np_) == -1, name              # negative capacity
        assert _live_call(lib, name, -1, None) == -1, name
        assert _live_call(lib, name, 0, None) == 0, name               # capacity 0: a no-op, like an empty batch
        assert _live_call(lib, name, 0, np_) == 0, name
    # misaligned (odd) addresses are refused like the plain twins do
    assert lib.xq_wino_conv3x3_live(1, 1, 1, None, 3, 4, np_, 128, 1, None) == -1
    assert lib.xq_heads_1x1_live(None, None, None, None, None, 91, np_, 128, None) == -1   # rows must be whole positions


def test_engine_packed_entry_points_reject_null():
    from xiangqi_alphazero_amd import hip
    lib = _lib()
    assert lib.xq_engine_compact(None, None, None) == -1
    assert lib.xq_engine_packed(None, None) == -1
    assert lib.xq_engine_expand_packed(None, None, None, None) == -1
    pb = hip.PackedBuffers()
    assert lib.xq_engine_packed(None, ctypes.byref(pb)) == -1


def test_stats_struct_keeps_its_size_and_gains_rows_evaluated():
    from xiangqi_alphazero_amd import hip
    assert ctypes.sizeof(hip.EngineStats) == 256
    assert hip.EngineStats.rows_evaluated.offset == 18 * 8          # the first of the formerly reserved words
    assert "rows_evaluated" in hip.EngineStats().as_dict()
    text = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct xq_engine_stats \{(.*?)\} xq_engine_stats;", text, re.S).group(1),
                  flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("uint64_t", "").split(",")]
    words = sum(int(re.search(r"\[(\d+)\]", n).group(1)) if "[" in n else 1 for n in names)
    assert words == 32 and names[18] == "rows_evaluated" and names[-1] == "reserved[13]"


def test_header_and_exports_list_the_new_symbols():
    from xiangqi_alphazero_amd import hip
    lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xq_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z_0-9]+)\s*\(", text))
    for name in LIVE + ENGINE:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert sorted(hip.EXPORTS) == sorted(declared)


def test_workspace_holds_the_packed_buffers():
    from xiangqi_alphazero_amd import engine
    lib = _lib()
    small = lib.xq_engine_workspace_bytes(ctypes.byref(engine.make_config(1, 1)))
    big = lib.xq_engine_workspace_bytes(ctypes.byref(engine.make_config(1025, 1)))
    # per slot at least: planes 5400 B, moves 256, row map / count / value 12, slot-ordered logits 512
    assert big - small >= 1024 * (5400 + 256 + 12 + 512)
