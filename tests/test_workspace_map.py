"""CPU checks of the option words' map (include/xq_hip.h: THE OPTION WORDS, xq_engine_option_words_sp) over the grid of
tests/workspace_grid.py: the workspace sizes recorded from the parent of the commit that introduced the map
(tests/golden/workspace_bytes.json), the map succeeding exactly where a size is returned, every block inside the region, the blocks
pairwise disjoint and aligned, and the offsets equal to the formulas the Python layer computed by hand until the map existed."""
import ctypes as C
import json

import pytest

import workspace_grid as grid

SCALARS = ("table", "gz_head", "gz_vhat", "gz_visits", "ar_head", "ar_op_counts", "ar_op_actions", "ar_n_live", "solver",
           "gr_ring", "gr_log", "gr_opening", "gr_head", "sp_rows", "sp_index", "sp_head")
PAIRS = ("ar_rows", "ar_x", "ar_moves", "ar_counts")
ALIGN_256 = {"solver", "gr_ring", "gr_log", "gr_opening", "gr_head", "sp_rows", "sp_index", "sp_head"}     # and every ar_* block


def up256(n):
    return (n + 255) & ~255


@pytest.fixture(scope="module")
def lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


@pytest.fixture(scope="module")
def recorded():
    fix = json.load(open(grid.FIXTURE))
    assert fix["fields"] == list(grid.FIELDS) + ["bytes"] and fix["calls"] == len(grid.cases()) == 5832
    sizes = {tuple(row[:-1]): row[-1] for row in fix["accepted"]}
    # 378 accepted shapes; with the 0 of the refused ones, 284 distinct return values
    assert len(sizes) == len(fix["accepted"]) == 378 and len(set(sizes.values())) == 283 and min(sizes.values()) > 0
    return sizes


def option_words(lib, case):
    """-> (return code, {block name: (offset, bytes)} of the blocks the engine has, region bytes)"""
    from xiangqi_alphazero_amd import hip
    args, keep = grid.arguments(case)
    w = hip.OptionWords()
    rc = lib.xq_engine_option_words_sp(*args, C.byref(w))
    blocks = {n: (getattr(w, n).offset, getattr(w, n).bytes) for n in SCALARS}
    blocks.update({f"{n}[{i}]": (getattr(w, n)[i].offset, getattr(w, n)[i].bytes) for n in PAIRS for i in range(2)})
    return rc, {n: b for n, b in blocks.items() if b[1]}, int(w.bytes)


def test_every_workspace_size_is_the_recorded_one(lib, recorded):
    for case in grid.cases():
        assert grid.workspace_bytes(lib, case) == recorded.get(case, 0), dict(zip(grid.FIELDS, case))


def test_the_map_succeeds_exactly_where_a_size_is_returned(lib, recorded):
    from xiangqi_alphazero_amd import hip
    for case in grid.cases():
        rc, blocks, _ = option_words(lib, case)
        assert rc == (0 if case in recorded else -1), dict(zip(grid.FIELDS, case))
    args, keep = grid.arguments(next(iter(recorded)))
    assert lib.xq_engine_option_words_sp(*args, None) == -1
    assert C.sizeof(hip.OptionWords) == 8 + 24 * 16 and C.sizeof(hip.WordsBlock) == 16


def test_the_sixteen_accepted_shapes(lib, recorded):
    """Which options share the region, as sets of what an accepted case has beyond the table."""
    shapes = set()
    for (G, S, mm, K, m, arena, solver, M, n) in recorded:
        shapes.add(tuple(name for name, on in (("K > 1", K > 1), ("gumbel", m), ("arena", arena), ("solver", solver),
                                               ("records", M), ("pool", n)) if on))
    assert shapes == {(), ("K > 1",), ("pool",), ("K > 1", "pool"), ("records",), ("K > 1", "records"), ("solver",),
                      ("solver", "pool"), ("solver", "records"), ("arena",), ("arena", "records"), ("arena", "solver"),
                      ("arena", "solver", "records"), ("gumbel",), ("gumbel", "pool"), ("gumbel", "records")}


def test_blocks_lie_inside_the_region_disjoint_and_aligned(lib, recorded):
    for case in recorded:
        G, S, mm, K, m, arena, solver, M, n = case
        rc, blocks, region = option_words(lib, case)
        what = dict(zip(grid.FIELDS, case))
        want = {"table"} | ({"gz_head", "gz_vhat", "gz_visits"} if m else set()) | ({"solver"} if solver else set()) | \
               ({"gr_ring", "gr_log", "gr_opening", "gr_head"} if M else set()) | ({"sp_rows", "sp_index", "sp_head"} if n else set()) | \
               ({"ar_head", "ar_op_counts", "ar_op_actions", "ar_n_live"} | {f"{p}[{i}]" for p in PAIRS for i in range(2)} if arena
                else set())
        assert set(blocks) == want, what
        spans = sorted((off, off + size, name) for name, (off, size) in blocks.items())
        assert spans[0][0] == 0 and spans[-1][1] <= region, what
        for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
            assert a1 <= b0, (an, bn, what)
        for name, (off, size) in blocks.items():
            assert off % (256 if name in ALIGN_256 or name.startswith("ar_") else 8) == 0, (name, what)
        # the workspace holds the region whole: the region that follows it starts at its end, rounded up
        assert region > 0 and (region % 256 == 0 if (M or n) else True), what


def test_offsets_are_the_formulas_python_used(lib, recorded):
    """SelfPlayEngine.gumbel_root_values and game_record_views computed these by hand before they read the map."""
    seen = set()
    for case in recorded:
        G, S, mm, K, m, arena, solver, M, n = case
        rc, blocks, end = option_words(lib, case)
        what = dict(zip(grid.FIELDS, case))
        assert blocks["table"] == (0, (S + 2 + (K if K > 1 else 0)) * 8), what
        if m:
            assert blocks["gz_head"] == ((S + 2) * 8, 16) and blocks["gz_vhat"] == ((S + 2) * 8 + 16, G * 8), what
            assert blocks["gz_visits"] == ((S + 2) * 8 + 16 + G * 8, m * S * 2), what
            seen.add("gumbel")
        if M:
            head = end - 256
            opening = head - up256(2 * G)
            log = opening - up256(1008 * G)
            ring = log - 1024 * M
            assert blocks["gr_head"] == (head, 256) and blocks["gr_opening"] == (opening, 2 * G), what
            assert blocks["gr_log"] == (log, 1008 * G) and blocks["gr_ring"] == (ring, 1024 * M), what
            seen.add("records")
        if n:
            head = end - 256
            index = head - up256(4 * G)
            assert blocks["sp_head"] == (head, 256) and blocks["sp_index"] == (index, 4 * G), what
            assert blocks["sp_rows"] == (index - up256(96 * n), 96 * n), what
            seen.add("pool")
    assert seen == {"gumbel", "records", "pool"}
