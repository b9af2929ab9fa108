"""The host model of table adjudication (tests/adjudicate_model.py) against the model tables of tests/endgame_model.py: the colour
swap is proven on the CPU before any kernel relies on it.  No GPU."""
import numpy as np
import pytest

import adjudicate_model as AM
import endgame_model as EM
from xiangqi_alphazero_amd import endgame

INITIAL = np.array([[5, 4, 3, 2, 1, 2, 3, 4, 5], [0] * 9, [0, 6, 0, 0, 0, 0, 0, 6, 0], [7, 0, 7, 0, 7, 0, 7, 0, 7], [0] * 9,
                    [0] * 9, [-7, 0, -7, 0, -7, 0, -7, 0, -7], [0, -6, 0, 0, 0, 0, 0, -6, 0], [0] * 9,
                    [-5, -4, -3, -2, -1, -2, -3, -4, -5]], dtype=np.int8).reshape(90)


def off_table_boards():
    """Three boards no "Ra" table covers: an extra pawn, the initial position, and a board without the black king."""
    foreign = np.zeros(90, dtype=np.int8)
    foreign[4], foreign[85], foreign[40], foreign[84], foreign[49] = 1, -1, 5, -2, 7
    kingless = np.zeros(90, dtype=np.int8)
    kingless[4], kingless[40], kingless[84] = 1, 5, -2
    return np.stack([foreign, INITIAL, kingless]), np.array([1, 1, -1], dtype=np.int8)


@pytest.mark.parametrize("signature,swapped_signature", [("Ra", "rA"), ("Nb", "nB")])
@pytest.mark.parametrize("draws", [True, False])
def test_swapped_board_reads_the_swapped_table(signature, swapped_signature, draws):
    """Every entry's board, colours swapped, adjudicated by the table of `signature`: the verdict is the one read directly from the
    model table of the swapped signature."""
    m, ms = EM.model(signature), EM.model(swapped_signature)
    boards, sides = endgame.index_to_board(signature, np.arange(m.entries))
    b2, s2 = AM.swap_colours(boards, sides)
    status, winner, value = AM.adjudicate(signature, m.table, b2, s2, draws=draws, both_colours=True)
    direct = endgame.board_to_index(swapped_signature, b2, s2)
    v = np.where(direct >= 0, ms.table[np.maximum(direct, 0)].astype(np.int64), EM.INVALID)
    covered = (direct >= 0) & (v != EM.INVALID)
    base = status & 0xEF
    assert covered.sum() > m.entries // 2
    assert ((base[~covered] & 7) != 0).all() and (winner[~covered] == 0).all() and (value[~covered] == 0).all()
    assert (value[covered] == v[covered]).all()
    want_base = np.where((v == 0) & (not draws), 8, 0)
    assert (base[covered] == want_base[covered]).all()
    decided = covered & (base == 0)
    assert (winner[decided] == np.sign(v[decided]) * s2[decided]).all() and (winner[~decided] == 0).all()
    # a board that still holds one of the two pieces is in the table through the image only; bare kings match directly
    men = (b2 != 0).sum(axis=1)
    assert ((status[covered & (men > 2)] & 16) == 16).all() and ((status[covered & (men == 2)] & 16) == 0).all()
    # and with both_colours off none of those is in the table
    off = AM.adjudicate(signature, m.table, b2[men > 2], s2[men > 2], draws=draws, both_colours=False)
    assert ((off[0] & 1) == 1).all() and (off[1] == 0).all() and (off[2] == 0).all()


def test_own_boards_read_their_own_entries():
    m = EM.model("Ra")
    idx = np.arange(m.entries)
    boards, sides, collide = endgame.index_to_board("Ra", idx, return_collisions=True)
    status, winner, value = AM.adjudicate("Ra", m.table, boards, sides, draws=True, both_colours=True)
    t = m.table.astype(np.int64)
    valid = ~collide & (t != EM.INVALID)
    assert (status[valid] == 0).all() and (value[valid] == t[valid]).all()
    assert (winner[valid] == np.sign(t[valid]) * sides[valid]).all()
    assert (status[~collide & (t == EM.INVALID)] == 4).all()


def test_drawn_entries_with_draws_off():
    m = EM.model("Ra")
    drawn = np.nonzero(m.table == 0)[0]
    assert len(drawn) > 100
    boards, sides = endgame.index_to_board("Ra", drawn)
    status, winner, value = AM.adjudicate("Ra", m.table, boards, sides, draws=False)
    assert (status == 8).all() and (winner == 0).all() and (value == 0).all()
    status, winner, value = AM.adjudicate("Ra", m.table, boards, sides, draws=True)
    assert (status == 0).all() and (winner == 0).all()


@pytest.mark.parametrize("both_colours", [True, False])
def test_off_table_boards(both_colours):
    m = EM.model("Ra")
    boards, sides = off_table_boards()
    status, winner, value = AM.adjudicate("Ra", m.table, boards, sides, both_colours=both_colours)
    assert list(status) == [1, 1, 2] and not winner.any() and not value.any()


def test_symmetric_signature_never_matches_through_the_image():
    """A signature that is its own colour swap: a board the image matches is matched directly.  Bit 16 is a matter of matching alone,
    so a table of draws stands in for the real one."""
    table = np.zeros(endgame.entries("Pp"), dtype=np.int16)
    idx = np.arange(0, len(table), 7)
    boards, sides = endgame.index_to_board("Pp", idx)
    b2, s2 = AM.swap_colours(boards, sides)
    for b, s in ((boards, sides), (b2, s2)):
        status, _, _ = AM.adjudicate("Pp", table, b, s, both_colours=True)
        assert not (status & 16).any() and (status == 0).sum() > len(idx) // 2


def test_engine_step_gates():
    """The engine stage's three early exits, its two stores and its counters, on hand-made state words."""
    m = EM.model("Ra")
    won = int(np.nonzero(m.table[:m.entries // 2] > 0)[0][0])
    board, side = endgame.index_to_board("Ra", [won])
    boards = np.repeat(np.pad(board, ((0, 0), (0, 6))), 5, axis=0)
    gi = np.zeros((5, 32), dtype=np.int32)
    gi[:, AM.GI_SIDE], gi[:, AM.GI_PHASE], gi[:, AM.GI_MC] = side[0], AM.PH_WAIT_ROOT, 3
    gi[1, AM.GI_PHASE] = 3
    gi[2, AM.GI_RSTATUS], gi[2, AM.GI_RWINNER] = 1, -1
    gi[3, AM.GI_MC] = 1
    boards[4], gi[4, AM.GI_SIDE] = np.pad(AM.swap_colours(board, side)[0][0], (0, 6)), -side[0]
    after, counters, why = AM.engine_step("Ra", m.table, boards, gi, np.zeros((5, 4), dtype=np.int64), min_ply=2)
    assert why == ["red", "phase", "status", "min_ply", "black+swapped"]
    assert list(after[:, AM.GI_RSTATUS]) == [5, 0, 1, 0, 5] and list(after[:, AM.GI_RWINNER]) == [1, 0, -1, 0, -1]
    changed = after != gi
    changed[:, [AM.GI_RSTATUS, AM.GI_RWINNER]] = False
    assert not changed.any()
    assert counters.tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1]]
