"""Host model of table adjudication (include/xq_hip.h: xq_tb_adjudicate_batch / xq_engine_adjudicate), in numpy.

`adjudicate` is the rule: boards and sides against one table (an int16 array in the layout of `endgame.index_to_board`, e.g. the
`table` of a `tests/endgame_model.py` model) -> (status, winner, value), word for word what the kernels write.  The index comes
from `endgame.board_to_index`; the status bits and the colour swap are written out here.  `engine_step` is the engine stage: which
slots the kernel looks at, what it writes into their two words, and the four counters."""
from __future__ import annotations

import numpy as np

from xiangqi_alphazero_amd import endgame

INVALID = -32768
REASON_TABLE = 5
PH_WAIT_ROOT = 2
GI_SIDE, GI_MC, GI_PHASE, GI_RSTATUS, GI_RWINNER = 0, 1, 3, 11, 12


def swap_colours(boards, sides):
    """The colour-swapped image: square i takes the negated piece of square 89 - i, and the other side is to move."""
    b = np.asarray(boards, dtype=np.int8).reshape(-1, 90)
    out = np.zeros_like(b)
    for i in range(90):
        out[:, i] = -b[:, 89 - i]
    return out, (-np.asarray(sides, dtype=np.int64).reshape(-1)).astype(np.int8)


def match_bits(signature, boards) -> np.ndarray:
    """int64[n]: +1 the board is not in this table (a piece the signature lacks, or one on a square outside its list), +2 a king is
    missing from its palace.  The r-th piece of a code in the signature takes the r-th such piece of the board in row-major order."""
    codes = endgame.parse_signature(signature)
    b = np.asarray(boards, dtype=np.int8).reshape(-1, 90)
    red = (b[:, endgame.RED_KING_SQUARES] == 1).any(axis=1)
    black = (b[:, endgame.BLACK_KING_SQUARES] == -1).any(axis=1)
    matched = np.zeros(len(b), dtype=np.int64)
    off_list = np.zeros(len(b), dtype=bool)
    for p, code in enumerate(codes):
        rank = sum(1 for q in codes[:p] if q == code)
        is_p = b == code
        hit = is_p & (np.cumsum(is_p, axis=1) == rank + 1)
        present = hit.any(axis=1)
        off_list |= present & ~np.isin(hit.argmax(axis=1), endgame.piece_squares(code))
        matched += present
    foreign = (b != 0).sum(axis=1) != matched + red + black
    return (off_list | foreign).astype(np.int64) + 2 * (~(red & black)).astype(np.int64)


def adjudicate(signature, table, boards, sides, draws: bool = True, both_colours: bool = True):
    """-> (status uint8[n], winner int8[n], value int16[n])."""
    codes = endgame.parse_signature(signature)
    table = np.asarray(table)
    assert table.dtype == np.int16 and len(table) == endgame.entries(codes)
    b = np.asarray(boards, dtype=np.int8).reshape(-1, 90)
    s = np.where(np.asarray(sides, dtype=np.int64).reshape(-1) == 1, 1, -1)
    n = len(b)
    st = match_bits(codes, b)
    idx = np.where(st == 0, endgame.board_to_index(codes, b, s), -1)
    swapped = np.zeros(n, dtype=bool)
    if both_colours:
        b2, s2 = swap_colours(b, s)
        st2 = match_bits(codes, b2)
        use = ((st & 1) != 0) & ((st2 & 1) == 0)       # the image is tried only where the board itself is "not in this table"
        st = np.where(use, st2, st)
        swapped = use & (st2 == 0)
        idx = np.where(swapped, endgame.board_to_index(codes, b2, s2), idx)
    assert ((idx >= 0) == (st == 0)).all()
    status = st.copy()
    matched = st == 0
    v = np.where(matched, table[np.maximum(idx, 0)].astype(np.int64), 0)
    invalid = matched & (v == INVALID)
    status[invalid] = 4
    read = matched & ~invalid                           # an entry's word was read and is a value
    value = np.where(read, v, 0)
    left_alone = read & (v == 0) & (not draws)
    status[left_alone] = 8
    winner = np.where(read & ~left_alone, np.sign(v) * s, 0)
    status[read & swapped] |= 16
    return status.astype(np.uint8), winner.astype(np.int8), value.astype(np.int16)


def engine_step(signature, table, boards, gi, counters, draws: bool = True, both_colours: bool = True, min_ply: int = 0):
    """One launch of the engine stage over every slot.  boards int8[G, >= 90], gi int32[G, 32] (both as read after select) and
    counters int64[G, 4] -> (gi after, counters after, why): why[s] names what the kernel did with slot s -- "phase", "status" or
    "min_ply" (left alone after its first loads), "not_covered" (status bits 1, 2 or 4), "left_alone" (a drawn entry with draws
    off), or "red", "black", "draw" (decided), with "+swapped" where the match went through the colour-swapped image."""
    gi = np.array(gi, dtype=np.int32, copy=True)
    counters = np.array(counters, dtype=np.int64, copy=True)
    why = []
    for slot in range(len(gi)):
        g = gi[slot]
        if g[GI_PHASE] != PH_WAIT_ROOT:
            why.append("phase")
        elif g[GI_RSTATUS] != 0:
            why.append("status")
        elif g[GI_MC] < min_ply:
            why.append("min_ply")
        else:
            st, w, _ = adjudicate(signature, table, np.asarray(boards)[slot, :90], [g[GI_SIDE]], draws, both_colours)
            st, w = int(st[0]), int(w[0])
            base = st & ~16
            if base == 0:
                g[GI_RSTATUS], g[GI_RWINNER] = REASON_TABLE, w
                counters[slot, 0 if w != 0 else 1] += 1
                name = {1: "red", -1: "black", 0: "draw"}[w]
            elif base == 8:
                counters[slot, 2] += 1
                name = "left_alone"
            else:
                name = "not_covered"
            if st & 16:
                counters[slot, 3] += 1
                name += "+swapped"
            why.append(name)
    return gi, counters, why
