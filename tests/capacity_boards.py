"""Crafted positions around the move list's capacity (XQ_MAXM = 128 of csrc/xq_rules.cuh), shared by
tests/test_capacity_edges.py (their move counts, on the CPU oracle) and tests/test_capacity_edges_gpu.py.

`rook_board(k)`: red king (0,4), black king (9,3), k red rooks on rows 1..k, one per column in the order ROOK_COLS, so no rook
stands in another's way: red has 121 / 139 / 152 legal moves for k = 7 / 8 / 9 and is not in check, black has one legal move.
The boards at the capacity are the k = 8 board plus ONE red advisor outside its palace: there it has no move of its own
(xq_rules.cuh gen_task, game_core.pyx:307-326) and only shortens the rooks' rays, which gives exactly 127, 128 and 129.

Every board here has at most 200 legal moves, the oracle's unchecked buffer (oracle/xq_oracle.py MAX_MOVES).
"""
from __future__ import annotations

import numpy as np

ROOK_COLS = (0, 1, 2, 5, 6, 7, 8, 3, 4)
ROOK_COUNTS = {7: 121, 8: 139, 9: 152}            # k -> red's legal moves
BLOCKER = {127: (7, 3), 128: (6, 3), 129: (5, 3)}   # red's legal moves -> square of the red advisor added to rook_board(8)
MAXM = 128


def rook_board(k: int) -> np.ndarray:
    b = np.zeros((10, 9), dtype=np.int8)
    b[0, 4], b[9, 3] = 1, -1
    for i in range(k):
        b[1 + i, ROOK_COLS[i]] = 5
    return b


def edge_board(n_moves: int) -> np.ndarray:
    """Red to move with exactly `n_moves` legal moves: 127, 128, 129 (one blocker), 121, 139, 152 (rooks only)."""
    for k, n in ROOK_COUNTS.items():
        if n == n_moves:
            return rook_board(k)
    b = rook_board(8)
    r, c = BLOCKER[n_moves]
    assert b[r, c] == 0
    b[r, c] = 2
    return b


ALL_COUNTS = (121, 127, 128, 129, 139, 152)


def board_from_planes(state: np.ndarray):
    """(board int8[90], side) back from the 15 input planes (game.py:618-640): planes 0-6 the mover's pieces, 7-13 the other
    side's, plane 14 all ones when red is to move."""
    s = np.asarray(state, dtype=np.float32).reshape(15, 90)
    side = 1 if s[14, 0] == 1.0 else -1
    b = np.zeros(90, dtype=np.int8)
    for i in range(1, 8):
        b[s[i - 1] == 1.0] = i * side
        b[s[6 + i] == 1.0] = -i * side
    return b, side
