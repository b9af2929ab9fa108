"""CPU model of the fixed alpha-beta opponent (include/xq_hip.h, xq_alphabeta_batch): the PLAIN minimax of the header over the
oracle's `legal_actions`, with no pruning, and the pick rule.  The kernels and `baseline.pick` are checked against it word for
word; `alphabeta_root` is the pruned search the kernel runs, kept here so the CPU suite can show that it gives the same scores."""
from __future__ import annotations

import numpy as np

from oracle import xq_oracle as O

MAX_DEPTH = 4
MATE = 30000
UNSCORED = -2 ** 31
NO_MOVE = 0xFFFF
MAXM = 128
VALUE = {0: 0, 1: 0, 2: 20, 3: 20, 4: 40, 5: 90, 6: 45, 7: 10}
_SIGNED = np.array([-VALUE[-p] if p < 0 else VALUE[p] for p in range(-7, 8)], dtype=np.int64)      # red minus black, by piece + 7


def balance(board, side: int) -> int:
    """material(side) - material(other) with the reference's piece values (the king counts 0)."""
    return side * int(_SIGNED[np.asarray(board, dtype=np.int64).reshape(90) + 7].sum())


def child(board, action: int) -> np.ndarray:
    b = np.array(board, dtype=np.int8).reshape(90)
    f, t = int(action) // 90, int(action) % 90
    b[t] = b[f]
    b[f] = 0
    return b


def value(board, side: int, d: int, ply: int, count=None) -> int:
    """V(pos, d, ply) from the view of `side`, to move in `board`; `count` (a one-entry list) counts the positions visited."""
    if count is not None:
        count[0] += 1
    if d == 0:
        return balance(board, side)
    acts = O.legal_actions(board, side)
    if len(acts) == 0:
        return -(MATE - ply)
    return max(-value(child(board, a), -side, d - 1, ply + 1, count) for a in acts)


def kings_stand(board) -> bool:
    b = np.asarray(board).reshape(10, 9)
    return bool((b[0:3, 3:6] == 1).any() and (b[7:10, 3:6] == -1).any())


def pick(scores, count: int, draw=None):
    """-> (best_action index, best_score) over scores[:count]: the draw-th (mod the number of ties) of the moves that reach the
    largest score, in move order; the first of them without a draw; (None, None) for an empty list."""
    if count == 0:
        return None, None
    s = [int(x) for x in scores[:count]]
    best = max(s)
    ties = [j for j, x in enumerate(s) if x == best]
    return ties[(int(draw) % len(ties)) if draw is not None else 0], best


def search(board, side: int, depth: int, draw=None) -> dict:
    """Every output of xq_alphabeta_batch for one position, by plain minimax."""
    assert 0 <= depth <= MAX_DEPTH
    out = {"moves": np.zeros(MAXM, dtype=np.uint16), "count": 0, "scores": np.full(MAXM, UNSCORED, dtype=np.int64),
           "nodes": np.zeros(MAXM, dtype=np.int64), "best_action": NO_MOVE, "best_score": 0, "status": 0}
    if not kings_stand(board):
        out["status"] = 2
        return out
    acts = O.legal_actions(board, side)
    n = len(acts)
    out["count"] = n
    out["moves"][:n] = acts
    if n == 0:
        out["best_score"] = -MATE
        return out
    for j, a in enumerate(acts):
        if depth == 0:
            out["scores"][j] = 0
        else:
            c = [0]
            out["scores"][j] = -value(child(board, a), -side, depth - 1, 1, c)
            out["nodes"][j] = c[0]
    j, best = pick(out["scores"], n, draw)
    out["best_action"], out["best_score"] = int(acts[j]), best
    return out


# ---- the pruned search the kernel runs -----------------------------------------------------------------------------------------

INF = 1 << 30


def _ab(board, side: int, d: int, ply: int, alpha: int, beta: int, count) -> int:
    """Fail-soft alpha-beta in move order, d >= 1; the level whose children are leaves (d == 1) scores all of them at once: a
    leaf's balance is the parent's plus the value of what the move captures."""
    count[0] += 1
    acts = O.legal_actions(board, side)
    if len(acts) == 0:
        return -(MATE - ply)
    if d == 1:
        count[0] += len(acts)
        b = np.asarray(board).reshape(90)
        return balance(board, side) + max(VALUE[abs(int(b[int(a) % 90]))] for a in acts)
    best = -INF
    for a in acts:
        v = -_ab(child(board, a), -side, d - 1, ply + 1, -beta, -max(alpha, best), count)
        best = max(best, v)
        if best >= beta:
            break
    return best


def alphabeta_root(board, side: int, depth: int):
    """-> (scores, nodes) of every root move, each searched on its own under a full window (depth >= 1)."""
    acts = O.legal_actions(board, side)
    scores, nodes = [], []
    b = np.asarray(board).reshape(90)
    for a in acts:
        if depth == 1:
            scores.append(balance(board, side) + VALUE[abs(int(b[int(a) % 90]))])
            nodes.append(1)
        else:
            c = [0]
            scores.append(-_ab(child(board, a), -side, depth - 1, 1, -INF, INF, c))
            nodes.append(c[0])
    return scores, nodes
