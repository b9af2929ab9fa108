"""CPU model of the endgame tablebases (include/xq_hip.h, xq_tb_*): the header's definitions over the oracle's `legal_actions` and
`is_in_check`.  The oracle is called once per entry to build a padded matrix of child indices; the value iteration itself is numpy
over that matrix, every pass reading the table of the pass before (the kernels work in place; the header argues that it is the
same).  `endgame.index_to_board` gives the layout, and only that: the child indices are worked out here, digit by digit.  The
kernels are checked against `table` word for word and against `probe` output for output."""
from __future__ import annotations

import functools

import numpy as np

from oracle import xq_oracle as O
from xiangqi_alphazero_amd import endgame

INVALID = -32768
NO_MOVE = 0xFFFF
MAXM = 128


class Model:
    """signature -> table int16[entries], passes, children int64[entries, width] (-1 past the count), counts, moves."""

    def __init__(self, signature):
        self.codes = endgame.parse_signature(signature)
        self.radix = endgame.radices(self.codes)
        self.entries = endgame.entries(self.codes)
        self.stride = [0] * len(self.radix)
        unit = 1
        for j in range(len(self.radix) - 1, -1, -1):
            self.stride[j] = unit
            unit *= self.radix[j]
        self._squares = [endgame.RED_KING_SQUARES, endgame.BLACK_KING_SQUARES] + [endgame.piece_squares(c) for c in self.codes]
        self._digit_of = [{int(s): d for d, s in enumerate(sq)} for sq in self._squares]
        self._expand()
        self._iterate()

    def _expand(self):
        n = self.entries
        boards, sides, collide = endgame.index_to_board(self.codes, np.arange(n), return_collisions=True)
        digits = endgame.index_to_digits(self.codes, np.arange(n))
        self.boards, self.sides = boards, sides
        table = np.zeros(n, dtype=np.int16)
        kids, acts_of = [None] * n, [None] * n
        width = 1
        nmen = len(self._squares)
        for e in range(n):
            if collide[e]:
                table[e] = INVALID
                continue
            b, s = boards[e], int(sides[e])
            if O.is_in_check(b, -s):
                table[e] = INVALID
                continue
            acts = O.legal_actions(b, s)
            if len(acts) == 0:
                table[e] = -1
                continue
            d = digits[e]
            at = {}
            for m in range(nmen):
                if d[1 + m] < len(self._squares[m]):
                    at[int(self._squares[m][d[1 + m]])] = m
            flip = self.stride[0] if s == 1 else -self.stride[0]
            row = []
            for a in acts.tolist():
                f, t = divmod(a, 90)
                m = at[f]
                c = e + flip + (self._digit_of[m][t] - int(d[1 + m])) * self.stride[1 + m]
                if t in at:
                    q = at[t]
                    assert q >= 2, "a king was captured"
                    c += (len(self._squares[q]) - int(d[1 + q])) * self.stride[1 + q]
                row.append(c)
            kids[e], acts_of[e] = row, acts
            width = max(width, len(row))
        self.children = np.full((n, width), -1, dtype=np.int64)
        self.moves = np.zeros((n, MAXM), dtype=np.uint16)
        self.counts = np.zeros(n, dtype=np.int64)
        for e in range(n):
            if kids[e] is not None:
                k = len(kids[e])
                self.children[e, :k] = kids[e]
                self.moves[e, :k] = acts_of[e]
                self.counts[e] = k
        self.table = table

    def _iterate(self):
        t = self.table
        rows = np.nonzero((t == 0) & (self.counts > 0))[0]
        k = 0
        while True:
            k += 1
            assert k <= 32000
            ch = self.children[rows]
            live = ch >= 0
            cv = np.where(live, t[np.maximum(ch, 0)].astype(np.int64), 0)
            if k & 1:
                hit = ((cv == -k) & live).any(axis=1)
                new = k
            else:
                hit = ((cv > 0) | ~live).all(axis=1) & (cv.max(axis=1) == k - 1)
                new = -(k + 1)
            if not hit.any():
                break
            t[rows[hit]] = new
            rows = rows[~hit]
        self.passes = k

    # ---- what the table says of its own entries ---------------------------------------------------------------
    def move_values(self) -> np.ndarray:
        """int64[entries, width]: what the side to move gets by every move (0 past the count)."""
        live = self.children >= 0
        cv = np.where(live, self.table[np.maximum(self.children, 0)].astype(np.int64), 0)
        return np.where(cv < 0, -cv, np.where(cv > 0, -(cv + 2), 0))

    def stats(self) -> dict:
        half = self.entries // 2
        out = {}
        for name, t in (("red", self.table[:half]), ("black", self.table[half:])):
            out[name] = (int((t == INVALID).sum()), int((t > 0).sum()), int(((t < 0) & (t != INVALID)).sum()), int((t == 0).sum()))
        out["longest_win"] = max(int(self.table.max()), 0)
        out["passes"] = self.passes
        return out

    def probe(self, rows=None) -> dict:
        """Every output of xq_tb_probe_batch for the entries `rows` (all of them by default), probed as their own boards."""
        rows = np.arange(self.entries) if rows is None else np.asarray(rows, dtype=np.int64)
        t = self.table[rows].astype(np.int64)
        bad = t == INVALID
        n = len(rows)
        counts = np.where(bad, 0, self.counts[rows])
        moves = np.where(bad[:, None], 0, self.moves[rows]).astype(np.uint16)
        mv = np.zeros((n, MAXM), dtype=np.int64)
        width = self.children.shape[1]
        mv[:, :width] = np.where(bad[:, None], 0, self.move_values()[rows])
        value = np.where(bad, 0, t)
        live = np.arange(MAXM)[None, :] < counts[:, None]
        eq = live & (mv == value[:, None])
        best = np.where(eq.any(axis=1), moves[np.arange(n), eq.argmax(axis=1)], NO_MOVE)
        return {"value": value, "moves": moves, "counts": counts, "move_value": mv, "best_action": best,
                "status": np.where(bad, 4, 0)}


@functools.lru_cache(maxsize=None)
def model(signature: str) -> Model:
    return Model(signature)


def best_of(move_values) -> int:
    """The value of a position with these move values: the quickest win, else a draw, else the slowest loss."""
    mv = [int(v) for v in move_values]
    wins = [v for v in mv if v > 0]
    if wins:
        return min(wins)
    return 0 if 0 in mv else min(mv)
