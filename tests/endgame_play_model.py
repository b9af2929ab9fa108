"""CPU model of the table as opponent and teacher (include/xq_hip.h, xq_tb_play_batch / xq_tb_samples), on top of
`endgame_model.Model`: its `children`, `moves`, `counts`, `table` and `move_values()`.  Entries are played as their own boards.
`play` gives every output of xq_tb_play_batch, `sample_rows` every byte of xq_tb_samples, and `walk` plays the table against
itself.  Everything is integers; the kernels are compared to it exactly."""
from __future__ import annotations

import functools

import numpy as np

import endgame_model as EM
from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE

INVALID, NO_MOVE, MAXM = EM.INVALID, EM.NO_MOVE, EM.MAXM


def apply_move(board, action):
    """The host's apply: `to` takes the man of `from`, `from` becomes empty."""
    f, t = divmod(int(action), 90)
    out = np.array(board, dtype=np.int8).reshape(90).copy()
    out[t] = out[f]
    out[f] = 0
    return out


class PlayModel:
    def __init__(self, signature):
        self.m = EM.model(signature)
        self.mv = self.m.move_values()
        # the table's own move per entry, over the whole table at once: the first move whose value is the entry's; -1 where the
        # entry is invalid or has no move
        m = self.m
        live = m.children >= 0
        first = (live & (self.mv == m.table.astype(np.int64)[:, None])).argmax(axis=1)
        self.best_child = np.where((m.counts > 0) & (m.table != INVALID), m.children[np.arange(m.entries), first], -1)

    def optimal(self, e):
        """bool[count]: the moves of a valid entry whose value equals the entry's."""
        k = int(self.m.counts[e])
        return self.mv[e, :k] == int(self.m.table[e])

    def play(self, rows, actions=None) -> dict:
        """Every output of xq_tb_play_batch for the entries `rows`; actions None (or NO_MOVE per row): the table chooses."""
        m = self.m
        rows = np.asarray(rows, dtype=np.int64)
        n = len(rows)
        out = {"boards": m.boards[rows].copy(), "side": m.sides[rows].copy(), "played": np.full(n, NO_MOVE, dtype=np.int64),
               "value": np.zeros(n, dtype=np.int64), "move_value": np.zeros(n, dtype=np.int64),
               "value_out": np.zeros(n, dtype=np.int64), "status": np.zeros(n, dtype=np.int64),
               "child": np.full(n, -1, dtype=np.int64)}
        for i, e in enumerate(rows.tolist()):
            t = int(m.table[e])
            if t == INVALID:
                out["status"][i] = 4
                continue
            out["value"][i] = t
            k = int(m.counts[e])
            if k == 0:
                out["status"][i] = 8
                continue
            want = NO_MOVE if actions is None else int(actions[i])
            hits = np.nonzero(self.optimal(e) if want == NO_MOVE else m.moves[e, :k] == want)[0]
            if len(hits) == 0:
                out["status"][i] = 16
                continue
            j = int(hits[0])
            c = int(m.children[e, j])
            out["boards"][i] = apply_move(m.boards[e], m.moves[e, j])
            out["side"][i] = -m.sides[e]
            out["played"][i] = int(m.moves[e, j])
            out["move_value"][i] = int(self.mv[e, j])
            out["value_out"][i] = int(m.table[c])
            out["child"][i] = c
        return out

    def sample_rows(self, rows, policy):
        """-> (SAMPLE_DTYPE[n], status int64[n]): what xq_tb_samples writes for the indices `rows` (any integers)."""
        m = self.m
        rows = np.asarray(rows, dtype=np.int64)
        out = np.zeros(len(rows), dtype=SAMPLE_DTYPE)
        status = np.zeros(len(rows), dtype=np.int64)
        for i, e in enumerate(rows.tolist()):
            if not 0 <= e < m.entries:
                status[i] = 1
                continue
            t = int(m.table[e])
            k = int(m.counts[e])
            if t == INVALID or k == 0:
                status[i] = 4 if t == INVALID else 8
                continue
            r = out[i]
            r["board"], r["side"], r["z"] = m.boards[e], m.sides[e], (t > 0) - (t < 0)
            r["n_moves"], r["game_seq"] = k, e
            r["actions"][:k] = m.moves[e, :k]
            best = self.optimal(e)
            if policy == 1:
                first = int(np.argmax(best))
                best = np.arange(k) == first
            r["visits"][:k] = best
        return out, status

    def walk_all(self, rows):
        """The table against itself from every entry of `rows` at once -> (plies int64[n], values: one int64[n] per step, the
        entries' values before each ply and after the last; a finished game repeats its last value)."""
        m = self.m
        at = np.asarray(rows, dtype=np.int64).copy()
        plies = np.zeros(len(at), dtype=np.int64)
        values = [m.table[at].astype(np.int64)]
        while (self.best_child[at] >= 0).any():
            go = self.best_child[at] >= 0
            at = np.where(go, self.best_child[at], at)
            plies += go
            values.append(m.table[at].astype(np.int64))
            assert len(values) <= 4096
        return plies, values

    def walk(self, e):
        """The table against itself from entry e -> the list of (entry, value) visited, the last one an entry without a move."""
        m = self.m
        path = [(int(e), int(m.table[e]))]
        while m.counts[path[-1][0]] > 0:
            r = self.play([path[-1][0]])
            assert r["status"][0] == 0
            path.append((int(r["child"][0]), int(r["value_out"][0])))
            assert len(path) <= 4096
        return path


@functools.lru_cache(maxsize=None)
def play_model(signature: str) -> PlayModel:
    return PlayModel(signature)
