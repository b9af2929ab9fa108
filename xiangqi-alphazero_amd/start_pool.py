"""Pools of start positions for `SelfPlayEngine(start_pool=(boards, sides, prob))`.

Every source returns `(boards int8[n, 90], sides int8[n])` on the host, duplicates kept: an entry that stands twice in the pool is
drawn twice as often, which is the caller's tool for weighting (concatenate, repeat).  The engine checks what it is given
(`hip.positions_check`); nothing here does.

    from_fens     FEN lines or a file of them, as the tactics yardstick's puzzle file is read
    from_table    entries of an endgame table (`Tablebase.entries_of`)
    from_records  one seeded ply of every drawn game record, through the device replay
    index_of      the engine's draw on the host: which entry a slot's game starts from
"""
from __future__ import annotations

import os

import numpy as np

from . import hip
from .sample_format import board_from_fen


def from_fens(lines_or_path):
    """One FEN per line (`sample_format.board_from_fen`); blank lines and lines that start with '#' are skipped.  `lines_or_path`:
    the path of such a file, its text, or an iterable of lines.  A malformed line raises ValueError naming it."""
    if isinstance(lines_or_path, (str, os.PathLike)) and "\n" not in str(lines_or_path) and os.path.exists(lines_or_path):
        with open(lines_or_path) as f:
            lines = f.read().splitlines()
    elif isinstance(lines_or_path, str):
        lines = lines_or_path.splitlines()
    else:
        lines = [str(x) for x in lines_or_path]
    rows = [board_from_fen(line) for line in lines if line.strip() and not line.lstrip().startswith("#")]
    boards = np.zeros((len(rows), 90), dtype=np.int8)
    sides = np.zeros(len(rows), dtype=np.int8)
    for i, (b, s) in enumerate(rows):
        boards[i], sides[i] = b, s
    return boards, sides


def from_table(tb, n: int, kinds=("win",), seed: int = 0, min_plies: int = 0):
    """`n` entries of the endgame table `tb` (an `endgame.Tablebase`) whose kind for the side to move is in `kinds` ("win",
    "draw", "loss"), a seeded draw without replacement among the entries one can move from; `min_plies` keeps wins and losses of
    at least that many plies.  Fewer than n such entries: XqError (`Tablebase.entries_of`)."""
    boards, sides, _ = tb.entries_of(kinds, n, seed, min_plies=min_plies)
    return np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 90), np.ascontiguousarray(sides, dtype=np.int8)


def from_records(records, n: int, seed: int = 0, min_ply: int = 0, max_ply: int = 200, perpetual_check: bool = False,
                 device="cuda"):
    """Positions out of recorded games (hip.GAME_RECORD_DTYPE, as `drain_games` returns): `n` seeded draws of a record, with
    replacement, and for each a seeded ply in [min_ply, min(max_ply, n_moves)], replayed on the device (`engine.replay_games`).
    Left out: a record shorter than min_ply, one that does not replay to its ply, and a position where the game is over (under
    the perpetual-check rule with `perpetual_check`).  So at most n positions come back.  The move count, the no-capture count and
    the history of the game do not come along: a pool game starts at ply 0."""
    from . import engine
    rec = np.ascontiguousarray(records)
    if rec.dtype != hip.GAME_RECORD_DTYPE:
        raise hip.XqError(f"from_records: records must have hip.GAME_RECORD_DTYPE, got {rec.dtype}")
    if isinstance(n, bool) or int(n) != n or int(n) < 0 or not 0 <= int(min_ply) <= int(max_ply):
        raise hip.XqError(f"from_records: n >= 0 and 0 <= min_ply <= max_ply required, got {n!r}, {min_ply!r}, {max_ply!r}")
    rec = rec.reshape(-1)
    rng = np.random.default_rng(int(seed))
    if len(rec) == 0 or int(n) == 0:
        return np.zeros((0, 90), dtype=np.int8), np.zeros(0, dtype=np.int8)
    pick = rng.integers(0, len(rec), size=int(n))
    hi = np.minimum(rec["n_moves"][pick].astype(np.int64), int(max_ply))
    long_enough = hi >= int(min_ply)
    ply = (int(min_ply) + np.floor(rng.random(int(n)) * (np.maximum(hi - int(min_ply), 0) + 1))).astype(np.int32)
    pick, ply = pick[long_enough], np.minimum(ply, hi)[long_enough].astype(np.int32)
    if len(pick) == 0:
        return np.zeros((0, 90), dtype=np.int8), np.zeros(0, dtype=np.int8)
    out = engine.replay_games(rec[pick], stop_ply=ply, perpetual_check=perpetual_check, device=device)
    keep = ((out["status"] == 0) & (out["over_kind"] == 0)).cpu().numpy()
    boards = out["board"].cpu().numpy().reshape(-1, 90)[keep]
    sides = out["side"].cpu().numpy()[keep]
    return np.ascontiguousarray(boards, dtype=np.int8), np.ascontiguousarray(sides, dtype=np.int8)


def index_of(seed: int, rank: int, slot: int, game_seq: int, n: int, prob: float) -> int:
    """The engine's draw on the host (`hip.start_pool_index`, the device's own code; no GPU needed): the entry of a pool of `n`
    that the game `game_seq` (1 for a slot's first game) of `slot` on `rank` starts from under `seed` and `prob`, or -1 for the
    initial position."""
    return hip.start_pool_index(seed, rank, slot, game_seq, n, prob)
