"""Game records as training samples, on the host.  TEST INFRASTRUCTURE ONLY.

The numpy twin of xq_records_sample_counts / xq_records_to_samples (include/xq_hip.h): the same selection of plies from a record's
header, the same rows byte for byte, the same status words.  Legal moves come from the oracle, as in tests/game_record_model.py;
a move is made by moving the piece (the replay judges no rule).  It is the only source of expected bytes of the GPU tests."""
from __future__ import annotations

import numpy as np

from oracle import xq_oracle as O
from xiangqi_alphazero_amd.sample_format import GAME_RECORD_DTYPE, RECORD_MAX_PLIES, SAMPLE_DTYPE

MOVERS_ALL, MOVERS_WINNER, MOVERS_RED, MOVERS_BLACK = 0, 1, 2, 3


def selection(n_moves: int, opening_plies: int, winner: int, movers: int, skip_opening: bool, skip_draws: bool):
    """-> (selected plies in order, malformed).  A malformed record selects nothing."""
    if n_moves > RECORD_MAX_PLIES or opening_plies > n_moves or winner not in (-1, 0, 1) or movers not in (0, 1, 2, 3):
        return [], True
    if skip_draws and winner == 0:
        return [], False
    if movers == MOVERS_ALL:
        sides = (1, -1)
    elif movers == MOVERS_WINNER:
        sides = (winner,) if winner != 0 else ()
    else:
        sides = (1,) if movers == MOVERS_RED else (-1,)
    lo = opening_plies if skip_opening else 0
    return [p for p in range(lo, n_moves) if (1 if p % 2 == 0 else -1) in sides], False


def _movers_of(i: int, movers: int, per_record_movers):
    return int(movers) if per_record_movers is None else int(per_record_movers[i])


def sample_counts(records: np.ndarray, movers: int = 0, per_record_movers=None, skip_opening: bool = True,
                  skip_draws: bool = False) -> np.ndarray:
    out = np.zeros(len(records), dtype=np.int32)
    for i, r in enumerate(records):
        plies, _ = selection(int(r["n_moves"]), int(r["opening_plies"]), int(r["winner"]), _movers_of(i, movers, per_record_movers),
                             skip_opening, skip_draws)
        out[i] = len(plies)
    return out


def record_rows(r, movers: int, skip_opening: bool, skip_draws: bool):
    """One record -> (rows SAMPLE_DTYPE[count], status): status 0 whole, k + 1 when ply k is illegal (the rows of the selected
    plies from k on are zero bytes), -1 malformed (no rows)."""
    plies, malformed = selection(int(r["n_moves"]), int(r["opening_plies"]), int(r["winner"]), movers, skip_opening, skip_draws)
    if malformed:
        return np.zeros(0, dtype=SAMPLE_DTYPE), -1
    rows = np.zeros(len(plies), dtype=SAMPLE_DTYPE)
    at = {p: j for j, p in enumerate(plies)}
    board, side, winner = O.initial_board().reshape(90).copy(), 1, int(r["winner"])
    for ply in range(int(r["n_moves"])):
        action = int(r["moves"][ply])
        legal = O.legal_actions(board, side)
        hit = np.nonzero(legal == action)[0]
        if len(hit) == 0:
            return rows, ply + 1
        if ply in at:
            s = rows[at[ply]]
            s["board"], s["side"], s["ply"] = board, side, ply
            s["z"] = 0 if winner == 0 else (1 if winner == side else -1)
            s["n_moves"] = len(legal)
            s["actions"][:len(legal)] = legal
            s["visits"][int(hit[0])] = 1
            s["slot"], s["game_seq"] = r["slot"], r["game_seq"]
        frm, to = divmod(action, 90)
        board[to], board[frm] = board[frm], 0
        side = -side
    return rows, 0


def records_to_samples(records: np.ndarray, movers: int = 0, per_record_movers=None, skip_opening: bool = True,
                       skip_draws: bool = False, offsets=None, fill: int = 0xA5):
    """-> dict(samples uint8[total, 640], offsets int32[n + 1], status int32[n], counts int32[n]).  `offsets` (default: the
    exclusive prefix sum of the counts) may be wrong on purpose: a record whose gap is not its count, or whose range leaves
    [0, offsets[n]], gets status -2 and its rows keep the `fill` byte the output starts with."""
    records = np.asarray(records, dtype=GAME_RECORD_DTYPE).reshape(-1)
    n = len(records)
    counts = sample_counts(records, movers, per_record_movers, skip_opening, skip_draws)
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(counts)])
    offsets = np.asarray(offsets, dtype=np.int32)
    total = int(offsets[n])
    out = np.full((total, SAMPLE_DTYPE.itemsize), fill, dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(records):
        rows, st = record_rows(r, _movers_of(i, movers, per_record_movers), skip_opening, skip_draws)
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if st != -1 and (hi - lo != len(rows) or lo < 0 or hi > total):
            st = -2
        status[i] = st
        if st >= 0 and len(rows):
            out[lo:hi] = rows.view(np.uint8).reshape(len(rows), -1)
    return dict(samples=out, offsets=offsets, status=status, counts=counts)
