"""A tactics yardstick: forced-mate puzzles labelled on the device, and how many of them a search solves.

The arena gate is relative and the alpha-beta baseline positional; neither says whether a network plus S simulations sees a
forced mate in two.  A puzzle is a position in which the side to move forces mate within N of its own moves
(`hip.mate_search_batch`, include/xq_hip.h: xq_mate_search_batch), by checks only (the classic puzzle) or by any move.  A puzzle
file is text, one FEN per line (`sample_format.board_to_fen`): it holds positions and no labels.  The labels always come from the
device (`label`), so a file can be scored under any N.

`solve_rate` runs one search-only `MCTS` over the puzzles (`search_many`: move count 0, no history, no noise) and asks the labels
about the move the search chose: any move that still forces mate within N solves the puzzle, one that mates as quickly as the
best move is optimal."""
from __future__ import annotations

import time
from typing import Dict

import numpy as np
import torch

from . import hip
from .sample_format import SAMPLE_DTYPE, board_from_fen, board_to_fen, position_key

MAX_MOVES = hip.MATE_MAX_MOVES
UNKNOWN = hip.MATE_UNKNOWN
NO_MOVE = hip.MATE_NO_MOVE

PUZZLE_DTYPE = np.dtype([("board", np.int8, 90), ("side", np.int8), ("mate_in", np.uint8), ("status", np.uint8),
                         ("n_moves", np.uint8), ("best_action", np.uint16), ("moves", np.uint16, hip.MAXM),
                         ("move_mate_in", np.uint8, hip.MAXM)])


class _Position:
    """One puzzle as `MCTS.search_many` takes it: the start of a game, nothing behind it."""

    def __init__(self, board, side):
        self.board = board
        self.current_player = int(side)
        self.move_count = 0
        self.no_capture_count = 0
        self.history = []


def _positions(boards, sides):
    """-> (int8[n, 90], int8[n]) from boards and sides, or from samples (SAMPLE_DTYPE) with sides None."""
    if isinstance(boards, np.ndarray) and boards.dtype == SAMPLE_DTYPE:
        s = boards.reshape(-1)
        return np.ascontiguousarray(s["board"]), np.ascontiguousarray(s["side"])
    if sides is None:
        raise hip.XqError("tactics: sides is None and boards are no samples (SAMPLE_DTYPE)")
    b = np.ascontiguousarray(np.asarray(boards, dtype=np.int8)).reshape(-1, 90)
    s = np.ascontiguousarray(np.asarray(sides, dtype=np.int8)).reshape(-1)
    if len(b) != len(s):
        raise hip.XqError(f"tactics: {len(b)} boards and {len(s)} sides")
    return b, s


def label(boards, sides=None, max_moves: int = 3, checks_only: bool = True, node_limit=None, device="cuda") -> np.ndarray:
    """One mate-search call over every position -> puzzles (PUZZLE_DTYPE), one per position in order: mate_in is the best
    mate-in (0: none within max_moves), move_mate_in the label of every root move (UNKNOWN: cut by the node limit), status the
    call's status byte."""
    b, s = _positions(boards, sides)
    out = np.zeros(len(b), dtype=PUZZLE_DTYPE)
    out["board"], out["side"] = b, s
    if len(b) == 0:
        hip.mate_search_batch(torch.zeros((0, 90), dtype=torch.int8), torch.zeros(0, dtype=torch.int8), max_moves, checks_only,
                              node_limit)            # the argument checks
        return out
    dev = torch.device(device)
    with torch.cuda.device(dev):
        r = hip.mate_search_batch(torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), max_moves, checks_only, node_limit)
        r = {k: v.cpu().numpy() for k, v in r.items()}
    out["mate_in"], out["status"], out["n_moves"] = r["best_mate_in"], r["status"], r["counts"]
    out["best_action"], out["moves"], out["move_mate_in"] = r["best_action"].view(np.uint16), r["moves"].view(np.uint16), r["mate_in"]
    return out


def select(puzzles: np.ndarray, max_moves: int, min_moves: int = 2, unique: bool = True) -> np.ndarray:
    """The labelled positions whose best mate-in is in [min_moves, max_moves]; with `unique` one per `position_key` (mirror
    images merged), the first occurrence."""
    keep = []
    seen = set()
    for i in np.nonzero((puzzles["mate_in"] >= int(min_moves)) & (puzzles["mate_in"] <= int(max_moves)))[0]:
        if unique:
            key = (position_key(puzzles["board"][i], int(puzzles["side"][i]), mirror=True)[0], int(puzzles["side"][i]))
            if key in seen:
                continue
            seen.add(key)
        keep.append(int(i))
    return puzzles[keep]


def find_puzzles(boards, sides=None, max_moves: int = 3, min_moves: int = 2, checks_only: bool = True, node_limit=None,
                 unique: bool = True, device="cuda") -> np.ndarray:
    """`label`, then `select`: the positions (boards and sides, or samples of SAMPLE_DTYPE) in which the side to move forces mate
    in min_moves .. max_moves of its own moves."""
    if isinstance(min_moves, bool) or int(min_moves) != min_moves or not 1 <= int(min_moves) <= MAX_MOVES:
        raise hip.XqError(f"find_puzzles: min_moves must be an integer in [1, {MAX_MOVES}], got {min_moves!r}")
    return select(label(boards, sides, max_moves, checks_only, node_limit, device), max_moves, min_moves, unique)


def puzzles_to_text(puzzles: np.ndarray, header=()) -> str:
    """One FEN per line; `header` lines go first behind '# '.  Labels are not written."""
    lines = ["# " + h for h in header]
    lines += [board_to_fen(p["board"], int(p["side"])) for p in np.asarray(puzzles).reshape(-1)]
    return "".join(line + "\n" for line in lines)


def puzzles_from_text(text: str) -> np.ndarray:
    """The positions of a puzzle file (PUZZLE_DTYPE with board and side set and no labels); blank lines and lines starting with
    '#' are skipped."""
    rows = [board_from_fen(line) for line in text.splitlines() if line.strip() and not line.lstrip().startswith("#")]
    out = np.zeros(len(rows), dtype=PUZZLE_DTYPE)
    for i, (b, s) in enumerate(rows):
        out["board"][i], out["side"][i] = b, s
    return out


def move_label(puzzle, action: int) -> int:
    """The mate-in of root move `action` of a labelled puzzle (0 when it is no root move)."""
    n = int(puzzle["n_moves"])
    at = np.nonzero(puzzle["moves"][:n] == int(action))[0]
    return int(puzzle["move_mate_in"][at[0]]) if len(at) else 0


def solve_rate(model_or_evaluator, puzzles, num_simulations: int, c_puct: float = 1.5, solver: bool = False,
               perpetual_check: bool = False, seed: int = 0, device="cuda", evaluator_kind: str = "hip",
               chunk: int = 256) -> Dict[str, object]:
    """How many labelled puzzles a search of `num_simulations` simulations solves (module docstring).  The move is the first
    maximum of the visits in move order, or `solver_choice` under `solver`.  Solved: the chosen move's label is a mate-in (1..N
    of the labelling; 0 and UNKNOWN are not); optimal: it equals the puzzle's best.  -> puzzles, solved, optimal, solve_rate,
    by_mate_in {m: [count, solved]}, simulations, seconds, chosen (the action per puzzle).  `model_or_evaluator` may be an `MCTS`
    the caller built: the pass searches with it, under its simulations and options; one built with `early_stop=True` ends a search
    as soon as its first choice is fixed: the same moves, sooner."""
    from .mcts import as_mcts, solver_choice
    t0 = time.time()
    puzzles = np.asarray(puzzles).reshape(-1)
    if puzzles.dtype != PUZZLE_DTYPE:
        raise hip.XqError(f"solve_rate: puzzles must be PUZZLE_DTYPE (tactics.label), got {puzzles.dtype}")
    if int(num_simulations) < 1:
        raise hip.XqError(f"solve_rate: num_simulations must be >= 1, got {num_simulations}")
    if int(chunk) < 1:
        raise hip.XqError(f"solve_rate: chunk must be >= 1, got {chunk}")
    n = len(puzzles)
    if n and bool(((puzzles["mate_in"] < 1) | (puzzles["mate_in"] > MAX_MOVES)).any()):
        raise hip.XqError("solve_rate: every puzzle needs a best mate-in in 1..%d (label the positions first)" % MAX_MOVES)
    chosen = np.zeros(n, dtype=np.int64)
    if n:
        mcts = as_mcts(model_or_evaluator, int(num_simulations), c_puct, device, evaluator_kind, seed=int(seed),
                       perpetual_check=perpetual_check, solver=solver)
        solver = mcts.solver
        width = min(int(chunk), n)
        with torch.cuda.device(torch.device(device)):
            for base in range(0, n, width):
                part = puzzles[base:base + width]
                games = [_Position(p["board"], p["side"]) for p in part]
                eng = mcts.search_decided(games + [games[0]] * (width - len(games)))
                for slot in range(len(part)):
                    r = eng.read_root(slot)
                    if len(r["actions"]) == 0:
                        raise hip.XqError("solve_rate: a puzzle has no legal move")
                    if solver:
                        chosen[base + slot] = solver_choice(r["actions"], r["visits"], eng.read_root_states(slot)["children"])
                    else:
                        chosen[base + slot] = int(r["actions"][int(np.argmax(r["visits"]))])
    return {**score(puzzles, chosen), "simulations": int(num_simulations), "seconds": time.time() - t0, "chosen": chosen}


def score(puzzles: np.ndarray, chosen) -> Dict[str, object]:
    """What the labels say of one chosen action per puzzle: puzzles, solved, optimal, solve_rate and by_mate_in."""
    n = len(puzzles)
    got = np.array([move_label(p, a) for p, a in zip(puzzles, chosen)], dtype=np.int64)
    ok = (got >= 1) & (got <= MAX_MOVES)
    best = puzzles["mate_in"].astype(np.int64)
    by = {int(m): [int((best == m).sum()), int((ok & (best == m)).sum())] for m in sorted(set(best.tolist()))}
    return {"puzzles": n, "solved": int(ok.sum()), "optimal": int((got == best).sum()),
            "solve_rate": float(ok.sum()) / n if n else 0.0, "by_mate_in": by}
