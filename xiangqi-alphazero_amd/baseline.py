"""A fixed, non-learning opponent and the match against it -- the absolute yardstick of a training run.

The arena gate compares one network with another, so every verdict is relative to the previous best.  The baseline is a
fixed-depth minimax player over the material evaluation (`hip.alphabeta_batch`, include/xq_hip.h: xq_alphabeta_batch): depth 0
plays uniformly random legal moves, depth d >= 1 searches d plies and breaks ties between equally good moves by a seeded draw.

`play_vs_baseline` is a host-driven match built from pieces that exist: a game's state is its record (`GAME_RECORD_DTYPE`);
every ply `engine.replay_games` gives the board, side, counts, 12-board history and the rules' verdict of all games at once, the
network's moves come from one search-only `MCTS` (`search_many`) and the baseline's from one `alphabeta_batch` call.  Game g is
slot g; the network is red in even games; games 2p and 2p + 1 share an opening of uniformly random legal plies (the arena's
pairing), so the pair is the sample (`arena.pair_statistics`)."""
from __future__ import annotations

import time
from typing import Dict

import numpy as np
import torch

from . import arena, engine, hip
from .mcts import as_mcts, solver_choice
from .sample_format import GAME_RECORD_DTYPE

MAX_DEPTH = hip.AB_MAX_DEPTH
MATE = hip.AB_MATE
UNSCORED = hip.AB_UNSCORED
NO_MOVE = hip.AB_NO_MOVE
MAX_OPENING = hip.ARENA_MAX_OPENING


def pick(scores, count: int, draw=None):
    """xq_alphabeta_batch's pick rule on the host: over scores[:count], the index of the (draw mod ties)-th of the moves that
    reach the largest score, in move order (the first of them when `draw` is None), and that score.  (None, None) when count
    is 0."""
    count = int(count)
    if count <= 0:
        return None, None
    s = np.asarray(scores).reshape(-1)[:count].astype(np.int64)
    best = int(s.max())
    ties = np.nonzero(s == best)[0]
    k = 0 if draw is None else int(draw) % len(ties)
    return int(ties[k]), best


class _Position:
    """One replayed game as `MCTS.search_many` takes it."""

    def __init__(self, board, side, move_count, no_capture, hist12):
        self.board = board
        self.current_player = int(side)
        self.move_count = int(move_count)
        self.no_capture_count = int(no_capture)
        k = min(12, self.move_count)
        self.history = [hist12[e].tobytes() for e in range(k)]


def _replay(records, perpetual_check, device) -> Dict[str, torch.Tensor]:
    st = engine.replay_games(records, perpetual_check=perpetual_check, device=device)
    if bool((st["status"] != 0).any().item()):
        raise hip.XqError("play_vs_baseline: a game's own record does not replay")
    return st


def _append(records, g: int, action: int) -> None:
    n = int(records["n_moves"][g])
    records["moves"][g, n] = action
    records["n_moves"][g] = n + 1


def _play_openings(records, plies: int, rng, perpetual_check, device) -> None:
    """`plies` uniformly random legal plies per pair, the same in both of its games.  A pair whose opening ends the game restarts
    without one (the arena's rule)."""
    n = len(records)
    pairs = n // 2
    live = np.ones(pairs, dtype=bool)
    for _ in range(plies):
        st = _replay(records, perpetual_check, device)
        moves, counts, _, _ = hip.movegen(st["board"], st["side"])
        moves, counts = moves.cpu().numpy().view(np.uint16), counts.cpu().numpy().astype(np.int64)
        over = st["over_kind"].cpu().numpy()
        for p in range(pairs):
            if not live[p]:
                continue
            if over[2 * p] != 0 or counts[2 * p] == 0:
                live[p] = False
                continue
            a = int(moves[2 * p, int(rng.integers(counts[2 * p]))])
            _append(records, 2 * p, a)
            _append(records, 2 * p + 1, a)
    over = _replay(records, perpetual_check, device)["over_kind"].cpu().numpy()
    for p in range(pairs):
        if live[p] and over[2 * p] == 0:
            records["opening_plies"][2 * p:2 * p + 2] = plies
        else:
            records["moves"][2 * p:2 * p + 2] = 0
            records["n_moves"][2 * p:2 * p + 2] = 0


def play_vs_baseline(model_or_evaluator, num_games: int, depth: int, num_simulations: int, opening_plies: int = 4, seed: int = 0,
                     max_game_length: int = 200, c_puct: float = 1.5, perpetual_check: bool = False, solver: bool = False,
                     device="cuda", evaluator_kind: str = "hip") -> Dict[str, object]:
    """A match of `num_games` (even) games between a network and the baseline of `depth` (module docstring).  The network moves
    as in the arena: `num_simulations` simulations without noise, the first maximum of the visit counts in move order, or
    `solver_choice` with `solver=True`.  The baseline takes one draw per game and ply from `np.random.default_rng(seed)`, the
    generator of the openings, in game order: the same seed gives the same match.  A game not over at `max_game_length` plies is
    a draw with reason 2; one the rules decide has reason 1, or 4 for a perpetual-check loss.
    `model_or_evaluator` may be an integer depth instead: then both sides are baseline players, that depth in the network's seat,
    and `num_simulations` is ignored.
    It may also be an `MCTS` the caller built: the match searches with it, under its simulations and options.  One built with
    `early_stop=True` ends a search as soon as its first choice is fixed: the same match, sooner.
    Returns `wins, losses, draws, win_rate` from the network's view, `pairs, win_rate_se, win_rate_ci95`
    (`arena.pair_statistics`), `game_records` (GAME_RECORD_DTYPE, slot = game), `baseline_nodes` (positions the baseline visited),
    `baseline_draws` (int64 [moves, 3]: game, ply and draw of every baseline move, so a move can be recomputed) and `seconds`."""
    t0 = time.time()
    num_games, depth, opening_plies = int(num_games), int(depth), int(opening_plies)
    ladder = isinstance(model_or_evaluator, (int, np.integer)) and not isinstance(model_or_evaluator, bool)
    if num_games <= 0 or num_games % 2:
        raise hip.XqError(f"play_vs_baseline: num_games must be positive and even (games come in colour-swapped pairs), got {num_games}")
    if not 0 <= depth <= MAX_DEPTH or (ladder and not 0 <= int(model_or_evaluator) <= MAX_DEPTH):
        raise hip.XqError(f"play_vs_baseline: a baseline's depth must be in [0, {MAX_DEPTH}]")
    if not 0 <= opening_plies <= MAX_OPENING:
        raise hip.XqError(f"play_vs_baseline: opening_plies must be in [0, {MAX_OPENING}], got {opening_plies}")
    if not 1 <= int(max_game_length) <= hip.RECORD_MAX_PLIES:
        raise hip.XqError(f"play_vs_baseline: max_game_length must be in [1, {hip.RECORD_MAX_PLIES}], got {max_game_length}")
    dev = torch.device(device)
    rng = np.random.default_rng(int(seed))
    records = np.zeros(num_games, dtype=GAME_RECORD_DTYPE)
    records["slot"] = np.arange(num_games)
    records["winner"] = 2
    mcts = None
    if not ladder:
        mcts = as_mcts(model_or_evaluator, int(num_simulations), c_puct, device, evaluator_kind, seed=int(seed),
                       perpetual_check=perpetual_check, solver=solver)
        solver = mcts.solver
    seats = (num_games + 1) // 2
    nodes = 0
    drawn = []                                             # (game, ply, draw) of every baseline move
    with torch.cuda.device(dev):
        if opening_plies > 0:
            _play_openings(records, opening_plies, rng, perpetual_check, dev)
        net_red = np.arange(num_games) % 2 == 0
        live = np.ones(num_games, dtype=bool)
        pad = None
        while live.any():
            st = _replay(records, perpetual_check, dev)
            over, winner = st["over_kind"].cpu().numpy(), st["winner"].cpu().numpy()
            side, mc = st["side"].cpu().numpy(), st["move_count"].cpu().numpy()
            for g in np.nonzero(live)[0]:
                if over[g] != 0:
                    records["winner"][g], records["reason"][g] = winner[g], 4 if over[g] == 4 else 1
                    live[g] = False
                elif mc[g] >= int(max_game_length):
                    records["winner"][g], records["reason"][g] = 0, 2
                    live[g] = False
            idx = np.nonzero(live)[0]
            if len(idx) == 0:
                break
            net_moves = (side[idx] == 1) == net_red[idx]
            if pad is None:
                pad = _replay(np.zeros(1, dtype=GAME_RECORD_DTYPE), perpetual_check, dev)
                pad = _Position(pad["board"].cpu().numpy()[0], 1, 0, 0, np.zeros((12, 90), dtype=np.int8))
            # the seats that search: one game of every pair has the network to move (both games of a pair advance a ply per turn)
            if not ladder and net_moves.any():
                boards, nocap, hist = st["board"].cpu().numpy(), st["no_capture"].cpu().numpy(), st["hist12"].cpu().numpy()
                mine = idx[net_moves]
                if len(mine) > seats:
                    raise hip.XqError("play_vs_baseline: more searching games than seats")
                games = [_Position(boards[g], side[g], mc[g], nocap[g], hist[g]) for g in mine]
                eng = mcts.search_decided(games + [pad] * (seats - len(games)))
                for slot, g in enumerate(mine):
                    r = eng.read_root(slot)
                    if len(r["actions"]) == 0:
                        raise hip.XqError("play_vs_baseline: a running game has no legal move")
                    if solver:
                        a = solver_choice(r["actions"], r["visits"], eng.read_root_states(slot)["children"])
                    else:
                        a = int(r["actions"][int(np.argmax(r["visits"]))])
                    _append(records, g, a)
            # the baseline's seats: one call per depth over the games in which it is to move, one draw per game in game order
            theirs = idx if ladder else idx[~net_moves]
            if len(theirs):
                draws = rng.integers(0, 2 ** 32, size=len(theirs), dtype=np.uint64)
                depths = np.where(net_moves, int(model_or_evaluator), depth) if ladder else np.full(len(theirs), depth)
                for d in sorted(set(depths.tolist())):
                    sel = np.nonzero(depths == d)[0]
                    rows = torch.from_numpy(theirs[sel].astype(np.int64)).to(dev)
                    out = hip.alphabeta_batch(st["board"].index_select(0, rows).contiguous(),
                                              st["side"].index_select(0, rows).contiguous(), int(d), draws[sel])
                    if bool((out["status"] != 0).any().item()):
                        raise hip.XqError("play_vs_baseline: the baseline's search reported a capacity error")
                    nodes += int(out["nodes"].to(torch.int64).sum().item())
                    best = out["best_action"].cpu().numpy().view(np.uint16)
                    for g, a, u in zip(theirs[sel], best, draws[sel]):
                        drawn.append((int(g), int(mc[g]), int(u)))
                        if int(a) == NO_MOVE:
                            raise hip.XqError("play_vs_baseline: a running game has no legal move")
                        _append(records, g, int(a))
    w = records["winner"].astype(np.int64)
    net_won = np.where(net_red, w == 1, w == -1)
    wins, draws_ = int(net_won.sum()), int((w == 0).sum())
    ps = arena.pair_statistics(w)
    return {"depth": depth, "games": num_games, "wins": wins, "losses": num_games - wins - draws_, "draws": draws_,
            "win_rate": (wins + 0.5 * draws_) / num_games, "pairs": ps["pairs"], "win_rate_se": ps["win_rate_se"],
            "win_rate_ci95": ps["win_rate_ci95"], "game_records": records, "baseline_nodes": nodes,
            "baseline_draws": np.array(drawn, dtype=np.int64).reshape(-1, 3), "seconds": time.time() - t0}
