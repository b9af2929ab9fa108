"""Host models of the start-position pool.  TEST INFRASTRUCTURE ONLY.

`check_position(board, side)`: the status bits of xq_positions_check_batch (include/xq_hip.h) in plain Python over the oracle's
`is_in_check` and `has_legal_moves`.
`play_game_from(cfg, peaked, draws, board, side)`: the plain loop of tests/selfplay_model.py (no option) on
`O.Game().set_board(board, side)`: no opening and no `randint` draw; move count, no-capture count and history start empty, so
every ply counter counts from the given position.
"""
from __future__ import annotations

import numpy as np

import leaf_batch_model as LB
import tree_reuse_model as M
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key

FATAL, NO_MOVE = 15, 16

_ADVISOR = {(0, 3), (0, 5), (1, 4), (2, 3), (2, 5)}
_ELEPHANT = {(0, 2), (0, 6), (2, 0), (2, 4), (2, 8), (4, 2), (4, 6)}


def _may_stand(kind: int, colour: int, r: int, c: int) -> bool:
    rr = r if colour == 1 else 9 - r                   # the row as red sees it: black is red mirrored
    if kind == 2:
        return (rr, c) in _ADVISOR
    if kind == 3:
        return (rr, c) in _ELEPHANT
    if kind == 7:
        return rr >= 5 or (rr >= 3 and c % 2 == 0)
    return True


def check_position(board, side) -> int:
    b = np.asarray(board, dtype=np.int64).reshape(10, 9)
    st = 0
    if (b < -7).any() or (b > 7).any() or int(side) not in (1, -1):
        st |= 1
    for colour in (1, -1):
        at = np.argwhere(b == colour)
        rows = (0, 1, 2) if colour == 1 else (7, 8, 9)
        if len(at) != 1 or int(at[0][0]) not in rows or not 3 <= int(at[0][1]) <= 5:
            st |= 2
    if st:
        return st                                      # the rules are not run on such a board
    bad = False
    for r in range(10):
        for c in range(9):
            p = int(b[r, c])
            if abs(p) >= 2 and not _may_stand(abs(p), 1 if p > 0 else -1, r, c):
                bad = True
    for kind in range(2, 8):
        most = 5 if kind == 7 else 2
        bad = bad or int((b == kind).sum()) > most or int((b == -kind).sum()) > most
    if bad:
        st |= 4
    if O.is_in_check(b, -int(side)):
        st |= 8
    if not O.has_legal_moves(b, int(side)):
        st |= 16
    return st


def play_game_from(cfg: dict, peaked: bool, draws, board, side):
    """One self-play game from (board, side) on `draws` (a Draws, or a seed) -> (samples, winner, plies): selfplay_model.play_game
    with every option off, without its opening."""
    d = Draws(draws) if isinstance(draws, int) else draws
    priors = LB.stub_priors(peaked)
    S, c_puct = int(cfg["num_simulations"]), float(cfg["c_puct"])
    g = O.Game()
    g.set_board(board, side)
    samples, resign_hist = [], []
    while True:
        over, w = g.is_game_over()
        if over:
            winner = w
            break
        if g.move_count >= int(cfg["max_game_length"]):
            diff = O.material(g.board, 1) - O.material(g.board, -1)
            winner = 1 if diff > 30 else (-1 if diff < -30 else 0)
            break
        late = g.move_count >= int(cfg["temperature_threshold"])
        s = M.ReuseSearch(g, S, priors, d.dirichlet(len(g.legal_actions())), None, c_puct, budget=S)
        s.run()
        visits, i, _ = s.move_end({})
        r = s.root()
        samples.append(dict(board=g.board.reshape(90).copy(), player=g.current_player, actions=r["actions"].copy(),
                            visits=visits.copy(), late=late))
        if i is None:
            i = M.choose(r["actions"], visits, late, d.uniform())
        g.make_action(int(r["actions"][i]))
        if cfg["enable_resign"] and len(samples) > 10:
            _, v = predict_from_key(state_key(g.state_for_nn()), peaked)
            resign_hist.append(v)
            K = int(cfg["resign_check_steps"])
            if len(resign_hist) >= K and all(x < float(cfg["resign_threshold"]) for x in resign_hist[-K:]):
                winner = -g.current_player
                break
    for smp in samples:
        smp["z"] = 0 if winner == 0 else (1 if winner == smp["player"] else -1)
    return samples, winner, g.move_count
