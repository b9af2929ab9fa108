"""Host model of the opt-in perpetual-check rule (include/xq_hip.h, xq_rules_opts).  TEST INFRASTRUCTURE
ONLY: it judges xq_game_over_batch_ex and the engine's terminal tests under xq_engine_init_ru.

`verdict` is is_game_over (game.py:565-616) written out in plain Python over the CPU oracle's primitives (`find_king`,
`legal_actions`, `material`, `is_in_check`), in the reference's order: king capture, no legal move, 120 no-capture plies, the
ply-200 material rule, repetition.  With the rule off it is the oracle's own `Game.is_game_over` (tests/test_perpetual_check_model.py
pins that over the corpus); the rule replaces the repetition's draw and nothing else:

    s = the side to move; entry e = the board e + 1 plies ago; E = the oldest entry of the 12-board window equal to the board;
    -s is to move in the even entries, s in the odd ones (ply parity);
    chk(-s): the side to move is in check now and in every odd entry e <= E; chk(s): in every even entry e <= E;
    exactly one holds: that side loses.

`PerpetualSearch` is the search of tests/leaf_batch_model.py (the reference's sequential search at K = 1) with that verdict at
the leaves and the one value the reference's backup cannot express: a decided leaf is worth 1 to the side that moved into it
(mcts.py:137-140), except that a leaf the rule gives to the side to move -- the mover's own check completed its perpetual -- is
worth -1 to the mover.
"""
from __future__ import annotations

import numpy as np

from leaf_batch_model import LeafBatchSearch
from oracle import xq_oracle as O

KINDS = ("not_over", "king_missing", "no_legal_move", "no_capture", "ply_200", "repetition_draw", "perpetual_check")
NOT_OVER, KING, NO_MOVE, NO_CAPTURE, PLY200, REPETITION, PERPETUAL = range(7)
HIST = 12


def perpetual_winner(board, side, entries):
    """`entries[e]` = the board e + 1 plies ago (newest first, at most 12).  -> the winner under the rule, 0 for a draw."""
    board = np.asarray(board, dtype=np.int8).reshape(90)
    same = [e for e, h in enumerate(entries) if np.array_equal(np.asarray(h, dtype=np.int8).reshape(90), board)]
    E = max(same)
    other_checks = O.is_in_check(board, side)          # every move -side made in the span gave check
    side_checks = True                                 # every move side made did
    for e in range(E + 1):
        if e % 2:
            other_checks = other_checks and O.is_in_check(entries[e], side)
        else:
            side_checks = side_checks and O.is_in_check(entries[e], -side)
    if other_checks == side_checks:
        return 0
    return side if other_checks else -side


def verdict(board, side, move_count, no_capture, hist, perpetual=False):
    """`hist`: the pre-move boards, oldest first (only the last min(12, move_count) count).  -> (kind, winner); winner 2 when
    the game is not over, as xq_game_over_batch reports it."""
    board = np.asarray(board, dtype=np.int8).reshape(90)
    side, mc = int(side), int(move_count)
    if O.find_king(board, 1) is None:
        return KING, -1
    if O.find_king(board, -1) is None:
        return KING, 1
    if len(O.legal_actions(board, side)) == 0:
        return NO_MOVE, -side
    if int(no_capture) >= 120:
        return NO_CAPTURE, 0
    if mc >= 200:
        diff = O.material(board, 1) - O.material(board, -1)
        return PLY200, (1 if diff > 30 else -1 if diff < -30 else 0)
    if mc >= 6:
        k = min(mc, HIST)
        hist = np.asarray(hist, dtype=np.int8).reshape(-1, 90)
        entries = [hist[len(hist) - 1 - e] for e in range(k)]          # newest first
        if sum(np.array_equal(h, board) for h in entries) >= 3:
            w = perpetual_winner(board, side, entries) if perpetual else 0
            return (PERPETUAL, w) if w != 0 else (REPETITION, 0)
    return NOT_OVER, 2


def game_verdict(game, perpetual=False):
    """`verdict` of an oracle `Game`."""
    return verdict(game.board, game.current_player, game.move_count, game.no_capture_count, game.history()[-HIST:], perpetual)


def is_game_over(game, perpetual=False):
    """`Game.is_game_over`'s shape: (True, winner) or (False, None)."""
    kind, winner = game_verdict(game, perpetual)
    return (True, winner) if kind != NOT_OVER else (False, None)


def terminal_value(kind, winner, side_to_move):
    """What a terminal leaf backs up, from the view of the side that moved into it."""
    if winner == 0:
        return 0.0
    return -1.0 if kind == PERPETUAL and winner == side_to_move else 1.0


class PerpetualSearch(LeafBatchSearch):
    """`LeafBatchSearch` with the rule's verdict at the leaves (`perpetual`; off: the parent class, which
    tests/test_perpetual_check_model.py pins)."""

    def __init__(self, game, num_simulations, leaves_per_step, priors, perpetual, c_puct=1.5, noise=None):
        super().__init__(game, num_simulations, leaves_per_step, priors, c_puct, noise)
        self.perpetual = bool(perpetual)

    def _terminal(self, sim, path):
        kind, winner = game_verdict(sim, self.perpetual)
        return None if kind == NOT_OVER else terminal_value(kind, winner, sim.current_player)


def search(game, num_simulations, leaves_per_step, priors, perpetual, c_puct=1.5, noise=None) -> dict:
    return PerpetualSearch(game, num_simulations, leaves_per_step, priors, perpetual, c_puct, noise).run().root()


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def _sq(r, c):
    return r * 9 + c


def _act(fr, to):
    return _sq(*fr) * 90 + _sq(*to)


def _board(pieces):
    b = np.zeros(90, dtype=np.int8)
    for (r, c), p in pieces.items():
        b[_sq(r, c)] = p
    return b


def _mirror(board):
    """Colours swapped, rows mirrored."""
    return (-np.asarray(board, dtype=np.int8).reshape(10, 9)[::-1]).reshape(90).copy()


def _mirror_action(a):
    fr, to = divmod(int(a), 90)
    m = lambda s: _sq(9 - s // 9, s % 9)
    return m(fr) * 90 + m(to)


# PC-red: red K d0, red R (8,0), black K (9,4), red to move; the rook checks on every red move of the 4-ply cycle
PC_RED_START = _board({(0, 3): 1, (8, 0): 5, (9, 4): -1})
PC_RED_CYCLE = [_act((8, 0), (9, 0)), _act((9, 4), (8, 4)), _act((9, 0), (8, 0)), _act((8, 4), (9, 4))]
# a quiet shuffle: two rooks step aside and back, no check anywhere
QUIET_START = _board({(0, 3): 1, (4, 0): 5, (9, 5): -1, (5, 8): -5})
QUIET_CYCLE = [_act((4, 0), (4, 1)), _act((5, 8), (5, 7)), _act((4, 1), (4, 0)), _act((5, 7), (5, 8))]
# mate in one for red (pins the sign of a decided leaf): rooks on (8,0) and (7,8), black K (9,4); R(7,8)->(9,8) mates
MATE_IN_ONE = _board({(0, 3): 1, (8, 0): 5, (7, 8): 5, (9, 4): -1})
MATE_MOVE = _act((7, 8), (9, 8))


def cycle_game(start, cycle, plies, player=1):
    """An oracle Game at `start` with `player` to move, advanced by `plies` plies of `cycle`."""
    g = O.Game()
    g.set_board(start, player)
    for p in range(plies):
        g.make_action(cycle[p % len(cycle)])
    return g


def pc_red(plies=12):
    return cycle_game(PC_RED_START, PC_RED_CYCLE, plies)


def pc_black(plies=12):
    return cycle_game(_mirror(PC_RED_START), [_mirror_action(a) for a in PC_RED_CYCLE], plies, player=-1)


def quiet(plies=12):
    return cycle_game(QUIET_START, QUIET_CYCLE, plies)


def state_of(game):
    """(board, side, move_count, no_capture, hist oldest first [k, 90]) of a Game."""
    return (game.board.reshape(90).copy(), game.current_player, game.move_count, game.no_capture_count, game.history()[-HIST:])


def synthetic_cases():
    """[(name, (board, side, move_count, no_capture, hist), (kind, winner) off, (kind, winner) on)]: the fixtures of the rule
    that need not be reachable positions, with the verdicts the rule's text gives them."""
    board, side, mc, nc, hist = state_of(pc_red(12))
    entry = lambda e: 11 - e                           # row of entry e in the oldest-first history of 12 boards
    out = []
    # both kings in check on every board: both sides "checked throughout" -> draw
    both = _board({(0, 3): 1, (5, 3): -5, (9, 5): -1, (4, 5): 5})
    out.append(("both_check", (both, 1, 12, 12, np.tile(both, (12, 1))), (REPETITION, 0), (REPETITION, 0)))
    # one quiet move among red's six checking ones (entry 4: the rook stands off the king's row) -> draw
    h = hist.copy()
    h[entry(4)] = _board({(0, 3): 1, (7, 0): 5, (9, 4): -1})
    out.append(("one_quiet_move", (board, side, mc, nc, h), (REPETITION, 0), (REPETITION, 0)))
    # a span shorter than the window: entries 1, 3, 7 equal the board, the four oldest differ (an extra pawn), E = 7; the
    # quiet board among e > E does not count -> still red's loss
    h = hist.copy()
    h[entry(1)] = board
    for e in (8, 9, 10, 11):
        h[entry(e)] = h[entry(e)].copy()
        h[entry(e)][_sq(3, 8)] = 7
    h[entry(10)] = _board({(0, 3): 1, (7, 0): 5, (9, 4): -1, (3, 8): 7})
    out.append(("short_span", (board, side, mc, nc, h), (REPETITION, 0), (PERPETUAL, -1)))
    # the same with the quiet board inside the span (entry 6 <= E) -> draw
    h = h.copy()
    h[entry(6)] = _board({(0, 3): 1, (7, 0): 5, (9, 4): -1})
    out.append(("short_span_quiet_inside", (board, side, mc, nc, h), (REPETITION, 0), (REPETITION, 0)))
    # earlier rules keep their verdict on a repeating position: ply 200 (red is a rook up), 120 no-capture plies
    out.append(("ply_200", (board, side, 200, nc, hist), (PLY200, 1), (PLY200, 1)))
    out.append(("no_capture", (board, side, mc, 120, hist), (NO_CAPTURE, 0), (NO_CAPTURE, 0)))
    return out


def uniform_priors(state, legal):
    """The stub of the leaf tests: uniform policy (1/8100 per action, dense probabilities), value 0."""
    p = np.full(len(legal), np.float32(1.0 / 8100.0), dtype=np.float32)
    s = np.float32(0.0)
    for x in p:
        s = np.float32(s + x)
    return (p / s).astype(np.float32), 0, 0.0


def pc_red_rotated(plies=12):
    """PC-red one ply on: black moves first, so red's checking move completes every repetition and, at ply 12, its own
    perpetual -- the verdict names the side to move (black) the winner."""
    start = _board({(0, 3): 1, (9, 0): 5, (9, 4): -1})
    return cycle_game(start, PC_RED_CYCLE[1:] + PC_RED_CYCLE[:1], plies, player=-1)
