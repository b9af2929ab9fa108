"""What a game record must hold, from the host models.  TEST INFRASTRUCTURE ONLY.

`expected_record` plays one game of `selfplay_model.play_game` and returns the move list the engine's record of that game must
carry: the opening plies are read off the game's history at the first `on_move` call (differences of consecutive pre-move boards,
the last one against the board itself), every later move is the one `on_move` reports.  selfplay_model.py is not touched; the list
is pinned against the oracle by replaying it on a fresh `oracle.Game` (tests/test_game_records_model.py)."""
from __future__ import annotations

import numpy as np

import selfplay_model as SP
from oracle import xq_oracle as O


def action_between(before, after) -> int:
    """The action that turns board `before` into board `after` (one move of one piece)."""
    b, a = np.asarray(before, dtype=np.int8).reshape(90), np.asarray(after, dtype=np.int8).reshape(90)
    changed = np.nonzero(b != a)[0]
    assert len(changed) == 2, changed
    frm = [int(s) for s in changed if a[s] == 0 and b[s] != 0]
    to = [int(s) for s in changed if a[s] != 0]
    assert len(frm) == 1 and len(to) == 1 and a[to[0]] == b[frm[0]]
    return frm[0] * 90 + to[0]


def expected_record(cfg: dict, peaked: bool, seed: int, **options) -> dict:
    """-> dict(moves, opening_plies, winner, n_moves, n_samples, samples, final_board) of the game the host model plays on
    Draws(seed)."""
    moves, opening, games = [], [], []

    def on_move(search, child, kept, game):
        if not games:
            games.append(game)                         # the loop's own game object: it holds the final position afterwards
            boards = list(game.history()) + [game.board.reshape(90).copy()]
            opening.extend(action_between(x, y) for x, y in zip(boards, boards[1:]))
        moves.append(int(search.action[child]))

    samples, winner, plies, _ = SP.play_game(cfg, peaked, seed, on_move=on_move, **options)
    assert moves, "a game without a searched move has no first on_move call to read the opening from"
    out = opening + moves
    assert len(out) == plies
    return dict(moves=out, opening_plies=len(opening), winner=int(winner), n_moves=int(plies), n_samples=len(samples),
                samples=samples, final_board=games[0].board.reshape(90).copy())


def replay_on_oracle(moves) -> O.Game:
    g = O.Game()
    for a in moves:
        assert int(a) in g.legal_actions(), a
        g.make_action(int(a))
    return g
