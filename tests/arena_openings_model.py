"""Host model of the arena with paired random openings (include/xq_hip.h, xq_engine_init_ar), written from the header's
rules on the oracle's `Game`, `mcts_search` (no noise) and `make_action`.

  * the opening rule: ply i plays move x_i % cnt of the ordered legal moves; a ply that ends the game restarts it from the
    initial position with no opening;
  * one arena game from a given list of opening actions (training/train.py:453-535): the model whose side is to move
    searches, the move is the first maximum of the visit counts, the opening plies count as plies, and a game that is not
    over after `max_game_length` plies is a draw.
"""
from __future__ import annotations

import draws as D
from oracle import xq_oracle as O


def opening_actions(raw_draws, plies: int):
    """The opening the engine plays from the raw 64-bit draws x_0 .. x_{plies-1}: the list of actions, [] after the restart
    rule."""
    g = O.Game()
    acts = []
    for i in range(int(plies)):
        legal = g.legal_actions()
        if len(legal) == 0:
            break
        a = int(legal[int(raw_draws[i]) % len(legal)])
        g.make_action(a)
        acts.append(a)
        if g.is_game_over()[0]:
            return []
    return acts


def choice_stream(seed: int, n: int):
    """The first n raw draws of the choice stream of tests/draws.py for `seed` (what a test injects as a slot's stream 1)."""
    s = D.Draws(seed).s_choice
    return [s.next_u64() for _ in range(n)]


def play_game(opening, predict_new, predict_old, new_is_red: bool, num_simulations: int, max_game_length: int,
              c_puct: float = 1.5):
    """One arena game that starts with the plies `opening` -> (winner, steps)."""
    g = O.Game()
    for a in opening:
        g.make_action(int(a))
    step = len(opening)
    done, w = g.is_game_over()
    while not done and step < max_game_length:
        use_new = bool(new_is_red) == (g.current_player == 1)          # train.py:479-483
        res = O.mcts_search(g, num_simulations, predict_new if use_new else predict_old, c_puct)
        assert res.n_children > 0
        best = 0                                                       # get_action(temperature=0): first maximum, mcts.py:197-200
        for i in range(1, res.n_children):
            if res.visits[i] > res.visits[best]:
                best = i
        g.make_action(int(res.actions[best]))
        step += 1
        done, w = g.is_game_over()
    return (int(w) if done else 0), step                               # train.py:494-496
