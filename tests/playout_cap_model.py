"""Host model of a self-play game with playout cap randomization (include/xq_hip.h, xq_engine_init_cap), with and without tree
reuse.  TEST INFRASTRUCTURE ONLY: it judges k_select<.., true> / k_expand<.., true>.

The game loop is tests/selfplay_model.py's, the one loop of every self-play model; the rules of the cap in it:
  * every position that will be searched (not over, not adjudicated at max_game_length) takes one draw u of the uniform stream
    when its root request is issued -- BEFORE the resign probe of that root evaluation -- and the move is full iff u < p;
  * a full move is the move of a game without the cap: Dirichlet noise, budget S, a sample;
  * a fast move takes no Dirichlet draw, has no noise at the root (a fresh root is a root with add_noise = 0; a reused root keeps
    the kind it had as an inner node), runs until sims >= S_fast -- no new simulation when it inherits that many -- and records
    no sample; the move choice is unchanged;
  * the resign rule counts recorded samples.
With cap = None no cap draw is taken (tests/test_playout_cap_model.py; tests/test_host_model_pins.py pins the games).
"""
from __future__ import annotations

import tree_reuse_model as M
from draws import Draws


class FastSearch(M.ReuseSearch):
    """The search of a fast move: `ReuseSearch` without root noise, budget `budget` <= num_simulations."""

    def __init__(self, game, num_simulations, budget, priors, kept=None, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, None, kept, c_puct, budget=budget)


class SplicedDraws(Draws):
    """Draws(seed) whose uniform stream has a dummy draw spliced in before every draw of the original stream: what a cap-on game
    with p = 1 must consume to replay the cap-off game of Draws(seed)."""

    def __init__(self, seed: int, dummy: float = 0.5):
        super().__init__(seed)
        self._odd, self._dummy = False, float(dummy)

    def uniform(self) -> float:
        self._odd = not self._odd
        return self._dummy if self._odd else super().uniform()


def play_game(cfg: dict, peaked: bool, draws, tree_reuse: bool = False, cap=None, on_move=None):
    import selfplay_model                              # it imports this module
    return selfplay_model.play_game(cfg, peaked, draws, tree_reuse=tree_reuse, cap=cap, on_move=on_move)
