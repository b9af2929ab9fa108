"""Host model of the proven-result search (MCTS-solver; include/xq_hip.h, xq_engine_init_sv), written from the header's rules 1-7.
TEST INFRASTRUCTURE ONLY: it judges the SOLVER instances of k_select.

The search is tests/tree_reuse_model.py's (oracle rules, the oracle's PUCT arithmetic, re-rooting), the game loop is
tests/selfplay_model.py's, the one loop of every self-play model (cap draw, full and fast moves, resign probe), plus
  * a state per node in {UNKNOWN, WIN, DRAW, LOSS}, seen from the side that moved into the node;
  * rule 1: a terminal leaf's state from the true result, its exact value backed up;
  * rule 2: propagation up the path while a state changes;
  * rule 3: a descent stops at the first decided non-root node; a LOSS child scores -inf unless the parent is WIN;
  * rule 4: whenever a search looks at its root -- before every simulation and before the test of the budget -- a root with a
    WIN child ends the move on the first such child;
  * rule 5: the counts a move ends with;
  * rule 6: the states ride through the re-root.
With solver off no state is ever set (tests/test_solver_model.py; tests/test_host_model_pins.py pins the games).
"""
from __future__ import annotations

import numpy as np

import leaf_batch_model as LB
import tree_reuse_model as M
from oracle import xq_oracle as O

UNKNOWN, WIN, DRAW, LOSS = 0, 1, 2, 3
VALUE = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}
ARRAYS = M.ARRAYS + ("state",)
COUNTERS = ("proven_nodes", "proven_stops", "proven_moves", "unspent_sims", "removed_visits")


class SolverSearch(M.ReuseSearch):
    """One move's search.  noise None: the root of a fast move or of an arena move (no noise); budget <= num_simulations."""

    ARRAYS = ARRAYS                                    # rule 6: the states ride through the re-root

    def __init__(self, game, num_simulations, priors, noise, kept=None, budget=None, solver=True, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, noise, kept, c_puct, budget=budget)
        self.solver = bool(solver)
        self.state = np.zeros(len(self.N), dtype=np.int64)
        self.early = None                    # rule 4: index of the proven child the move ended on
        self.proven_nodes = self.proven_stops = 0
        self.draw_stops = self.max_propagation = 0

    # ---- rule 3: the stop and the score ----------------------------------------------------------------------------------------
    def _decided(self, node):
        return self.solver and node != 0 and self.state[node] != UNKNOWN

    def _scores(self, p):
        ucb = super()._scores(p)
        if self.solver and self.state[p] != WIN:
            f, n = self.first[p], self.nch[p]
            ucb = np.where(self.state[f:f + n] == LOSS, -np.inf, ucb)
            assert np.isfinite(ucb).any(), "every child LOSS under a parent that is not WIN"
        return ucb

    def _terminal(self, sim, path):
        node = path[-1]
        if self._decided(node):                         # rule 3
            stop = int(self.state[node])
            self.proven_stops += 1
            self.draw_stops += stop == DRAW
            return VALUE[stop]
        over, winner = sim.is_game_over()
        if not (over and self.solver):
            return super()._terminal(sim, path)
        mover = -sim.current_player                     # rule 1
        st = DRAW if winner == 0 else (WIN if winner == mover else LOSS)
        assert len(path) > 1
        self.state[node] = st
        self.proven_nodes += 1 + self._propagate(path)
        return VALUE[st]

    # ---- rule 4 --------------------------------------------------------------------------------------------------------------
    def _finished(self):
        if self.solver and self.state[0] == LOSS:       # some root child is WIN; tested ahead of the budget
            f, n = int(self.first[0]), int(self.nch[0])
            wins = np.nonzero(self.state[f:f + n] == WIN)[0]
            assert len(wins) > 0
            self.early = int(wins[0])
            return True
        return super()._finished()

    # ---- rule 2 --------------------------------------------------------------------------------------------------------------
    def _propagate(self, path):
        changed = 0
        for j in range(len(path) - 2, -1, -1):
            p, c = path[j], path[j + 1]
            if self.state[p] != UNKNOWN:
                break
            if self.state[c] == WIN:
                ns = LOSS
            else:
                f, n = self.first[p], self.nch[p]
                st = self.state[f:f + n]
                if (st == UNKNOWN).any():
                    break
                ns = DRAW if (st == DRAW).any() else WIN
                assert ns == DRAW or (st == LOSS).all()
            self.state[p] = ns
            changed += 1
        self.max_propagation = max(self.max_propagation, changed)
        return changed

    # ---- what the engine's readers report ----------------------------------------------------------------------------------------
    def root_states(self):
        """(children, root) in xq_engine_read_root_states' code: from the view of the side to move at the root."""
        f, n = int(self.first[0]), int(self.nch[0])
        child = np.array([{UNKNOWN: 0, WIN: 1, DRAW: 2, LOSS: -1}[int(s)] for s in self.state[f:f + n]], dtype=np.int8)
        return child, {UNKNOWN: 0, WIN: -1, DRAW: 2, LOSS: 1}[int(self.state[0])]

    def final_counts(self):
        """Rule 5 -> (v, removed)."""
        f, n = int(self.first[0]), int(self.nch[0])
        N, st = self.N[f:f + n].astype(np.int64), self.state[f:f + n]
        unspent = max(0, self.budget - self.sims) if self.early is not None else 0
        v = N.copy()
        if self.solver and (st != LOSS).any():
            v[st == LOSS] = 0
        if self.early is not None:
            v[self.early] += unspent
        if not v.any():
            v = N.copy()
        return v, int((N - v).clip(min=0).sum())

    def move_end(self, stats):
        v, removed = self.final_counts()
        for k in ("proven_nodes", "proven_stops", "draw_stops"):
            stats[k] += getattr(self, k)
        stats["removed_visits"] += removed
        if self.early is not None:
            stats["proven_moves"] += 1
            stats["unspent_sims"] += max(0, self.budget - self.sims)
            stats["fast_early"] += self.noise is None   # a fast move
        return v.astype(np.int32), self.early, dict(visits=int(v.sum()), early=self.early is not None)

    def check_consistency(self):
        """The invariants of rules 1-2 over the whole tree."""
        for p in range(self.alloc):
            n = int(self.nch[p])
            if n == 0:
                continue
            st = self.state[int(self.first[p]):int(self.first[p]) + n]
            if (st == WIN).any():
                assert self.state[p] == LOSS, p                       # a WIN child implies a LOSS parent
            elif not (st == UNKNOWN).any():
                assert self.state[p] == (DRAW if (st == DRAW).any() else WIN), p
            if self.state[p] == UNKNOWN:
                assert not (st == WIN).any(), p


def minimax(game, depth):
    """Brute-force result of `game` from the view of the side that moved into it over the oracle's rules, looking `depth` plies
    ahead: WIN / DRAW / LOSS, or UNKNOWN when the horizon does not decide it."""
    over, winner = game.is_game_over()
    if over:
        mover = -game.current_player
        return DRAW if winner == 0 else (WIN if winner == mover else LOSS)
    if depth == 0:
        return UNKNOWN
    res = []
    for a in game.legal_actions():
        g = game.clone()
        g.make_action(int(a))
        r = minimax(g, depth - 1)
        if r == WIN:
            return LOSS
        res.append(r)
    if UNKNOWN in res:
        return UNKNOWN
    return DRAW if DRAW in res else WIN


def play_game(cfg: dict, peaked: bool, draws, tree_reuse: bool = False, cap=None, solver: bool = True, on_move=None):
    import selfplay_model                              # it imports this module
    return selfplay_model.play_game(cfg, peaked, draws, tree_reuse=tree_reuse, cap=cap, solver=solver, on_move=on_move)


def search_position(game, num_simulations, peaked=False, noise=None, solver=True):
    """Search only (manual_moves = 1): one search of `game` under the stub evaluator; `noise`: eta per legal move or None."""
    return SolverSearch(game, num_simulations, LB.stub_priors(peaked), noise, None, None, solver).run()


def crafted_game(pieces, player=1):
    """A Game on an otherwise empty board: pieces = [(row, col, piece)], red positive."""
    g = O.Game()
    b = np.zeros((10, 9), dtype=np.int8)
    for r, c, p in pieces:
        b[r, c] = p
    g.set_board(b, player)
    return g


def arena_game(predict_priors, new_is_red, num_simulations, max_game_length, solver=True, opening=()):
    """One arena game (no noise, first maximum of rule 5's v) -> (winner, plies, moves, stats).  predict_priors = (new, old):
    a priors function per model; `opening`: actions played first.  moves: per move (action, child states, chosen index, the first
    maximum of the plain visit counts: what an engine without the option would have played from this tree, ended by rule 4)."""
    g = O.Game()
    for a in opening:
        g.make_action(int(a))
    stats = {k: 0 for k in COUNTERS}
    stats["sims"] = 0
    moves = []
    while True:
        over, w = g.is_game_over()
        if over:
            return w, g.move_count, moves, stats
        if g.move_count >= int(max_game_length):
            return 0, g.move_count, moves, stats
        new_to_move = (g.current_player == 1) == bool(new_is_red)
        s = SolverSearch(g, num_simulations, predict_priors[0 if new_to_move else 1], None, None, None, solver).run()
        v, removed = s.final_counts()
        stats["sims"] += s.sims
        stats["proven_nodes"] += s.proven_nodes
        stats["proven_stops"] += s.proven_stops
        stats["removed_visits"] += removed
        if s.early is not None:
            i = s.early
            stats["proven_moves"] += 1
            stats["unspent_sims"] += max(0, s.budget - s.sims)
        else:
            i = int(np.argmax(v))
        r = s.root()
        moves.append((int(r["actions"][i]), s.root_states()[0], i, int(np.argmax(r["visits"])), s.early is not None))
        g.make_action(int(r["actions"][i]))
