"""Host model of the proven-result search (MCTS-solver; include/xq_hip.h, xq_engine_init_sv), written from the header's rules 1-7.
TEST INFRASTRUCTURE ONLY: it judges the SOLVER instances of k_select.

The search is tests/tree_reuse_model.py's (oracle rules, the oracle's PUCT arithmetic, re-rooting), the game loop follows
tests/playout_cap_model.py's (cap draw, full and fast moves, resign probe), plus
  * a state per node in {UNKNOWN, WIN, DRAW, LOSS}, seen from the side that moved into the node;
  * rule 1: a terminal leaf's state from the true result, its exact value backed up;
  * rule 2: propagation up the path while a state changes;
  * rule 3: a descent stops at the first decided non-root node; a LOSS child scores -inf unless the parent is WIN;
  * rule 4: whenever a search looks at its root -- before every simulation and before the test of the budget -- a root with a
    WIN child ends the move on the first such child;
  * rule 5: the counts a move ends with;
  * rule 6: the states ride through the re-root.
With solver off no state is ever set and the game is playout_cap_model.play_game's (tests/test_solver_model.py).
"""
from __future__ import annotations

import math

import numpy as np

import leaf_batch_model as LB
import tree_reuse_model as M
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key

UNKNOWN, WIN, DRAW, LOSS = 0, 1, 2, 3
VALUE = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}
ARRAYS = M.ARRAYS + ("state",)
COUNTERS = ("proven_nodes", "proven_stops", "proven_moves", "unspent_sims", "removed_visits")


class SolverSearch(M.ReuseSearch):
    """One move's search.  noise None: the root of a fast move or of an arena move (no noise); budget <= num_simulations."""

    def __init__(self, game, num_simulations, priors, noise, kept=None, budget=None, solver=True, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, noise, kept, c_puct)
        self.budget = self.S if budget is None else int(budget)
        self.solver = bool(solver)
        self.state = np.zeros(len(self.N), dtype=np.int64)
        self.early = None                    # rule 4: index of the proven child the move ended on
        self.proven_nodes = self.proven_stops = self.terminal_sims = 0
        self.draw_stops = self.max_propagation = 0

    # ---- rule 3: the score ---------------------------------------------------------------------------------------------------
    def _select(self, p):
        f, n = self.first[p], self.nch[p]
        nn = self.N[f:f + n]
        q = np.zeros(n, dtype=np.float64)
        np.divide(self.W[f:f + n], nn.astype(np.float64), out=q, where=nn != 0)
        sq = math.sqrt(float(self.N[p]))
        if self.kind[p] == 0:
            t = np.float32(self.c) * self.P32[f:f + n]
            t = t * np.float32(sq)
            t = t / (1 + nn).astype(np.float32)
            ucb = (q.astype(np.float32) + t).astype(np.float64)
        else:
            t = self.c * self.P64[f:f + n]
            t = t * sq
            t = t / (1 + nn).astype(np.float64)
            ucb = q + t
        if self.solver and self.state[p] != WIN:
            ucb = np.where(self.state[f:f + n] == LOSS, -np.inf, ucb)
            assert np.isfinite(ucb).any(), "every child LOSS under a parent that is not WIN"
        return int(f + int(np.argmax(ucb)))             # first maximum

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

    def _root_setup(self):
        g = self.game
        legal = g.legal_actions()
        pri, kind, _ = self.priors(g.state_for_nn(), legal)
        if len(legal) == 0:
            return False
        noisy = self.noise is not None
        if self.kept is None:
            self._expand(0, legal, pri, kind, noisy)
            return True
        n_nodes = len(self.kept["N"])
        for k in ARRAYS:
            getattr(self, k)[:n_nodes] = self.kept[k]
        self.alloc = n_nodes
        f, n = int(self.first[0]), int(self.nch[0])
        assert n == len(legal) and list(self.action[f:f + n]) == list(legal)
        if noisy:
            eta = np.asarray(self.noise, dtype=np.float64)[:n]
            if kind == 0:
                assert self.P32[f:f + n].tobytes() == np.asarray(pri, np.float32).tobytes()
                self.P32[f:f + n] = pri
                self.P64[f:f + n] = (np.float32(1.0 - self.eps) * pri).astype(np.float32).astype(np.float64) + self.eps * eta
            else:
                self.P64[f:f + n] = (1.0 - self.eps) * (1.0 / n) + self.eps * eta
            self.kind[0] = 1
        else:
            assert int(self.kind[0]) == kind           # the kind it had as an inner node
            if kind == 0:
                assert self.P32[f:f + n].tobytes() == np.asarray(pri, np.float32).tobytes()
                self.P32[f:f + n] = pri
            else:
                self.P64[f:f + n] = 1.0 / n
        self.reused = int(self.N[f:f + n].sum())
        self.N[0] = self.reused
        self.sims = self.reused
        return True

    def run(self):
        g = self.game
        if not self._root_setup():
            return self
        self.start = {k: getattr(self, k)[:self.alloc].copy() for k in ARRAYS}
        while True:
            if self.solver and self.state[0] == LOSS:   # rule 4: some root child is WIN; tested ahead of the budget
                f, n = int(self.first[0]), int(self.nch[0])
                wins = np.nonzero(self.state[f:f + n] == WIN)[0]
                assert len(wins) > 0
                self.early = int(wins[0])
                break
            if self.sims >= self.budget:
                break
            sim = g.clone()
            node, path, stop = 0, [0], UNKNOWN
            while True:
                if self.solver and node != 0 and self.state[node] != UNKNOWN:
                    stop = int(self.state[node])
                    break
                if self.nch[node] == 0:
                    break
                node = self._select(node)
                sim.make_action(int(self.action[node]))
                path.append(node)
            if stop != UNKNOWN:                         # rule 3
                self._backup(path, VALUE[stop])
                self.proven_stops += 1
                self.draw_stops += stop == DRAW
                self.terminal_sims += 1
            else:
                over, winner = sim.is_game_over()
                if over and self.solver:                # rule 1
                    mover = -sim.current_player
                    st = DRAW if winner == 0 else (WIN if winner == mover else LOSS)
                    assert len(path) > 1
                    self.state[node] = st
                    self._backup(path, VALUE[st])
                    self.proven_nodes += 1 + self._propagate(path)
                    self.terminal_sims += 1
                elif over:
                    self._backup(path, 0.0 if winner == 0 else 1.0)
                    self.terminal_sims += 1
                else:
                    lg = sim.legal_actions()
                    p, k, value = self.priors(sim.state_for_nn(), lg)
                    self._expand(node, lg, p, k, False)
                    self._backup(path, -float(np.float32(value)))
            self.sims += 1
        return self

    def reroot(self, c):
        if self.first[c] < 0:
            return None
        order = M.compaction_order(self.first, self.nch, c, self.alloc)
        out = {k: getattr(self, k)[order].copy() for k in ARRAYS}
        out["first"] = M.remap_first(self.first, order)
        out["old_index"] = order
        return out

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


def _searchable(g, cfg):
    return not g.is_game_over()[0] and g.move_count < int(cfg["max_game_length"])


def play_game(cfg: dict, peaked: bool, draws, tree_reuse: bool = False, cap=None, solver: bool = True, on_move=None):
    """One self-play game on `draws` (a Draws, or a seed) -> (samples, winner, plies, stats): playout_cap_model.play_game with the
    solver's rules.  Samples carry `visits` = rule 5's v and `proven` (reserved1).  stats adds the five solver counters,
    terminal_sims, fast_early (fast moves ended by rule 4) and draw_stops."""
    d = Draws(draws) if isinstance(draws, int) else draws
    priors = LB.stub_priors(peaked)
    S = int(cfg["num_simulations"])
    g = O.Game()
    k = d.randint(0, int(cfg["random_opening_moves"]))
    for _ in range(k):
        legal = g.legal_actions()
        if len(legal) == 0:
            break
        g.make_action(int(legal[d.choice_index(len(legal))]))
        if g.is_game_over()[0]:
            g = O.Game()
            break
    samples, resign_hist, kept = [], [], None
    stats = dict(sims=0, reused_visits=0, reroots=0, fast_moves=0, fast_sims=0, full_moves=0, moves=[], terminal_sims=0,
                 fast_early=0, draw_stops=0, **{k: 0 for k in COUNTERS})
    full = True
    if cap is not None and _searchable(g, cfg):
        full = d.uniform() < float(cap[0])
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
        budget = S if full else int(cap[1])
        noise = d.dirichlet(len(g.legal_actions())) if full else None
        s = SolverSearch(g, S, priors, noise, kept, budget, solver).run()
        new = s.sims - s.reused
        assert new == (max(0, budget - s.reused) if s.early is None else new) and new >= 0
        stats["full_moves" if full else "fast_moves"] += 1
        if not full:
            stats["fast_sims"] += new
        stats["sims"] += new
        stats["reused_visits"] += s.reused
        stats["reroots"] += kept is not None
        stats["terminal_sims"] += s.terminal_sims
        stats["proven_nodes"] += s.proven_nodes
        stats["proven_stops"] += s.proven_stops
        stats["draw_stops"] += s.draw_stops
        r = s.root()
        v, removed = s.final_counts()
        stats["removed_visits"] += removed
        if s.early is not None:
            stats["proven_moves"] += 1
            stats["unspent_sims"] += max(0, budget - s.sims)
            stats["fast_early"] += not full
        stats["moves"].append(dict(full=full, reused=s.reused, visits=int(v.sum()), new=new, early=s.early is not None))
        if full:
            samples.append(dict(board=g.board.reshape(90).copy(), player=g.current_player, actions=r["actions"].copy(),
                                visits=v.astype(np.int32), late=late, proven=int(s.early is not None)))
        i = s.early if s.early is not None else M.choose(r["actions"], v, late, d.uniform())
        c = int(s.first[0]) + i
        kept = s.reroot(c) if tree_reuse else None
        if on_move is not None:
            on_move(s, c, kept, g)
        g.make_action(int(r["actions"][i]))
        if cap is not None and _searchable(g, cfg):
            full = d.uniform() < float(cap[0])
        if cfg["enable_resign"] and len(samples) > 10:
            _, val = predict_from_key(state_key(g.state_for_nn()), peaked)
            resign_hist.append(val)
            K = int(cfg["resign_check_steps"])
            if len(resign_hist) >= K and all(x < float(cfg["resign_threshold"]) for x in resign_hist[-K:]):
                winner = -g.current_player
                break
    for smp in samples:
        smp["z"] = 0 if winner == 0 else (1 if winner == smp["player"] else -1)
    return samples, winner, g.move_count, stats


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
