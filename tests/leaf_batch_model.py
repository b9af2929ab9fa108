"""Host model of the engine's search with leaf batching (K leaves per slot and step under virtual loss; include/xq_hip.h,
xq_engine_init_leaves).  TEST INFRASTRUCTURE ONLY: it judges k_select_multi / k_expand_multi.

Rules come from the CPU oracle (`oracle.xq_oracle.Game`: legal actions, make_action, is_game_over, state_for_nn); the PUCT
arithmetic is the one the oracle documents (oracle/xq_oracle.c, "MCTS (mcts.py)"), with the virtual loss vl of the header:
child i of parent p is scored with n = N_i + vl_i, w = W_i - vl_i (float64) and sqrt(N_p + vl_p).  With K = 1 no vl is ever
non-zero and the model is the reference's sequential search (tests/test_leaf_batch_model.py pins that against the oracle).

A step: descents j = 0, 1, ... from the root until K leaves are pending, or sims + pending == S, or a collision (a descent
that ends on a leaf already pending in this step: dropped, not a simulation, ends the collection); a terminal leaf is backed
up at once (at most 48 per step); then the pending leaves are evaluated, expanded and backed up in descent order, each
backup removing its descent's virtual loss.
"""
from __future__ import annotations

import math

import numpy as np

from stub_eval import predict_from_key, state_key

TERMINAL_RUN = 48          # terminal simulations per step and slot at most (k_select's bound)


def stub_priors(peaked: bool):
    """priors(state, legal) -> (priors, kind, value) from the stub evaluator's dense probabilities, as the engine's expand
    computes them (is_probs = 1): sequential float32 sum over the legal moves, float32 division; a zero sum gives uniform."""
    cache = {}

    def f(state, legal):
        key = state_key(state)
        if key not in cache:
            cache[key] = predict_from_key(key, peaked)
        probs, value = cache[key]
        return priors_from_probs(probs[np.asarray(legal, dtype=np.int64)]) + (value,)

    return f


def priors_from_probs(p):
    p = np.asarray(p, dtype=np.float32)
    s = np.float32(0.0)
    for x in p:                                        # builtin sum(): sequential float32, move order
        s = np.float32(s + x)
    if s > 0:
        return (p / s).astype(np.float32), 0
    return np.full(len(p), 1.0 / len(p), dtype=np.float64), 2


class LeafBatchSearch:
    """One position's search.  `priors(state f32[15,10,9], legal u16[n]) -> (priors, kind, value)`: kind 0 float32 priors,
    2 uniform (float64 1/n); value the network's float32 output.  `noise`: float64 eta per legal root move (kind 1 root)."""

    def __init__(self, game, num_simulations: int, leaves_per_step: int, priors, c_puct: float = 1.5, noise=None,
                 noise_eps: float = 0.25):
        self.game, self.S, self.K, self.priors, self.c = game, int(num_simulations), int(leaves_per_step), priors, float(c_puct)
        cap = 1 + (self.S + 1) * 200
        self.N = np.zeros(cap, dtype=np.int64)
        self.W = np.zeros(cap, dtype=np.float64)
        self.vl = np.zeros(cap, dtype=np.int64)
        self.P32 = np.zeros(cap, dtype=np.float32)
        self.P64 = np.zeros(cap, dtype=np.float64)
        self.first = np.full(cap, -1, dtype=np.int64)
        self.nch = np.zeros(cap, dtype=np.int64)
        self.kind = np.zeros(cap, dtype=np.int64)
        self.action = np.zeros(cap, dtype=np.int64)
        self.alloc = 1
        self.sims = self.collisions = self.steps = self.terminal_sims = 0
        self.leaves_per_step = []
        self.noise, self.eps = noise, float(noise_eps)

    # ---- tree ------------------------------------------------------------------------------------------------------------
    def _noisy(self, pri, kind, n):
        """The float64 priors of a noisy root (kind 1) over priors of `kind`."""
        eta = np.asarray(self.noise, dtype=np.float64)[:n]
        if kind == 0:
            return (np.float32(1.0 - self.eps) * pri).astype(np.float32).astype(np.float64) + self.eps * eta
        return (1.0 - self.eps) * (1.0 / n) + self.eps * eta

    def _expand(self, node, legal, pri, kind, noisy):
        n = len(legal)
        f = self.alloc
        self.alloc += n
        self.first[node], self.nch[node] = f, n
        self.action[f:f + n] = legal
        if noisy:
            self.P64[f:f + n] = self._noisy(pri, kind, n)
            self.kind[node] = 1
        elif kind == 0:
            self.P32[f:f + n] = pri
            self.kind[node] = 0
        else:
            self.P64[f:f + n] = 1.0 / n
            self.kind[node] = 2

    def _scores(self, p):
        """The PUCT score of every child of p: float32 arithmetic over float32 priors (kind 0), float64 otherwise."""
        f, n = self.first[p], self.nch[p]
        v = self.vl[f:f + n]
        nn = self.N[f:f + n] + v
        w = self.W[f:f + n] - v.astype(np.float64)
        q = np.zeros(n, dtype=np.float64)
        np.divide(w, nn.astype(np.float64), out=q, where=nn != 0)
        sq = math.sqrt(float(self.N[p] + self.vl[p]))
        if self.kind[p] == 0:
            t = np.float32(self.c) * self.P32[f:f + n]
            t = t * np.float32(sq)
            t = t / (1 + nn).astype(np.float32)
            ucb = q.astype(np.float32) + t
        else:
            t = self.c * self.P64[f:f + n]
            t = t * sq
            t = t / (1 + nn).astype(np.float64)
            ucb = q + t
        return ucb

    def _select(self, p):
        return int(self.first[p] + int(np.argmax(self._scores(p))))     # first maximum

    def _descend(self, sim):
        """One descent from the root to a leaf (or to a node `_decided` stops it at), played on `sim` -> the path."""
        node, path = 0, [0]
        while self.nch[node] > 0 and not self._decided(node):
            node = self._select(node)
            sim.make_action(int(self.action[node]))
            path.append(node)
        return path

    def _decided(self, node):
        """A node whose value is known without looking below it (none here: the solver's rule 3)."""
        return False

    def _terminal(self, sim, path):
        """The value a descent that ended on a finished game backs up, from the view of the side that moved into the leaf, or
        None when the leaf is to be evaluated."""
        over, winner = sim.is_game_over()
        return (0.0 if winner == 0 else 1.0) if over else None

    def _backup(self, path, v, vl=0):
        for k, nd in enumerate(reversed(path)):
            self.N[nd] += 1
            self.W[nd] += v if k % 2 == 0 else -v
            self.vl[nd] -= vl

    # ---- search ----------------------------------------------------------------------------------------------------------
    def run(self):
        g = self.game
        legal = g.legal_actions()
        self.current = g                               # the position being evaluated (for evaluators that need it)
        pri, kind, _ = self.priors(g.state_for_nn(), legal)
        if len(legal) == 0:
            return self
        self._expand(0, legal, pri, kind, self.noise is not None)
        while self.sims < self.S:
            self.steps += 1
            pend = []                                  # (path, state, legal, game)
            term_run = 0
            while True:
                if pend and (len(pend) >= self.K or self.sims + len(pend) >= self.S):
                    break
                if self.sims >= self.S:
                    break
                sim = g.clone()
                path = self._descend(sim)
                if any(p[0][-1] == path[-1] for p in pend):
                    self.collisions += 1
                    break
                v = self._terminal(sim, path)
                if v is not None:
                    self._backup(path, v)
                    self.sims += 1
                    self.terminal_sims += 1
                    term_run += 1
                    if term_run >= TERMINAL_RUN:
                        break
                    continue
                pend.append((path, sim.state_for_nn(), sim.legal_actions(), sim))
                self.vl[path] += 1
            if pend:
                self.leaves_per_step.append(len(pend))
            for path, state, lg, sim in pend:
                self.current = sim
                pri, kind, value = self.priors(state, lg)
                self._expand(path[-1], lg, pri, kind, False)
                self._backup(path, -float(np.float32(value)), vl=1)
                self.sims += 1
        assert not self.vl.any()
        return self

    def root(self) -> dict:
        f, n = self.first[0], self.nch[0]
        if n <= 0:
            return dict(actions=np.zeros(0, np.uint16), visits=np.zeros(0, np.int32), total_value=np.zeros(0), prior=np.zeros(0),
                        prior_is_f64=False, root_visits=int(self.N[0]), collisions=self.collisions)
        k = self.kind[0]
        prior = self.P32[f:f + n].astype(np.float64) if k == 0 else self.P64[f:f + n].copy()
        return dict(actions=self.action[f:f + n].astype(np.uint16), visits=self.N[f:f + n].astype(np.int32),
                    total_value=self.W[f:f + n].copy(), prior=prior, prior_is_f64=bool(k != 0), root_visits=int(self.N[0]),
                    collisions=self.collisions)


def search(game, num_simulations, leaves_per_step, priors, c_puct=1.5, noise=None) -> dict:
    return LeafBatchSearch(game, num_simulations, leaves_per_step, priors, c_puct, noise).run().root()
