"""Host model of a self-play game with forced playouts and policy target pruning (include/xq_hip.h, xq_engine_init_fp), with and
without tree reuse and the playout cap.  TEST INFRASTRUCTURE ONLY: it judges k_select<.., .., true>.  Written from the header's
text, not from the kernel.

The game loop is tests/selfplay_model.py's, the one loop of every self-play model, with the two rules applied to FULL moves
only -- their root is the noisy root, prior kind 1, node 0:
  * forcing, in the descent at node 0: child i with N_i > 0 and N_i^2 < (k rootP[i]) N_root scores +infinity, the first
    maximum takes the lowest-index forced child (ForcedSearch._scores);
  * pruning, at the move's end: the sample's visits and the move-choice weights are the pruned counts v (pruned()); the tree
    keeps N and W, so the hand-off to the next search is unchanged.
k is rounded to float32 once and widened to float64 at every use, as the engine keeps it.  With forced = None no search forces
and no count is pruned (tests/test_forced_playouts_model.py; tests/test_host_model_pins.py pins the games).
"""
from __future__ import annotations

import math

import numpy as np

import tree_reuse_model as M


class ForcedSearch(M.ReuseSearch):
    """The search of a full move with forced playouts at its noisy root."""

    def __init__(self, game, num_simulations, priors, noise, kept=None, k: float = 2.0, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, noise, kept, c_puct)
        self.k = float(np.float32(k))
        self.forced_sims = 0

    def _scores(self, p):
        ucb = super()._scores(p)
        if p != 0 or self.kind[0] != 1:
            return ucb
        f, n = int(self.first[0]), int(self.nch[0])
        assert not self.vl[f:f + n].any() and self.vl[0] == 0          # K = 1: no virtual loss
        N = self.N[f:f + n]
        fi = (self.k * self.P64[f:f + n]) * float(int(self.N[0]))
        forced = (N > 0) & (N.astype(np.float64) * N.astype(np.float64) < fi)
        if forced.any():
            ucb[forced] = np.inf                       # the first maximum takes the lowest-index forced child
            self.forced_sims += 1
        return ucb

    def move_end(self, stats):
        visits = self.root()["visits"]
        assert int(self.N[0]) == self.S == int(visits.sum())           # Nr is the move's budget
        pr = pruned(self)
        stats["forced_sims"] += self.forced_sims
        stats["pruned_visits"] += pr["pruned_visits"]
        stats["pruned_children"] += pr["pruned_children"]
        stats["pruned"].append(pr)
        return pr["v"], None, {}                       # the tree keeps its real N and W


def pruned(s) -> dict:
    """The pruned visit counts of a finished full search `s` (root of kind 1): v int32[n], d (visits subtracted before the
    single-playout rule), cstar, pruned_visits = sum(N - v), pruned_children = children with N > 0 and v == 0."""
    f, n = int(s.first[0]), int(s.nch[0])
    assert int(s.kind[0]) == 1
    N, W, P = s.N[f:f + n], s.W[f:f + n], s.P64[f:f + n]
    k = float(np.float32(getattr(s, "k")))
    nr = int(s.N[0])
    sq = math.sqrt(float(nr))
    cstar = int(np.argmax(N))                          # first maximum

    def puct(i, visits):
        q = float(W[i]) / float(int(N[i]))
        t = float(s.c) * float(P[i])
        t = t * sq
        t = t / float(1 + visits)
        return q + t

    p_star = puct(cstar, int(N[cstar]))
    v = N.astype(np.int64).copy()
    dd = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if i == cstar or N[i] <= 0:
            continue
        fi = (k * float(P[i])) * float(nr)
        m, d = int(N[i]), 0
        while m > 1 and float((d + 1) * (d + 1)) < fi and puct(i, m - 1) < p_star:
            m -= 1
            d += 1
        if d > 0 and m == 1:
            m = 0
        v[i], dd[i] = m, d
    return dict(v=v.astype(np.int32), d=dd, cstar=cstar, N=N.astype(np.int32).copy(),
                pruned_visits=int((N - v).sum()), pruned_children=int(((N > 0) & (v == 0)).sum()))


def play_game(cfg: dict, peaked: bool, draws, tree_reuse: bool = False, cap=None, forced=None, on_move=None):
    import selfplay_model                              # it imports this module
    return selfplay_model.play_game(cfg, peaked, draws, tree_reuse=tree_reuse, cap=cap, forced=forced, on_move=on_move)
