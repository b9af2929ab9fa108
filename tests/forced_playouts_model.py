"""Host model of a self-play game with forced playouts and policy target pruning (include/xq_hip.h, xq_engine_init_fp), with and
without tree reuse and the playout cap.  TEST INFRASTRUCTURE ONLY: it judges k_select<.., .., true>.  Written from the header's
text, not from the kernel.

It is tests/playout_cap_model.py's game loop (imported, not edited; that one is tests/tree_reuse_model.py's plus the cap) with
the two rules applied to FULL moves only -- their root is the noisy root, prior kind 1, node 0:
  * forcing, in the descent at node 0: child i with N_i > 0 and N_i^2 < (k rootP[i]) N_root scores +infinity, the first
    maximum takes the lowest-index forced child (ForcedSearch._select);
  * pruning, at the move's end: the sample's visits and the move-choice weights are the pruned counts v (pruned()); the tree
    keeps N and W, so the hand-off to the next search is unchanged.
k is rounded to float32 once and widened to float64 at every use, as the engine keeps it.  With forced = None the game is
playout_cap_model.play_game's (tests/test_forced_playouts_model.py checks that on every recorded game).
"""
from __future__ import annotations

import math

import numpy as np

import leaf_batch_model as LB
import playout_cap_model as PC
import tree_reuse_model as M
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key


class ForcedSearch(M.ReuseSearch):
    """The search of a full move with forced playouts at its noisy root."""

    def __init__(self, game, num_simulations, priors, noise, kept=None, k: float = 2.0, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, noise, kept, c_puct)
        self.k = float(np.float32(k))
        self.forced_sims = 0

    def _select(self, p):
        if p != 0 or self.kind[0] != 1:
            return super()._select(p)
        f, n = int(self.first[0]), int(self.nch[0])
        assert not self.vl[f:f + n].any() and self.vl[0] == 0          # K = 1: no virtual loss
        N = self.N[f:f + n]
        q = np.zeros(n, dtype=np.float64)
        np.divide(self.W[f:f + n], N.astype(np.float64), out=q, where=N != 0)
        nr = int(self.N[0])
        t = self.c * self.P64[f:f + n]
        t = t * math.sqrt(float(nr))
        t = t / (1 + N).astype(np.float64)
        ucb = q + t
        fi = (self.k * self.P64[f:f + n]) * float(nr)
        forced = (N > 0) & (N.astype(np.float64) * N.astype(np.float64) < fi)
        if forced.any():
            ucb[forced] = np.inf
            self.forced_sims += 1
        return f + int(np.argmax(ucb))                 # first maximum


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
    """One self-play game on `draws` (a Draws, or a seed) -> (samples, winner, plies, stats).  cap = (p, S_fast) or None;
    forced = k or None.  stats: playout_cap_model's plus forced_sims, pruned_visits, pruned_children and, per full move,
    `pruned` (the dict of pruned())."""
    if forced is None:
        samples, winner, plies, stats = PC.play_game(cfg, peaked, draws, tree_reuse=tree_reuse, cap=cap, on_move=on_move)
        stats.update(forced_sims=0, pruned_visits=0, pruned_children=0, pruned=[])
        return samples, winner, plies, stats
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
    stats = dict(sims=0, reused_visits=0, reroots=0, fast_moves=0, fast_sims=0, full_moves=0, moves=[], forced_sims=0,
                 pruned_visits=0, pruned_children=0, pruned=[])
    full = True
    if cap is not None and PC._searchable(g, cfg):
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
        if full:
            noise = d.dirichlet(len(g.legal_actions()))
            s = ForcedSearch(g, S, priors, noise, kept, k=forced).run()
            new = S - s.reused
            stats["full_moves"] += 1
            stats["forced_sims"] += s.forced_sims
        else:
            s = PC.FastSearch(g, S, int(cap[1]), priors, kept).run()
            new = max(0, int(cap[1]) - s.reused)
            stats["fast_moves"] += 1
            stats["fast_sims"] += new
        assert s.sims == s.reused + new
        stats["sims"] += new
        stats["reused_visits"] += s.reused
        stats["reroots"] += kept is not None
        r = s.root()
        visits = r["visits"]
        stats["moves"].append(dict(full=full, reused=s.reused, visits=int(visits.sum()), new=new))
        if full:
            assert int(s.N[0]) == S == int(visits.sum())               # Nr is the move's budget
            pr = pruned(s)
            visits = pr["v"]
            stats["pruned_visits"] += pr["pruned_visits"]
            stats["pruned_children"] += pr["pruned_children"]
            stats["pruned"].append(pr)
            samples.append(dict(board=g.board.reshape(90).copy(), player=g.current_player, actions=r["actions"].copy(),
                                visits=visits.copy(), late=late))
        i = M.choose(r["actions"], visits, late, d.uniform())
        c = int(s.first[0]) + i
        kept = s.reroot(c) if tree_reuse else None     # the tree keeps its real N and W
        if on_move is not None:
            on_move(s, c, kept)
        g.make_action(int(r["actions"][i]))
        if cap is not None and PC._searchable(g, cfg):
            full = d.uniform() < float(cap[0])
        if cfg["enable_resign"] and len(samples) > 10:
            _, v = predict_from_key(state_key(g.state_for_nn()), peaked)
            resign_hist.append(v)
            K = int(cfg["resign_check_steps"])
            if len(resign_hist) >= K and all(x < float(cfg["resign_threshold"]) for x in resign_hist[-K:]):
                winner = -g.current_player
                break
    for smp in samples:
        smp["z"] = 0 if winner == 0 else (1 if winner == smp["player"] else -1)
    return samples, winner, g.move_count, stats
