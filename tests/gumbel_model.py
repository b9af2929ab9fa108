"""Host model of a self-play game (and of one search) with the Gumbel root search with sequential halving (include/xq_hip.h,
xq_engine_init_gz).  TEST INFRASTRUCTURE ONLY: it judges k_select<false, false, false, true> / k_expand<false, false, true>.
Written from the header's text, not from the kernels.

The game loop is tests/selfplay_model.py's, the one loop of every self-play model, the search tests/tree_reuse_model.py's, with
the header's rules:
  * root expansion: l_i = log(max(tP[i], FLT_MIN)) in float64, g_i from the raw Dirichlet stream of tests/draws.py (injected
    draws: ((x >> 40) % 4096 - 1024) / 512), rootP = g + l, prior kind 3, no Dirichlet noise;
  * root selection: the candidates are the children with N_i == considered_visits(min(m, cnt), S)[root visits]; the first
    maximum of rootP (cv == 0) or rootP + sigma(q) (cv > 0) wins; every other level is the PUCT of the parent model;
  * end of a move: the first maximum of rootP + sigma(q) over the most visited children is played, no temperature, no uniform
    draw; the sample's visits are the completed-Q improved policy quantised to 16 bits.
c_visit and c_scale are rounded to float32 once and widened at every use, as the engine keeps them.

Every root arg-max (selections and the final move) also records the gap between the winner and the runner-up among its
candidates: the engine's float64 log may differ from this host's in the last bits, so a comparison with the engine is only
meaningful on games whose smallest gap is far above that (stats["min_gap"]; the GPU test asserts it).
"""
from __future__ import annotations

import math

import numpy as np

import tree_reuse_model as M

FLT_MIN = float(np.finfo(np.float32).tiny)


def considered_visits(k: int, S: int):
    """The header's restatement of mctx's get_sequence_of_considered_visits."""
    if k <= 1:
        return list(range(S))
    L = (k - 1).bit_length()                           # ceil(log2(k))
    out, c, base = [], k, 0
    while len(out) < S:
        e = max(1, S // (L * c))
        for j in range(e):
            out.extend([base + j] * c)
        base += e
        c = max(2, c // 2)
    return out[:S]


def injected_gumbels(stream, n: int):
    """n draws g of the header's injected formula from a raw draws.Stream (exact in float64)."""
    return np.array([(float((stream.next_u64() >> 40) % 4096) - 1024.0) / 512.0 for _ in range(n)], dtype=np.float64)


def _gap(score, cand, win):
    """winner's score minus the best other candidate's (inf when it has no rival)."""
    rest = [float(score[i]) for i in np.nonzero(cand)[0] if i != win]
    return float(score[win]) - max(rest) if rest else math.inf


class GumbelSearch(M.ReuseSearch):
    """The search of one position under the Gumbel root rule; `g`: one float64 Gumbel value per legal move."""

    def __init__(self, game, num_simulations, priors, g, gumbel, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, None, None, c_puct)
        self.g = np.asarray(g, dtype=np.float64)
        self.m = int(gumbel[0])
        self.c_visit, self.c_scale = float(np.float32(gumbel[1])), float(np.float32(gumbel[2]))
        self.min_gap = math.inf
        self.tables = {}

    def sigma_scale(self, max_n: int) -> float:
        return (self.c_visit + float(max_n)) * self.c_scale

    def _expand_root(self, legal, pri, kind, value):
        self._expand(0, legal, pri, kind, False)
        f, n = int(self.first[0]), int(self.nch[0])
        if kind != 0:                                  # no mass on the legal moves: float32 uniform priors
            self.P32[f:f + n] = np.float32(1.0 / n)
        self.l = np.array([math.log(max(float(p), FLT_MIN)) for p in self.P32[f:f + n]], dtype=np.float64)
        self.P64[f:f + n] = self.g[:n] + self.l
        self.kind[0] = 3
        self.v_hat = float(np.float32(value))
        self.k = min(self.m, n)

    def _select(self, p):
        if p != 0 or self.kind[0] != 3:
            return super()._select(p)
        f, n = int(self.first[0]), int(self.nch[0])
        N, rootP = self.N[f:f + n], self.P64[f:f + n]
        if self.k not in self.tables:
            self.tables[self.k] = considered_visits(self.k, self.S)
        cv = self.tables[self.k][int(self.N[0])]
        cand = N == cv
        assert cand.any(), "the equal-visit rule found no candidate"
        score = rootP.copy()
        if cv > 0:
            q = np.zeros(n, dtype=np.float64)
            np.divide(self.W[f:f + n], N.astype(np.float64), out=q, where=N != 0)
            score = rootP + self.sigma_scale(int(N.max())) * ((q + 1.0) * 0.5)
        score = np.where(cand, score, -np.inf)
        win = int(np.argmax(score))                    # first maximum
        self.min_gap = min(self.min_gap, _gap(score, cand, win))
        return f + win

    def root(self) -> dict:
        r = super().root()
        r["prior_kind"] = int(self.kind[0])
        return r

    def finish(self) -> dict:
        """The end of the move: played child, the quantised improved policy, and the pieces the tests look at."""
        f, n = int(self.first[0]), int(self.nch[0])
        N, W, rootP = self.N[f:f + n], self.W[f:f + n], self.P64[f:f + n]
        tP = self.P32[f:f + n]
        q = [float(W[i]) / float(int(N[i])) if N[i] else 0.0 for i in range(n)]
        max_n = sum_n = 0
        num = den = 0.0
        for i in range(n):                             # sequential, move order
            max_n = max(max_n, int(N[i]))
            sum_n += int(N[i])
            if N[i] > 0:
                num += float(tP[i]) * q[i]
                den += float(tP[i])
        scale = self.sigma_scale(max_n)
        v_mix = (self.v_hat + float(sum_n) * (num / den if den > 0.0 else self.v_hat)) / (1.0 + float(sum_n))
        x = [float(self.l[i]) + scale * (((q[i] if N[i] else v_mix) + 1.0) * 0.5) for i in range(n)]
        mx = max(x)
        e = [math.exp(v - mx) for v in x]
        total = 0.0
        for v in e:
            total += v
        pi = [v / total for v in e]
        target = np.array([int(math.floor(p * 65535.0 + 0.5)) for p in pi], dtype=np.int64)
        cand = N == max_n
        score = np.where(cand, rootP + scale * ((np.array(q) + 1.0) * 0.5), -np.inf)
        played = int(np.argmax(score))                 # first maximum
        gap = _gap(score, cand, played)
        self.min_gap = min(self.min_gap, gap)
        return dict(played=played, target=target, pi=np.array(pi), v_mix=v_mix, gap=gap, considered=self.k,
                    offprior=int(played != int(np.argmax(tP))), visited=int((N > 0).sum()), max_n=max_n, sum_n=sum_n,
                    unvisited_mass=float(sum(p for p, c in zip(pi, N) if c == 0)),
                    unvisited_with_target=int(((N == 0) & (target > 0)).sum()))

    def move_end(self, stats):
        r, fin = self.root(), self.finish()
        assert fin["sum_n"] == self.S == int(self.N[0])
        stats["gumbel_moves"] += 1
        stats["gumbel_considered"] += fin["considered"]
        stats["gumbel_offprior"] += fin["offprior"]
        stats["min_gap"] = min(stats["min_gap"], self.min_gap)
        fin["visits"] = r["visits"].copy()
        return fin["target"], fin["played"], fin        # no temperature, no uniform draw


def search(game, num_simulations, priors, g, gumbel, c_puct=1.5) -> GumbelSearch:
    return GumbelSearch(game, num_simulations, priors, g, gumbel, c_puct).run()


def play_game(cfg: dict, peaked: bool, seed, gumbel=None):
    import selfplay_model                              # it imports this module
    return selfplay_model.play_game(cfg, peaked, seed, gumbel=gumbel)
