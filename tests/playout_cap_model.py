"""Host model of a self-play game with playout cap randomization (include/xq_hip.h, xq_engine_init_cap), with and without tree
reuse.  TEST INFRASTRUCTURE ONLY: it judges k_select<.., true> / k_expand<.., true>.

It is tests/tree_reuse_model.py's game loop (imported, not edited) plus the rules of the cap:
  * every position that will be searched (not over, not adjudicated at max_game_length) takes one draw u of the uniform stream
    when its root request is issued -- BEFORE the resign probe of that root evaluation -- and the move is full iff u < p;
  * a full move is the move of tree_reuse_model.play_game: Dirichlet noise, budget S, a sample;
  * a fast move takes no Dirichlet draw, has no noise at the root (a fresh root is a root with add_noise = 0; a reused root keeps
    the kind it had as an inner node), runs until sims >= S_fast -- no new simulation when it inherits that many -- and records
    no sample; the move choice is unchanged;
  * the resign rule counts recorded samples.
With cap = None no cap draw is taken and the game is tree_reuse_model.play_game's (tests/test_playout_cap_model.py).
"""
from __future__ import annotations

import numpy as np

import leaf_batch_model as LB
import tree_reuse_model as M
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key


class FastSearch(M.ReuseSearch):
    """The search of a fast move: no root noise, budget `budget` <= num_simulations (which only sizes the arrays, so that a tree
    inherited from a full search fits)."""

    def __init__(self, game, num_simulations, budget, priors, kept=None, c_puct: float = 1.5):
        super().__init__(game, num_simulations, priors, None, kept, c_puct)
        self.budget = int(budget)

    def run(self):
        g = self.game
        legal = g.legal_actions()
        pri, kind, _ = self.priors(g.state_for_nn(), legal)
        if len(legal) == 0:
            return self
        if self.kept is None:
            self._expand(0, legal, pri, kind, False)
        else:
            n_nodes = len(self.kept["N"])
            for k in M.ARRAYS:
                getattr(self, k)[:n_nodes] = self.kept[k]
            self.alloc = n_nodes
            f, n = int(self.first[0]), int(self.nch[0])
            assert n == len(legal) and list(self.action[f:f + n]) == list(legal)
            assert int(self.kind[0]) == kind               # the kind it had as an inner node: same position, same evaluation
            if kind == 0:
                assert self.P32[f:f + n].tobytes() == np.asarray(pri, np.float32).tobytes()
                self.P32[f:f + n] = pri
            else:
                self.P64[f:f + n] = 1.0 / n
            self.reused = int(self.N[f:f + n].sum())
            self.N[0] = self.reused
            self.sims = self.reused
        self.start = {k: getattr(self, k)[:self.alloc].copy() for k in M.ARRAYS}
        while self.sims < self.budget:
            sim = g.clone()
            node, path = 0, [0]
            while self.nch[node] > 0:
                node = self._select(node)
                sim.make_action(int(self.action[node]))
                path.append(node)
            over, winner = sim.is_game_over()
            if over:
                self._backup(path, 0.0 if winner == 0 else 1.0)
            else:
                lg = sim.legal_actions()
                p, k, value = self.priors(sim.state_for_nn(), lg)
                self._expand(node, lg, p, k, False)
                self._backup(path, -float(np.float32(value)))
            self.sims += 1
        return self


class SplicedDraws(Draws):
    """Draws(seed) whose uniform stream has a dummy draw spliced in before every draw of the original stream: what a cap-on game
    with p = 1 must consume to replay the cap-off game of Draws(seed)."""

    def __init__(self, seed: int, dummy: float = 0.5):
        super().__init__(seed)
        self._odd, self._dummy = False, float(dummy)

    def uniform(self) -> float:
        self._odd = not self._odd
        return self._dummy if self._odd else super().uniform()


def _searchable(g, cfg):
    """The root request of g's position is issued with status 0: neither over nor adjudicated."""
    return not g.is_game_over()[0] and g.move_count < int(cfg["max_game_length"])


def play_game(cfg: dict, peaked: bool, draws, tree_reuse: bool = False, cap=None, on_move=None):
    """One self-play game on `draws` (a Draws, or a seed) -> (samples, winner, plies, stats).  cap = (p, S_fast) or None.
    stats: sims (new simulations), reused_visits, reroots, fast_moves, fast_sims, full_moves, and `moves`, one dict per search
    (full, reused, visits, new)."""
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
    stats = dict(sims=0, reused_visits=0, reroots=0, fast_moves=0, fast_sims=0, full_moves=0, moves=[])
    full = True
    if cap is not None and _searchable(g, cfg):
        full = d.uniform() < float(cap[0])                 # the first position's cap draw (no resign probe precedes a game)
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
            s = M.ReuseSearch(g, S, priors, noise, kept).run()
            new = S - s.reused
            stats["full_moves"] += 1
        else:
            s = FastSearch(g, S, int(cap[1]), priors, kept).run()
            new = max(0, int(cap[1]) - s.reused)
            stats["fast_moves"] += 1
            stats["fast_sims"] += new
        assert s.sims == s.reused + new
        stats["sims"] += new
        stats["reused_visits"] += s.reused
        stats["reroots"] += kept is not None
        r = s.root()
        stats["moves"].append(dict(full=full, reused=s.reused, visits=int(r["visits"].sum()), new=new))
        if full:
            samples.append(dict(board=g.board.reshape(90).copy(), player=g.current_player, actions=r["actions"].copy(),
                                visits=r["visits"].copy(), late=late))
        i = M.choose(r["actions"], r["visits"], late, d.uniform())
        c = int(s.first[0]) + i
        kept = s.reroot(c) if tree_reuse else None
        if on_move is not None:
            on_move(s, c, kept)
        g.make_action(int(r["actions"][i]))
        if cap is not None and _searchable(g, cfg):
            full = d.uniform() < float(cap[0])             # drawn when the root request is issued: before the resign probe
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
