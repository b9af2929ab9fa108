"""Host model of a self-play game with tree reuse across moves (include/xq_hip.h, XQ_ENGINE_TREE_REUSE).  TEST INFRASTRUCTURE
ONLY: it judges k_select<true> / k_reroot / k_expand<true>.

The game loop is the oracle's (oracle/xq_oracle.c, xqo_play_one_game: random opening, adjudication, Dirichlet noise per move,
sample, move from the visit counts, resign probe) with the draws injected (tests/draws.py).  The search is the K = 1 search of
tests/leaf_batch_model.py (oracle rules, the oracle's PUCT arithmetic), which test_leaf_batch_model.py pins against the
reference.  With reuse off the model is the oracle's game (tests/test_tree_reuse_model.py checks that on every recorded game).

With reuse on, when a move ends the chosen child c, if it was expanded, becomes the next search's root with its subtree:
  * the arena is compacted as k_reroot does it -- c at node 0, its descendants in their old order from node 1 on;
  * the root request still happens: the children's float32 priors are rewritten from the root evaluation, fresh noise goes into
    the float64 root priors (kind 1), and the search starts at sims = root N = the sum of the children's visits;
  * the search stops at S visits, as always.
"""
from __future__ import annotations

import numpy as np

import leaf_batch_model as LB
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key

ARRAYS = ("N", "W", "P32", "P64", "first", "nch", "kind", "action")


def compaction_order(first, nch, c, mark):
    """Old index of every node of the re-rooted arena: c, then c's descendants in ascending old index (k_reroot's stable
    compaction).  Validates the arena invariants the kernel relies on."""
    kept = np.zeros(int(mark), dtype=bool)
    stack = [int(c)]
    while stack:
        x = stack.pop()
        f, n = int(first[x]), int(nch[x])
        if f < 0:
            continue
        assert x < f and n > 0 and f + n <= mark, (x, f, n, mark)
        assert not kept[f:f + n].any()
        kept[f:f + n] = True
        stack.extend(range(f, f + n))
    return np.concatenate([[int(c)], np.nonzero(kept)[0]]).astype(np.int64)


def remap_first(first_old, order):
    """First-child words of the compacted arena (nodes in `order`): -1 stays -1, an old index maps to its new one."""
    new_of = {int(o): i for i, o in enumerate(order)}
    return np.array([-1 if int(first_old[o]) < 0 else new_of[int(first_old[o])] for o in order], dtype=np.int64)


class ReuseSearch(LB.LeafBatchSearch):
    """The K = 1 search of one move; `kept` (from `reroot`) starts it from the previous move's subtree."""

    def __init__(self, game, num_simulations, priors, noise, kept=None, c_puct: float = 1.5, noise_eps: float = 0.25):
        super().__init__(game, num_simulations, 1, priors, c_puct, noise, noise_eps)
        self.kept = kept
        self.reused = 0

    def run(self):
        g = self.game
        legal = g.legal_actions()
        pri, kind, _ = self.priors(g.state_for_nn(), legal)
        if len(legal) == 0:
            return self
        if self.kept is None:
            self._expand(0, legal, pri, kind, True)
        else:
            n_nodes = len(self.kept["N"])
            for k in ARRAYS:
                getattr(self, k)[:n_nodes] = self.kept[k]
            self.alloc = n_nodes
            f, n = int(self.first[0]), int(self.nch[0])
            assert n == len(legal) and list(self.action[f:f + n]) == list(legal)
            eta = np.asarray(self.noise, dtype=np.float64)[:n]
            if kind == 0:
                assert self.P32[f:f + n].tobytes() == np.asarray(pri, np.float32).tobytes()   # same position, same priors
                self.P32[f:f + n] = pri
                self.P64[f:f + n] = (np.float32(1.0 - self.eps) * pri).astype(np.float32).astype(np.float64) + self.eps * eta
            else:
                self.P64[f:f + n] = (1.0 - self.eps) * (1.0 / n) + self.eps * eta
            self.kind[0] = 1
            self.reused = int(self.N[f:f + n].sum())
            self.N[0] = self.reused
            self.sims = self.reused
        self.start = {k: getattr(self, k)[:self.alloc].copy() for k in ARRAYS}    # the first search state of this move
        while self.sims < self.S:
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

    def reroot(self, c):
        """The arrays of the next search's tree when child c becomes its root, or None when c was never expanded."""
        if self.first[c] < 0:
            return None
        order = compaction_order(self.first, self.nch, c, self.alloc)
        out = {k: getattr(self, k)[order].copy() for k in ARRAYS}
        out["first"] = remap_first(self.first, order)
        out["old_index"] = order
        return out


def choose(actions, visits, late: bool, u: float, late_temperature: float = 0.3) -> int:
    """Index of the played child: np.random.choice over the dense pi (action-id order) with the injected uniform, as the
    engine computes it (mcts.py:190-206, numpy's cdf / searchsorted)."""
    order = np.argsort(np.asarray(actions, dtype=np.int64), kind="stable")
    inv_t = 1.0 / late_temperature
    w = [(float(visits[i]) ** inv_t if visits[i] > 0 else 0.0) if late else float(visits[i]) for i in order]
    total = 0.0
    for x in w:
        total += x
    last = 0.0
    for x in w:
        last += x / total
    run = 0.0
    for j, x in enumerate(w):
        run += x / total
        if run / last > u:
            return int(order[j])
    return int(order[-1])


def play_game(cfg: dict, peaked: bool, seed: int, tree_reuse: bool = False, on_move=None):
    """One self-play game with Draws(seed) -> (samples, winner, plies, stats).  samples: dicts with board, player, actions,
    visits, late, z.  `on_move(search, chosen_child, next_kept)` is called after every search (tests)."""
    d = Draws(seed)
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
    stats = dict(sims=0, reused_visits=0, reroots=0)
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
        noise = d.dirichlet(len(g.legal_actions()))
        s = ReuseSearch(g, S, priors, noise, kept).run()
        stats["sims"] += S - s.reused
        stats["reused_visits"] += s.reused
        stats["reroots"] += kept is not None
        r = s.root()
        samples.append(dict(board=g.board.reshape(90).copy(), player=g.current_player, actions=r["actions"].copy(),
                            visits=r["visits"].copy(), late=late))
        i = choose(r["actions"], r["visits"], late, d.uniform())
        c = int(s.first[0]) + i
        kept = s.reroot(c) if tree_reuse else None
        if on_move is not None:
            on_move(s, c, kept)
        g.make_action(int(r["actions"][i]))
        if cfg["enable_resign"] and len(samples) > 10:
            _, v = predict_from_key(state_key(g.state_for_nn()), peaked)
            resign_hist.append(v)
            K = int(cfg["resign_check_steps"])
            if len(resign_hist) >= K and all(x < float(cfg["resign_threshold"]) for x in resign_hist[-K:]):
                winner = -g.current_player                 # a pending re-root is not counted: no search follows
                break
    for smp in samples:
        smp["z"] = 0 if winner == 0 else (1 if winner == smp["player"] else -1)
    return samples, winner, g.move_count, stats
