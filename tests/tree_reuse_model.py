"""Host model of a self-play game with tree reuse across moves (include/xq_hip.h, XQ_ENGINE_TREE_REUSE).  TEST INFRASTRUCTURE
ONLY: it judges k_select<true> / k_reroot / k_expand<true>.

The game loop is tests/selfplay_model.py's, the one loop of every self-play model (the oracle's, with the draws injected).  The
search, `ReuseSearch`, is the one sequential search of a move: the K = 1 search of tests/leaf_batch_model.py (oracle rules, the
oracle's PUCT arithmetic, its descent and its terminal test), which test_leaf_batch_model.py pins against the reference; the
searches of the other options subclass it.  With reuse off the model is the oracle's game (tests/test_tree_reuse_model.py checks
that on every recorded game).

With reuse on, when a move ends the chosen child c, if it was expanded, becomes the next search's root with its subtree:
  * the arena is compacted as k_reroot does it -- c at node 0, its descendants in their old order from node 1 on;
  * the root request still happens: the children's float32 priors are rewritten from the root evaluation, fresh noise goes into
    the float64 root priors (kind 1), and the search starts at sims = root N = the sum of the children's visits;
  * the search stops at S visits, as always.
"""
from __future__ import annotations

import numpy as np

import leaf_batch_model as LB

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
    """The K = 1 search of one move.  `kept` (from `reroot`) starts it from the previous move's subtree; `noise` None is a root
    without noise (a fast move, an arena move); it runs until sims >= `budget` <= num_simulations (which sizes the arrays, so
    that a tree inherited from a full search fits)."""

    ARRAYS = ARRAYS                                    # what `reroot` hands to the next search

    def __init__(self, game, num_simulations, priors, noise, kept=None, c_puct: float = 1.5, noise_eps: float = 0.25,
                 budget=None):
        super().__init__(game, num_simulations, 1, priors, c_puct, noise, noise_eps)
        self.kept = kept
        self.budget = self.S if budget is None else int(budget)
        self.reused = 0

    def _expand_root(self, legal, pri, kind, value):
        self._expand(0, legal, pri, kind, self.noise is not None)

    def _root_setup(self):
        """Expands a fresh root, or takes `kept` over and redoes what the root request does to it -> False without a legal move."""
        legal = self.game.legal_actions()
        pri, kind, value = self.priors(self.game.state_for_nn(), legal)
        if len(legal) == 0:
            return False
        if self.kept is None:
            self._expand_root(legal, pri, kind, value)
            return True
        n_nodes = len(self.kept["N"])
        for k in self.ARRAYS:
            getattr(self, k)[:n_nodes] = self.kept[k]
        self.alloc = n_nodes
        f, n = int(self.first[0]), int(self.nch[0])
        assert n == len(legal) and list(self.action[f:f + n]) == list(legal)
        if kind == 0:
            assert self.P32[f:f + n].tobytes() == np.asarray(pri, np.float32).tobytes()   # same position, same priors
            self.P32[f:f + n] = pri
        if self.noise is not None:
            self.P64[f:f + n] = self._noisy(pri, kind, n)
            self.kind[0] = 1
        else:
            assert int(self.kind[0]) == kind               # the kind it had as an inner node: same position, same evaluation
            if kind != 0:
                self.P64[f:f + n] = 1.0 / n
        self.reused = int(self.N[f:f + n].sum())
        self.N[0] = self.reused
        self.sims = self.reused
        return True

    def _finished(self):
        return self.sims >= self.budget

    def run(self):
        if not self._root_setup():
            return self
        self.start = {k: getattr(self, k)[:self.alloc].copy() for k in self.ARRAYS}    # the first search state of this move
        while not self._finished():
            sim = self.game.clone()
            path = self._descend(sim)
            v = self._terminal(sim, path)
            if v is None:
                lg = sim.legal_actions()
                p, k, value = self.priors(sim.state_for_nn(), lg)
                self._expand(path[-1], lg, p, k, False)
                v = -float(np.float32(value))
            else:
                self.terminal_sims += 1
            self._backup(path, v)
            self.sims += 1
        return self

    def reroot(self, c):
        """The arrays of the next search's tree when child c becomes its root, or None when c was never expanded."""
        if self.first[c] < 0:
            return None
        order = compaction_order(self.first, self.nch, c, self.alloc)
        out = {k: getattr(self, k)[order].copy() for k in self.ARRAYS}
        out["first"] = remap_first(self.first, order)
        out["old_index"] = order
        return out

    def move_end(self, stats):
        """The end of a self-play move: adds this search's own counters to `stats` -> (the visit counts the sample records and the
        move is drawn from, the child the move is already decided on or None, what the search adds to the move's record)."""
        return self.root()["visits"], None, {}


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


def play_game(cfg: dict, peaked: bool, seed, tree_reuse: bool = False, on_move=None):
    import selfplay_model                              # it imports this module
    return selfplay_model.play_game(cfg, peaked, seed, tree_reuse=tree_reuse, on_move=on_move)
