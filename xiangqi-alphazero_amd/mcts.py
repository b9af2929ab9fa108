"""Serving shim -- the reference's `MCTS` call shape (training/mcts.py:76-206) on the engine, for single-game callers
(the demos' `mcts.search(game, temperature=0.1, add_noise=False)`, `train.py`'s serial paths).

    mcts = MCTS(model, num_simulations=200, c_puct=1.5)
    pi = mcts.search(game, temperature=1.0, add_noise=True)      # float64[8100], same as the reference
    a  = mcts.get_action(game, temperature=0)

`game` is duck-typed like the reference's `XiangqiGame`: `.board` (int8[10,9]), `.current_player`, `.move_count`,
`.no_capture_count`, `.history` (list of the pre-move boards as 90-byte `bytes`).  `n_parallel` positions can be
searched at once with `search_many`.  One slot of a search-only engine (`manual_moves = 1`) per position; the network
is evaluated on the GPU.  With `add_noise=True` the root noise comes from the device Dirichlet(0.3) generator.

`leaves_per_step = K > 1` (opt-in, K <= 64) batches up to K leaves per position and step under virtual loss
(engine.SelfPlayEngine): a search of S simulations takes about S / K + 1 steps instead of S + 1.  It is knowingly not the
reference's sequential search (the visit counts differ); K = 1 is.

`perpetual_check=True` (opt-in) searches under the perpetual-check rule (engine.SelfPlayEngine): a
repetition one side forced by checking on every move is that side's loss at the root and at every leaf, not a draw.

`solver=True` (opt-in) searches with proven results (engine.SelfPlayEngine): `get_action` at temperature 0
returns the proven winning move when the search found one, and never a move shown to lose while another is not (`solver_choice`
over the root's visits and `read_root_states`); `search`'s pi stays the visit counts'.

`search_many(..., return_values=True)` also returns the search's value of every position, from the view of its side to move
(`root_value`: the engine's root_q arithmetic of DESIGN.md section 4.13 over `read_root`'s arrays); `root_values` keeps the last
search's.

`eval_mirror=True` (opt-in) evaluates every request of the search under a randomly chosen left-right orientation
(engine.SelfPlayEngine).  The orientation is a function of the seed, the position's index in the call, its
`move_count` and the request's place in the search, so the same call gives the same answer again: serving stays reproducible.

`eval_dedup=True` (opt-in) evaluates every distinct position of a `search_many` step once (engine.SelfPlayEngine, DESIGN.md
section 4.24): equal positions among the `n_parallel`, and searches that walk into the same position in the same step, share one
row of the network's batch.  The visit counts are those of the search without it.

`early_stop=True` (opt-in) lets `get_action(temperature=0)` end its search as soon as the first choice is fixed
(engine.SelfPlayEngine): a forced move, or a leader the simulations that are left cannot catch.  The action
is the full search's, always.  `search` / `search_many`, at any temperature, keep the full search: their pi and `root_value` are
functions of all S simulations.  Not with leaves_per_step > 1 or solver.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from . import engine, evaluator as ev_mod
from .sample_format import ACTION_SPACE, dense_pi


def solver_choice(actions, visits, child_states) -> int:
    """The move a solver engine's root gives at temperature 0 (`child_states`: engine.read_root_states' code, +1 wins, -1 loses):
    the first proven win; else the first maximum of the visits over the moves not shown to lose; else, every move lost, the
    first maximum of the visits."""
    st, v = np.asarray(child_states), np.asarray(visits, dtype=np.int64)
    wins = np.nonzero(st == 1)[0]
    if len(wins):
        return int(actions[wins[0]])
    if (st != -1).any():
        v = np.where(st == -1, -1, v)
    return int(actions[int(np.argmax(v))])


def root_value(visits, total_value) -> np.float32:
    """The root's search value from the view of the side to move, as an engine with root_stats=True records it
    (include/xq_hip.h, xq_engine_init_rs): one sequential float64 sum of the children's W in move order over the sum of their N,
    cast to float32 once; 0.0 for a position without legal moves or without visits."""
    sum_w, sum_n = 0.0, 0
    for w, n in zip(np.asarray(total_value, dtype=np.float64).tolist(), np.asarray(visits).tolist()):
        sum_w += w
        sum_n += int(n)
    return np.float32(sum_w / float(sum_n)) if sum_n > 0 else np.float32(0.0)


def as_mcts(model_or_evaluator, num_simulations: int, c_puct: float, device, evaluator_kind: str, **options) -> "MCTS":
    """What a yardstick searches with: `model_or_evaluator` itself when the caller built the `MCTS` (its simulations and options
    hold, `early_stop` for one), else a new `MCTS` of the model or evaluator with `options`."""
    if isinstance(model_or_evaluator, MCTS):
        return model_or_evaluator
    return MCTS(model_or_evaluator, num_simulations, c_puct, device, evaluator_kind, **options)


class MCTS:
    def __init__(self, model, num_simulations: int = 200, c_puct: float = 1.5, device: str = "cuda",
                 evaluator_kind: str = "auto", seed: int = 0, leaves_per_step: int = 1, perpetual_check: bool = False,
                 solver: bool = False, eval_mirror: bool = False, eval_dedup: bool = False, early_stop: bool = False):
        if not 1 <= int(leaves_per_step) <= 64:
            from .hip import XqError
            raise XqError(f"leaves_per_step must be in [1, 64], got {leaves_per_step}")
        self.leaves_per_step = int(leaves_per_step)
        self.perpetual_check = bool(perpetual_check)
        self.solver = bool(solver)
        self.eval_mirror = bool(eval_mirror)
        self.eval_dedup = bool(eval_dedup)
        # checked here, without a GPU: the engines are made at the first search
        self.early_stop = engine.parse_early_stop(engine.make_config(1, int(num_simulations), manual_moves=1), early_stop,
                                                  leaves_per_step=self.leaves_per_step, solver=self.solver)
        self.model = model
        self.num_simulations = num_simulations
        self.c_puct = c_puct
        self.device = device
        self.seed = seed
        self.evaluator = model if callable(model) and not hasattr(model, "state_dict") else \
            ev_mod.make_evaluator(model, device, evaluator_kind)[0]
        self._engines = {}
        self.root_values = np.zeros(0, dtype=np.float32)      # the last search's root value per position

    def refresh(self, model=None):
        """Re-fold the weights after the caller changed its model in place (or hand over a new one).  The reference's
        MCTS reads the live model on every `.predict`; this shim snapshots BN-folded / pre-transformed weights, so a
        caller that keeps training between searches calls this first."""
        if model is not None:
            self.model = model
        if hasattr(self.evaluator, "update") and hasattr(self.model, "state_dict"):
            self.evaluator.update(self.model)

    def _engine(self, n: int, add_noise: bool, early_stop: bool = False):
        key = (n, add_noise, True) if early_stop else (n, add_noise)      # the full searches' engines keep their two-part key
        if key not in self._engines:
            cfg = engine.make_config(n, self.num_simulations, c_puct=self.c_puct, add_noise=add_noise, manual_moves=1,
                                     seed=self.seed)
            self._engines[key] = engine.SelfPlayEngine(cfg, self.device, evaluator=self.evaluator,
                                                       leaves_per_step=self.leaves_per_step,
                                                       perpetual_check=self.perpetual_check, solver=self.solver,
                                                       eval_mirror=self.eval_mirror, eval_dedup=self.eval_dedup,
                                                       early_stop=early_stop)
        return self._engines[key]

    def search_many(self, games: Sequence, temperature: float = 1.0, add_noise: bool = True, return_values: bool = False):
        """pi float64[8100] per position; with `return_values` (pis, float32[len(games)]): the search's value of every position
        as well (`root_value`), which `root_values` holds after any search."""
        out, values = self._search(games, temperature, add_noise, False)
        return (out, values) if return_values else out

    def _search(self, games: Sequence, temperature: float, add_noise: bool, early_stop: bool):
        """`search_many` on the engine keyed by `early_stop` -> (pis, values).  With it a search may hold before S simulations,
        so the engine is stepped in chunks of 8 with a test after each from the start."""
        eng = self._engine(len(games), add_noise, early_stop)
        for slot, g in enumerate(games):
            hist = [np.frombuffer(h, dtype=np.int8) for h in list(g.history)[-12:]]
            eng.set_position(slot, np.asarray(g.board, dtype=np.int8), int(g.current_player), int(g.move_count),
                             int(g.no_capture_count), np.stack(hist) if hist else None)
        # the root, then S simulations in at least ceil(S / K) steps; collisions (K > 1) and long runs of terminal leaves
        # can add steps, so the engine is stepped on in small chunks until every slot holds its finished search
        K = self.leaves_per_step
        blind = 0 if early_stop else -(-self.num_simulations // K) + 1      # a search that may settle is tested from the start
        for _ in range(blind):
            eng.step()
        extra, limit = 0, 4 * self.num_simulations + 64 + (self.num_simulations + 8 if early_stop else 0)
        while not eng.held():
            for _ in range(8):
                eng.step()
            extra += 8
            if extra > limit:
                raise RuntimeError("search did not finish")
        out = []
        values = np.zeros(len(games), dtype=np.float32)
        for slot in range(len(games)):
            r = eng.read_root(slot)
            values[slot] = root_value(r["visits"], r["total_value"])
            if len(r["actions"]) == 0:
                out.append(np.zeros(ACTION_SPACE))                       # mcts.py:111-112
            else:
                out.append(dense_pi(r["actions"], r["visits"].astype(np.float64), temperature))
        self.root_values = values
        return out, values

    def search_decided(self, games: Sequence, add_noise: bool = False):
        """The searches behind the temperature-0 moves of many positions -> the engine whose slot i holds the search of games[i]
        (`read_root`; the move is the first maximum of its visits in move order).  With `early_stop` a search may have ended
        before S simulations: its first maximum is the full search's, its other counts are not.  What `get_action(temperature=0)`
        runs for one position, and what the yardsticks (baseline, tactics, endgame) run for many."""
        self._search(games, 0.0, add_noise, self.early_stop)
        return self._engine(len(games), add_noise, self.early_stop)

    def search(self, game, temperature: float = 1.0, add_noise: bool = True) -> np.ndarray:
        return self.search_many([game], temperature, add_noise)[0]

    def get_action(self, game, temperature: float = 0.0, add_noise: bool = False) -> int:
        """mcts.py:166-174"""
        probs = self._search([game], temperature, add_noise, self.early_stop and temperature == 0)[0][0]
        if temperature == 0 and self.solver:
            eng = self._engine(1, add_noise)           # the engine `search` just used: slot 0 holds the finished search
            r = eng.read_root(0)
            if len(r["actions"]):
                return solver_choice(r["actions"], r["visits"], eng.read_root_states(0)["children"])
        if temperature == 0:
            return int(np.argmax(probs))
        return int(np.random.choice(len(probs), p=probs))
