"""The one self-play game loop of the host models.  TEST INFRASTRUCTURE ONLY: tree_reuse_model, playout_cap_model,
forced_playouts_model, gumbel_model and solver_model each keep their search and their rules; their `play_game` is this one.

The loop is the oracle's (oracle/xq_oracle.c, xqo_play_one_game: random opening, adjudication, Dirichlet noise per move, sample,
move from the visit counts, resign probe) with the draws injected (tests/draws.py).  With every option off it is the oracle's game
(tests/test_tree_reuse_model.py checks that on every recorded game); what it computes under each option is pinned digest for
digest in tests/test_host_model_pins.py.  What an option changes in a move sits with its search (`move_end`); the loop knows
  * tree reuse: the chosen child's subtree, when it was expanded, starts the next search;
  * the playout cap: one uniform draw per position that will be searched, taken when its root request is issued -- after the move
    that leads to it, BEFORE the resign probe -- the move is full iff u < p; a fast move takes no Dirichlet draw, runs to S_fast
    and records no sample;
  * Gumbel: the move's values come from the raw Dirichlet stream, the search decides the move (no uniform draw), late = False.
"""
from __future__ import annotations

import math

import forced_playouts_model as FP
import gumbel_model as GM
import leaf_batch_model as LB
import solver_model as SM
import tree_reuse_model as M
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key


def _searchable(g, cfg):
    """The root request of g's position is issued with status 0: neither over nor adjudicated."""
    return not g.is_game_over()[0] and g.move_count < int(cfg["max_game_length"])


def play_game(cfg: dict, peaked: bool, draws, *, tree_reuse=False, cap=None, forced=None, gumbel=None, solver=False, on_move=None):
    """One self-play game on `draws` (a Draws, or a seed) -> (samples, winner, plies, stats).  cap = (p, S_fast), forced = k,
    gumbel = (m, c_visit, c_scale), or None.  samples: dicts with board, player, actions, visits, late, z and `proven` (1: the
    solver's rule 4 ended the move).  stats: sims (new simulations), terminal_sims, reused_visits, reroots, full_moves,
    fast_moves, fast_sims, every option's own counters (zero when it is off), `pruned` (forced playouts: pruned() of every full
    move) and `moves`, one dict per search (full, reused, visits, new, and what the search adds).  `on_move(search, chosen_child,
    next_kept, game)` is called after every search, before the move is made (tests)."""
    if gumbel is not None and (tree_reuse or cap is not None or forced is not None or solver):
        raise ValueError("the Gumbel root search excludes tree reuse, the playout cap, forced playouts and the solver")
    if solver and forced is not None:
        raise ValueError("the solver excludes forced playouts")
    d = Draws(draws) if isinstance(draws, int) else draws
    priors = LB.stub_priors(peaked)
    S, c_puct = int(cfg["num_simulations"]), float(cfg["c_puct"])
    g = O.Game()
    for _ in range(d.randint(0, int(cfg["random_opening_moves"]))):
        legal = g.legal_actions()
        if len(legal) == 0:
            break
        g.make_action(int(legal[d.choice_index(len(legal))]))
        if g.is_game_over()[0]:
            g = O.Game()
            break

    def next_is_full():
        """The cap draw of g's position; none without the cap or before a position that will not be searched."""
        return cap is None or not _searchable(g, cfg) or d.uniform() < float(cap[0])

    samples, resign_hist, kept = [], [], None
    stats = dict(sims=0, terminal_sims=0, reused_visits=0, reroots=0, fast_moves=0, fast_sims=0, full_moves=0, moves=[],
                 forced_sims=0, pruned_visits=0, pruned_children=0, pruned=[],
                 gumbel_moves=0, gumbel_considered=0, gumbel_offprior=0, min_gap=math.inf,
                 fast_early=0, draw_stops=0, **{k: 0 for k in SM.COUNTERS})
    full = next_is_full()                              # the first position's (no resign probe precedes a game)
    while True:
        over, w = g.is_game_over()
        if over:
            winner = w
            break
        if g.move_count >= int(cfg["max_game_length"]):
            diff = O.material(g.board, 1) - O.material(g.board, -1)
            winner = 1 if diff > 30 else (-1 if diff < -30 else 0)
            break
        late = gumbel is None and g.move_count >= int(cfg["temperature_threshold"])
        budget = S if full else int(cap[1])
        n = len(g.legal_actions())
        if gumbel is not None:
            s = GM.GumbelSearch(g, S, priors, GM.injected_gumbels(d.s_dirichlet, n), gumbel, c_puct)
        else:
            noise = d.dirichlet(n) if full else None
            if solver:
                s = SM.SolverSearch(g, S, priors, noise, kept, budget, c_puct=c_puct)
            elif forced is not None and full:
                s = FP.ForcedSearch(g, S, priors, noise, kept, forced, c_puct)
            else:
                s = M.ReuseSearch(g, S, priors, noise, kept, c_puct, budget=budget)
        s.run()
        visits, i, record = s.move_end(stats)
        new = s.sims - s.reused
        assert new == max(0, budget - s.reused) or (solver and i is not None)      # only rule 4 ends a search early
        stats["full_moves" if full else "fast_moves"] += 1
        if not full:
            stats["fast_sims"] += new
        stats["sims"] += new
        stats["terminal_sims"] += s.terminal_sims
        stats["reused_visits"] += s.reused
        stats["reroots"] += kept is not None
        r = s.root()
        stats["moves"].append({**dict(full=full, reused=s.reused, visits=int(r["visits"].sum()), new=new), **record})
        if full:
            samples.append(dict(board=g.board.reshape(90).copy(), player=g.current_player, actions=r["actions"].copy(),
                                visits=visits.copy(), late=late, proven=int(solver and i is not None)))
        if i is None:
            i = M.choose(r["actions"], visits, late, d.uniform())
        c = int(s.first[0]) + i
        kept = s.reroot(c) if tree_reuse else None
        if on_move is not None:
            on_move(s, c, kept, g)
        g.make_action(int(r["actions"][i]))
        full = next_is_full()                          # drawn when the root request is issued: before the resign probe
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
