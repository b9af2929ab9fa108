"""Pins of what the self-play host models (tests/*_model.py) compute: one SHA-256 per case over a canonical serialisation of
everything a case produces, recorded in tests/golden/host_model_pins.json.  The GPU tests judge the engine against these models,
so a change to a model that moves a single bit of a sample, a counter or a tree array must show here, on the CPU.

Whole games: every sample, winner, plies, the counters, the per-move records and -- through `on_move`, where the model offers
it -- every finished search's tree arrays up to `alloc`, its `start` snapshot and the re-rooted arrays.  Single searches: the
leaf-batched search, the perpetual-check search, the Gumbel search with handed values, the solver's search of crafted positions
and its arena games.  Floats go in as float.hex() or as their raw float64 bytes (float32 widens exactly), never rounded.

    python tests/test_host_model_pins.py --record      rewrites the JSON from the models as they stand

Record only from a tree whose models are known good; a refactor of the models must pass against the JSON as it was.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import forced_playouts_model as FP
import golden_io as G
import gumbel_model as GM
import leaf_batch_model as LB
import perpetual_check_model as PM
import playout_cap_model as PC
import solver_model as SM
import tree_reuse_model as M
from draws import Draws, Stream
from oracle import xq_oracle as O
from test_gumbel_gpu import CONFIGS, SEEDS
from test_solver_gpu import ARENA, S_SEARCH, _arena_openings, _candidates
from test_solver_model import GAMES, no_resign

PINS = os.path.join(G.GOLDEN, "host_model_pins.json")
TREE = ("N", "W", "P32", "P64", "first", "nch", "kind", "action")
TR_KEYS = ("sims", "reused_visits", "reroots")
PC_KEYS = TR_KEYS + ("fast_moves", "fast_sims", "full_moves")
FP_KEYS = PC_KEYS + ("forced_sims", "pruned_visits", "pruned_children")
GM_KEYS = ("sims", "gumbel_moves", "gumbel_considered", "gumbel_offprior", "min_gap")
SM_KEYS = PC_KEYS + ("terminal_sims", "fast_early", "draw_stops") + SM.COUNTERS
MOVE = ("full", "reused", "visits", "new")
GM_MOVE = ("played", "target", "pi", "v_mix", "gap", "considered", "offprior", "visited", "max_n", "sum_n", "unvisited_mass",
           "unvisited_with_target", "visits")
PRUNED = ("v", "d", "cstar", "N", "pruned_visits", "pruned_children")
SAMPLE = ("board", "player", "actions", "visits", "late", "z")


def feed(h, x):
    """Canonical bytes of x into h: tagged, so that no two different values serialise alike."""
    if x is None:
        h.update(b"n;")
    elif isinstance(x, (bool, np.bool_)):
        h.update(b"b1;" if x else b"b0;")
    elif isinstance(x, (int, np.integer)):
        h.update(b"i%d;" % int(x))
    elif isinstance(x, (float, np.floating)):
        h.update(b"f" + float(x).hex().encode() + b";")
    elif isinstance(x, str):
        h.update(b"s" + x.encode() + b";")
    elif isinstance(x, np.ndarray):
        wide = x.astype(np.float64) if x.dtype.kind == "f" else x.astype(np.int64)
        h.update(b"a" + x.dtype.kind.replace("u", "i").replace("b", "i").encode() + repr(x.shape).encode())
        h.update(np.ascontiguousarray(wide).tobytes())
    elif isinstance(x, dict):
        h.update(b"d%d;" % len(x))
        for k in sorted(x):
            feed(h, k)
            feed(h, x[k])
    elif isinstance(x, (list, tuple)):
        h.update(b"l%d;" % len(x))
        for v in x:
            feed(h, v)
    else:
        raise TypeError(type(x))


def pick(d, keys):
    return {k: d[k] for k in keys}


def tree(s, names=TREE):
    return {k: getattr(s, k)[:s.alloc] for k in names}


def search_hook(h, names=TREE):
    """An on_move that feeds every finished search: its tree, its first state, the chosen child and the re-rooted arrays."""
    def on_move(s, c, kept, *rest):
        feed(h, ("search", int(s.sims), int(s.reused), int(s.alloc), int(c), tree(s, names), pick(s.start, names),
                 None if kept is None else pick(kept, names + ("old_index",))))
    return on_move


def feed_game(h, result, stat_keys, move_keys=None, sample_keys=SAMPLE):
    samples, winner, plies, stats = result
    feed(h, ([pick(s, sample_keys) for s in samples], winner, plies, pick(stats, stat_keys)))
    if move_keys is not None:
        feed(h, [pick(m, move_keys) for m in stats["moves"]])


def cap_of(cfg, p):
    return None if p is None else (p, max(1, int(cfg["num_simulations"]) // 4))


def replay(actions):
    g = O.Game()
    for a in actions:
        g.make_action(int(a))
    return g


# ---- whole games ----------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name):
    def deco(f):
        assert name not in CASES
        CASES[name] = f
        return f
    return deco


def _whole_games():
    for cfg, peaked, seed, name in GAMES:
        for reuse in (False, True):
            tag = "%s-%s" % (name, "reuse" if reuse else "fresh")

            @case("tree_reuse-" + tag)
            def _(h, cfg=cfg, peaked=peaked, seed=seed, reuse=reuse):
                feed_game(h, M.play_game(cfg, peaked, seed, tree_reuse=reuse, on_move=search_hook(h)), TR_KEYS)

            for p in (0.25, 0.5):
                @case("playout_cap-%s-p%s" % (tag, p))
                def _(h, cfg=cfg, peaked=peaked, seed=seed, reuse=reuse, p=p):
                    feed_game(h, PC.play_game(cfg, peaked, seed, tree_reuse=reuse, cap=cap_of(cfg, p), on_move=search_hook(h)),
                              PC_KEYS, MOVE)

            @case("playout_cap-%s-spliced" % tag)
            def _(h, cfg=cfg, peaked=peaked, seed=seed, reuse=reuse):
                feed_game(h, PC.play_game(cfg, peaked, PC.SplicedDraws(seed), tree_reuse=reuse, cap=(1.0, 1),
                                          on_move=search_hook(h)), PC_KEYS, MOVE)

            for p in (None, 0.5):
                cap_tag = "nocap" if p is None else "cap"

                @case("forced-%s-%s" % (tag, cap_tag))
                def _(h, cfg=cfg, peaked=peaked, seed=seed, reuse=reuse, p=p):
                    r = FP.play_game(cfg, peaked, seed, tree_reuse=reuse, cap=cap_of(cfg, p), forced=2.0, on_move=search_hook(h))
                    feed_game(h, r, FP_KEYS, MOVE)
                    feed(h, [pick(pr, PRUNED) for pr in r[3]["pruned"]])

                @case("solver-%s-%s" % (tag, cap_tag))
                def _(h, cfg=cfg, peaked=peaked, seed=seed, reuse=reuse, p=p):
                    r = SM.play_game(no_resign(cfg), peaked, seed, tree_reuse=reuse, cap=cap_of(cfg, p),
                                     on_move=search_hook(h, TREE + ("state",)))
                    feed_game(h, r, SM_KEYS, MOVE + ("early",), SAMPLE + ("proven",))

    for reuse in (False, True):
        @case("playout_cap-two_games_one_stream-%s" % ("reuse" if reuse else "fresh"))
        def _(h, reuse=reuse):
            cfg, peaked, seed, name = GAMES[0]
            assert name == "resign" and cfg["enable_resign"]
            d = Draws(seed)
            for _ in range(2):
                feed_game(h, PC.play_game(cfg, peaked, d, tree_reuse=reuse, cap=(0.5, 6), on_move=search_hook(h)), PC_KEYS, MOVE)

    for cfg, peaked, seed, name in CONFIGS:
        for m in (4, 16):
            @case("gumbel-%s-m%d" % (name, m))
            def _(h, cfg=cfg, peaked=peaked, seed=SEEDS.get((name, m), seed), m=m):
                feed_game(h, GM.play_game(cfg, peaked, seed, gumbel=(m, 50.0, 1.0)), GM_KEYS, GM_MOVE)


_whole_games()


# ---- single searches -----------------------------------------------------------------------------------------------------------
def feed_leaf_search(h, s):
    feed(h, (s.root(), int(s.steps), list(s.leaves_per_step), int(s.collisions), int(s.terminal_sims), int(s.sims), tree(s)))


for _K in (1, 2, 4, 8):
    for _S in (16, 100):
        @case("leaf_batch-K%d-S%d" % (_K, _S))
        def _(h, K=_K, S=_S):
            """Every recorded position of that S: both stubs, with and without root noise."""
            traces = [t for t in G.mcts_traces() if t["sims"] == S]
            assert {(t["stub"], t["eta"] is None) for t in traces} == {(a, b) for a in ("flat", "peaked") for b in (False, True)}
            for t in traces:
                noise = None if t["eta"] is None else np.array([G.hexf(x) for x in t["eta"]])
                s = LB.LeafBatchSearch(replay(t["actions"]), S, K, LB.stub_priors(t["stub"] == "peaked"), noise=noise).run()
                feed_leaf_search(h, s)
                if t is traces[0]:                     # the module's function is the class's root()
                    feed(h, LB.search(replay(t["actions"]), S, K, LB.stub_priors(t["stub"] == "peaked"), noise=noise))

    for _rule in (False, True):
        if _K in (1, 4):
            @case("perpetual-K%d-%s" % (_K, "on" if _rule else "off"))
            def _(h, K=_K, rule=_rule):
                for g in (PM.pc_red(11), PM.pc_black(11), PM.quiet(11), PM.pc_red_rotated(11),
                          PM.cycle_game(PM.MATE_IN_ONE, [], 0)):
                    feed_leaf_search(h, PM.PerpetualSearch(g, 64, K, PM.uniform_priors, rule).run())
                    feed(h, PM.search(g, 64, K, PM.uniform_priors, rule))


@case("gumbel-search_only")
def _(h):
    d = G.corpus()
    picks = [i for i in range(5, len(d["board"]), 70) if not d["done"][i]][:16]
    games = [O.Game()] + [replay(d["taken"][i - d["ply"][i]:i]) for i in picks]
    priors = LB.stub_priors(True)
    for slot, g in enumerate(games):
        gs = GM.injected_gumbels(Stream(700 + slot, 3), len(g.legal_actions()))
        s = GM.search(g, 32, priors, gs, (8, 50.0, 1.0))
        feed(h, (s.root(), s.finish(), s.v_hat, s.l, s.min_gap, int(s.sims), tree(s)))


def _crafted_positions():
    games = _candidates(7, 6, 1) + _candidates(8, 3, -1) + _candidates(9, 2, 1, 119)
    return games + [SM.crafted_game([(1, 5, 1), (1, 7, 5), (3, 6, 5), (7, 3, -1)])]


for _solver in (False, True):
    @case("solver-search_position-%s" % ("on" if _solver else "off"))
    def _(h, solver=_solver):
        for g in _crafted_positions():
            n = len(g.legal_actions())
            for noise in (np.full(n, 1.0 / n), None):
                s = SM.search_position(g, S_SEARCH, noise=noise, solver=solver)
                feed(h, (s.root(), s.root_states(), s.final_counts(), int(s.sims), s.early, int(s.budget), int(s.proven_nodes),
                         int(s.proven_stops), int(s.terminal_sims), int(s.draw_stops), int(s.max_propagation),
                         tree(s, TREE + ("state",)), pick(s.start, TREE + ("state",))))

    for _options in (False, True):
        @case("solver-arena-%s-%s" % ("arena_opts" if _options else "plain", "on" if _solver else "off"))
        def _(h, solver=_solver, options=_options):
            _, openings = _arena_openings(options)
            pri = (LB.stub_priors(True), LB.stub_priors(False))
            for g in range(ARENA["games"]):
                winner, plies, moves, stats = SM.arena_game(pri, g % 2 == 0, ARENA["sims"], ARENA["max_len"], solver=solver,
                                                            opening=openings[g])
                feed(h, (winner, plies, [list(m) for m in moves], stats))


def digest(name):
    h = hashlib.sha256()
    CASES[name](h)
    return h.hexdigest()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_output_is_pinned(name):
    pins = json.load(open(PINS))
    assert set(pins) == set(CASES)
    assert digest(name) == pins[name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    with open(PINS, "w") as f:
        json.dump({name: digest(name) for name in sorted(CASES)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(CASES), "digests in", PINS)
