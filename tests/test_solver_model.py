"""The host model of the proven-result search (tests/solver_model.py) against what it is built on, on the CPU:

* with the solver off it is tests/playout_cap_model.py's game on every recorded game, tree reuse and the cap off and on;
* after every search of the solver-on games the states are consistent (a WIN child implies a LOSS parent, a parent without an
  UNKNOWN child has the derived state, no UNKNOWN parent has a WIN child), and every decided node within three plies of the root
  agrees with a brute-force minimax over the oracle's rules, run to the height of the node's own proof;
* the games the GPU tests compare prove something: over them proven_nodes, proven_stops and proven_moves are each > 0, and the
  game that decides nothing equals the solver-off model record for record.
"""
import numpy as np
import pytest

import golden_io as G
import playout_cap_model as PC
import solver_model as SM

_LONG = dict(num_simulations=100, c_puct=1.5, temperature_threshold=10, max_game_length=70, random_opening_moves=4,
             enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
GAMES = [(t["cfg"], t["stub"] == "peaked", t["seed"], t["name"]) for t in G.game_traces()] + [(_LONG, True, 31, "long_peaked")]
IDS = [g[3] for g in GAMES]


def no_resign(cfg):
    """The configuration the solver games are compared under: a game that would resign first goes on to where nodes are decided."""
    return dict(cfg, enable_resign=False)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert bytes(x["board"]) == bytes(y["board"]) and x["player"] == y["player"] and x["late"] == y["late"] and x["z"] == y["z"]
        assert list(x["actions"]) == list(y["actions"]) and list(x["visits"]) == list(y["visits"])


@pytest.mark.parametrize("cap", [None, 0.5], ids=["nocap", "cap"])
@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
@pytest.mark.parametrize("game", GAMES, ids=IDS)
def test_solver_off_is_the_playout_cap_model(game, reuse, cap):
    c, peaked, seed, _ = game
    cap = None if cap is None else (cap, max(1, int(c["num_simulations"]) // 4))
    want = PC.play_game(c, peaked, seed, tree_reuse=reuse, cap=cap)
    mine = SM.play_game(c, peaked, seed, tree_reuse=reuse, cap=cap, solver=False)
    _same(mine[0], want[0])
    assert mine[1:3] == want[1:3]
    for k in ("sims", "reused_visits", "reroots", "fast_moves", "fast_sims", "full_moves"):
        assert mine[3][k] == want[3][k], k
    assert all(mine[3][k] == 0 for k in SM.COUNTERS) and not any(s["proven"] for s in mine[0])


def _proof_height(s, node):
    """The height of the decided subtree that proves `node`: 0 for a terminal leaf."""
    n = int(s.nch[node])
    if n == 0:
        return 0
    f = int(s.first[node])
    kids = [c for c in range(f, f + n) if s.state[c] != SM.UNKNOWN]
    if s.state[node] == SM.LOSS:                       # one WIN child proves it
        return 1 + min(_proof_height(s, c) for c in kids if s.state[c] == SM.WIN)
    return 1 + max(_proof_height(s, c) for c in kids)


def _check_against_minimax(s, game, checked):
    level = [(0, game)]
    for depth in range(4):
        nxt = []
        for node, g in level:
            if node != 0 or depth == 0:
                st = int(s.state[node])
                if st != SM.UNKNOWN and int(s.start["state"][node] if node < len(s.start["state"]) else 0) == SM.UNKNOWN:
                    h = _proof_height(s, node)
                    if h <= 3:
                        assert SM.minimax(g, h) == st, (node, depth, h)
                        checked.append((depth, h))
            if depth == 3:
                continue
            f, n = int(s.first[node]), int(s.nch[node])
            for c in range(f, f + n):
                if s.nch[c] > 0 or s.state[c] != SM.UNKNOWN:
                    g2 = g.clone()
                    g2.make_action(int(s.action[c]))
                    nxt.append((c, g2))
        level = nxt


@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
@pytest.mark.parametrize("game", GAMES, ids=IDS)
def test_states_are_consistent_and_agree_with_minimax(game, reuse):
    c, peaked, seed, name = game
    checked, searches = [], []

    def on_move(s, chosen, kept, g):
        s.check_consistency()
        _check_against_minimax(s, g, checked)
        searches.append(s)
        v, _ = s.final_counts()
        f, n = int(s.first[0]), int(s.nch[0])
        st = s.state[f:f + n]
        assert 0 < int(v.sum()) <= s.budget
        if (st != SM.LOSS).any():                       # no played move is shown to lose while a sibling is not
            assert s.state[chosen] != SM.LOSS or not v[st != SM.LOSS].any()
        if s.early is not None:
            assert s.state[chosen] == SM.WIN

    _, _, _, st = SM.play_game(no_resign(c), peaked, seed, tree_reuse=reuse, on_move=on_move)
    print(name, "reuse", reuse, {k: st[k] for k in SM.COUNTERS}, "minimax checks (depth, height)", sorted(set(checked)))
    assert (st["proven_nodes"] > 0) == (name != "maxlen")
    if st["proven_nodes"]:
        assert checked


# (decided nodes, stops, early ends) of the five games on fresh trees without the cap, resignation off: pinned
FRESH = {"resign": (30, 0, 1), "maxlen": (0, 0, 0), "natural": (24, 6, 0), "resign_late": (21, 4, 1), "long_peaked": (4, 0, 1)}


def test_the_compared_games_prove_something():
    total = dict.fromkeys(SM.COUNTERS, 0)
    for c, peaked, seed, name in GAMES:
        smp, winner, plies, st = SM.play_game(no_resign(c), peaked, seed)
        assert (st["proven_nodes"], st["proven_stops"], st["proven_moves"]) == FRESH[name], name
        assert sum(s["proven"] for s in smp) == st["proven_moves"]
        for k in total:
            total[k] += st[k]
        if name == "maxlen":                           # nothing decided: the solver-off game, record for record
            off = SM.play_game(no_resign(c), peaked, seed, solver=False)
            _same(smp, off[0])
            assert (winner, plies) == off[1:3] and all(st[k] == 0 for k in SM.COUNTERS)
    assert total["proven_nodes"] > 0 and total["proven_stops"] > 0 and total["proven_moves"] > 0
    assert total["unspent_sims"] > 0 and total["removed_visits"] > 0


def test_two_rooks_against_a_bare_king_are_decided():
    # red K (1,5), R (1,7), R (3,6) against black K (7,3), red to move, uniform stub, flat noise
    g = SM.crafted_game([(1, 5, 1), (1, 7, 5), (3, 6, 5), (7, 3, -1)])
    s = SM.search_position(g, 256, noise=np.full(len(g.legal_actions()), 1.0 / len(g.legal_actions())))
    s.check_consistency()
    assert s.state[0] != SM.UNKNOWN and s.proven_nodes > 0
    child, root = s.root_states()
    assert root == 1 and (child == 1).any()             # the side to move wins
