"""The tree-reuse host model (tests/tree_reuse_model.py) on the CPU: with reuse off it is the oracle's self-play game on every
recorded game (tests/golden/game_traces.json); with reuse on every sample still holds S visits and each search starts from the
previous tree's subtree of the chosen child, node for node.  This pins the model before tests/test_tree_reuse_gpu.py uses it
to judge the engine."""
import numpy as np
import pytest

import golden_io as G
import tree_reuse_model as M
from draws import Draws
from oracle import xq_oracle as O
from stub_eval import StubEvaluator


@pytest.mark.parametrize("idx", range(4))
def test_model_without_reuse_is_the_oracle_game(idx):
    t = G.game_traces()[idx]
    peaked = t["stub"] == "peaked"
    d = Draws(t["seed"])
    want, w_winner, w_steps, _, _ = O.play_one_game(t["cfg"], StubEvaluator(peaked=peaked).predict, d.randint, d.choice_index,
                                                    d.dirichlet, d.uniform)
    got, winner, steps, stats = M.play_game(t["cfg"], peaked, t["seed"], tree_reuse=False)
    assert (winner, steps, len(got)) == (w_winner, w_steps, len(want)) == (t["winner"], t["steps"], len(t["plies"]))
    for a, b in zip(got, want):
        assert list(a["actions"]) == list(b["actions"]) and list(a["visits"]) == list(b["visits"])
        assert a["z"] == b["z"] and a["player"] == b["player"] and bytes(a["board"]) == bytes(b["board"])
    assert stats["reused_visits"] == 0 and stats["reroots"] == 0


def _same_subtree(old, x, new, y, is_root):
    """Node y of the new tree is node x of the old one, with the same children in the same order, recursively."""
    f, n = int(old["first"][x]), int(old["nch"][x])
    g, m = int(new["first"][y]), int(new["nch"][y])
    assert n == m and (f < 0) == (g < 0)
    assert old["W"][x].tobytes() == new["W"][y].tobytes() and old["action"][x] == new["action"][y]
    if not is_root:
        assert old["N"][x] == new["N"][y] and old["kind"][x] == new["kind"][y]
        assert old["P32"][x].tobytes() == new["P32"][y].tobytes()
    for i in range(n if f >= 0 else 0):
        _same_subtree(old, f + i, new, g + i, False)
    return 1 + sum(_count(old, f + i) for i in range(n if f >= 0 else 0))


def _count(t, x):
    f, n = int(t["first"][x]), int(t["nch"][x])
    return 1 + (sum(_count(t, f + i) for i in range(n)) if f >= 0 else 0)


@pytest.mark.parametrize("idx", range(4))
def test_model_with_reuse_keeps_the_chosen_subtree(idx):
    t = G.game_traces()[idx]
    S = int(t["cfg"]["num_simulations"])
    moves = []
    got, winner, steps, stats = M.play_game(t["cfg"], t["stub"] == "peaked", t["seed"], tree_reuse=True,
                                            on_move=lambda s, c, kept, g: moves.append((s, c, kept)))
    assert all(int(s["visits"].sum()) == S for s in got)
    checked = 0
    for (prev, c, kept), (nxt, _, _) in zip(moves, moves[1:]):
        old = {k: getattr(prev, k)[:prev.alloc] for k in M.ARRAYS}
        if old["first"][c] < 0:
            assert nxt.reused == 0
            continue
        new = nxt.start
        n_kept = _same_subtree(old, c, new, 0, True)
        assert len(new["N"]) == n_kept and list(kept["old_index"][:1]) == [c]
        f, n = int(new["first"][0]), int(new["nch"][0])
        assert f == 1 and new["kind"][0] == 1 and new["N"][0] == new["N"][f:f + n].sum() == nxt.reused == old["N"][c] - 1
        checked += 1
    assert checked > 0 and stats["reroots"] == checked
    assert stats["sims"] + stats["reused_visits"] == S * len(got)
