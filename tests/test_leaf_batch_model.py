"""The leaf-batching host model (tests/leaf_batch_model.py) at K = 1 is the reference's sequential search: it reproduces the
recorded reference traces (tests/golden/mcts_traces.json) and the CPU oracle's search bit for bit.  This pins the model
before tests/test_leaf_batch_gpu.py uses it to judge the engine at K > 1."""
import numpy as np
import pytest

import golden_io as G
import leaf_batch_model as M
from oracle import xq_oracle as O
from stub_eval import StubEvaluator


def _replay(actions):
    g = O.Game()
    for a in actions:
        g.make_action(a)
    return g


@pytest.mark.parametrize("sims", [16, 100])
def test_model_k1_reproduces_reference_traces(sims):
    traces = [t for t in G.mcts_traces() if t["sims"] == sims]
    assert traces
    for t in traces:
        noise = None if t["eta"] is None else np.array([G.hexf(x) for x in t["eta"]])
        r = M.search(_replay(t["actions"]), sims, 1, M.stub_priors(t["stub"] == "peaked"), noise=noise)
        tag = (t["name"], t["stub"], t["noisy"])
        assert list(r["actions"]) == t["root_actions"], tag
        assert list(r["visits"]) == t["visits"], tag
        assert [float(x).hex() for x in r["total_value"]] == t["total_value"], tag
        assert [float(x).hex() for x in r["prior"]] == t["prior"], tag
        assert r["root_visits"] == t["root_visits"] and r["collisions"] == 0, tag


@pytest.mark.parametrize("peaked", [False, True])
def test_model_k1_equals_oracle_on_corpus_positions(peaked):
    d = G.corpus()
    picks = [i for i in range(5, len(d["board"]), 70) if not d["done"][i]][:8]
    for i in picks:
        first = i - d["ply"][i]
        g = _replay([int(a) for a in d["taken"][first:i]])
        want = O.mcts_search(g, 100, StubEvaluator(peaked=peaked).predict)
        got = M.search(g, 100, 1, M.stub_priors(peaked))
        n = want.n_children
        assert list(got["actions"]) == list(want.actions[:n])
        assert list(got["visits"]) == list(want.visits[:n]), i
        assert [float(x).hex() for x in got["total_value"]] == [float(x).hex() for x in want.total_value[:n]], i
        assert [float(x).hex() for x in got["prior"]] == [float(x).hex() for x in want.prior[:n]], i


def test_model_k_gt_1_invariants():
    """K > 1: every simulation is accounted for (root visits == S, children's visits sum to S), the virtual loss is gone
    after every step (asserted inside the model), and batching takes fewer steps than K = 1."""
    g = _replay([])
    for K in (2, 4, 8):
        s = M.LeafBatchSearch(g, 100, K, M.stub_priors(True)).run()
        r = s.root()
        assert r["root_visits"] == 100 and int(r["visits"].sum()) == 100
        assert max(s.leaves_per_step) <= K and s.steps < 100
