"""The settled-move cutoff's rule on the host (tests/settle_model.py): exact -- a settled search keeps its first maximum however the
remaining simulations are spent -- and strict -- at lead == remaining the first maximum can still move."""
import os

import numpy as np
import pytest

import settle_model as SM

NCH = (1, 2, 63, 64, 65, 128)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def the_header_states_the_rule_the_model_implements():
    """The model stands for xq_engine_settle: without that entry and its rule in include/xq_hip.h it pins nothing."""
    text = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "int xq_engine_settle(" in text and "n1 - n2 > budget - sims_done" in text and "nch == 1" in text


def _vectors(nch, rng, n=300):
    """(visits, sims_done, budget) with every shape of lead: peaked, flat, tied, fresh and nearly finished searches."""
    for _ in range(n):
        budget = int(rng.integers(1, 400))
        done = int(rng.integers(0, budget + 1))
        kind = int(rng.integers(0, 4))
        if kind == 0:                                   # what a search gives: done visits spread by a peaked distribution
            p = rng.dirichlet(np.full(nch, 0.05))
            v = rng.multinomial(done, p)
        elif kind == 1:                                 # flat
            v = rng.multinomial(done, np.full(nch, 1.0 / nch))
        elif kind == 2:                                 # a tie for first, somewhere
            v = rng.integers(0, 5, size=nch)
            v[rng.integers(0, nch, size=min(2, nch))] = 7
        else:                                           # the lead within one of the remaining simulations, either side
            v = rng.integers(0, 3, size=nch)
            v[int(rng.integers(0, nch))] = max(0, int(v.max()) + (budget - done) + int(rng.integers(-1, 2)))
        yield np.asarray(v, dtype=np.int64), done, budget


@pytest.mark.parametrize("nch", NCH)
def test_a_settled_search_keeps_its_first_maximum(nch):
    rng = np.random.default_rng(100 + nch)
    seen = {True: 0, False: 0}
    for v, done, budget in _vectors(nch, rng):
        s = SM.settled(v, done, budget)
        seen[s] += 1
        if not s:
            continue
        assert done < budget
        best, rem = SM.first_max(v), budget - done
        order = np.argsort(-v, kind="stable")
        rivals = [int(order[1])] if nch > 1 else []                          # the runner-up (lowest index among equals)
        rivals += [0, nch - 1, int(rng.integers(0, nch))]                    # the lowest index, the highest, any
        for c in rivals:
            assert SM.first_max(SM.after(v, c, rem)) == best, (v, done, budget, c)
        for _ in range(4):                                                   # and spread at random, over every prefix
            w = v.copy()
            for c in rng.integers(0, nch, size=rem):
                w[c] += 1
                assert SM.first_max(w) == best
    assert seen[True] > 20 and (nch == 1 or seen[False] > 20)                # both verdicts occurred


def test_the_inequality_is_strict():
    """lead == remaining, the runner-up at the lower index: not settled, and the runner-up does take the first maximum."""
    v, done, budget = np.array([3, 9, 0]), 12, 18
    assert SM.lead(v) == budget - done == 6
    assert not SM.settled(v, done, budget)
    assert SM.first_max(v) == 1 and SM.first_max(SM.after(v, 0, budget - done)) == 0
    assert SM.settled(v, done + 1, budget)                                   # one simulation fewer to go: settled
    assert SM.first_max(SM.after(v, 0, budget - done - 1)) == 1
    # the runner-up behind the leader: a tie would not move the first maximum, yet the rule does not look at indices
    assert not SM.settled(np.array([9, 3, 0]), 12, 18)


@pytest.mark.parametrize("nch", NCH)
def test_a_tie_for_first_is_never_settled_unless_the_move_is_forced(nch):
    rng = np.random.default_rng(7 + nch)
    for _ in range(100):
        budget = int(rng.integers(2, 300))
        done = int(rng.integers(0, budget))
        v = rng.integers(0, 6, size=nch)
        if nch > 1:
            a, b = rng.choice(nch, size=2, replace=False)
            v[a] = v[b] = 50
            assert SM.lead(v) == 0
        assert SM.settled(v, done, budget) == (nch == 1)


def test_a_forced_move_is_settled_before_its_first_simulation_and_a_finished_search_is_not():
    assert SM.settled([0], 0, 32) and SM.settled([5], 5, 32)
    assert not SM.settled([32], 32, 32) and not SM.settled([30, 2], 32, 32)
    assert not SM.settled([], 0, 32)
    assert SM.totals([(0, [0], 0), (3, [20, 1], 21), (5, [4, 4], 8)], 32) == ([0, 3], 2, 32 + 11)
