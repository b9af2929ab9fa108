"""The perpetual-check rule's host model (tests/perpetual_check_model.py) without a GPU: with the rule off it is the oracle's
is_game_over, with it on the fixtures of the rule get the verdicts its text gives them, and the search model backs the verdict up
with the sign of a mate."""
import numpy as np
import pytest

import golden_io as G
import leaf_batch_model as LB
import perpetual_check_model as M
from oracle import xq_oracle as O


def test_rule_off_is_the_oracle_over_the_corpus():
    d = G.corpus()
    picks = sorted(set(np.nonzero(d["done"])[0].tolist()) | set(range(0, len(d["board"]), 9)))
    for i in picks:
        kind, winner = M.verdict(d["board"][i], d["side"][i], d["move_count"][i], d["no_capture"][i], G.history_tail(d, i))
        assert (kind != M.NOT_OVER) == bool(d["done"][i]) and winner == d["winner"][i], i
    assert {M.verdict(d["board"][i], d["side"][i], d["move_count"][i], d["no_capture"][i], G.history_tail(d, i))[0]
            for i in np.nonzero(d["done"])[0]} >= {M.NO_MOVE, M.PLY200, M.REPETITION}


@pytest.mark.parametrize("make,winner_on", [(M.pc_red, -1), (M.pc_black, 1), (M.pc_red_rotated, None)],
                         ids=["pc_red", "pc_black", "pc_red_rotated"])
def test_replayed_perpetual_check(make, winner_on):
    for plies in range(12):
        g = make(plies)
        assert g.is_game_over() == (False, None), plies
        assert M.is_game_over(g, False) == (False, None) and M.is_game_over(g, True) == (False, None), plies
    g = make(12)
    assert g.move_count == 12 and g.is_game_over() == (True, 0)
    assert M.game_verdict(g, False) == (M.REPETITION, 0)
    if winner_on is None:                              # the checker's move completed the span: the side to move wins
        winner_on = g.current_player
        assert O.is_in_check(g.board, g.current_player)
    assert M.game_verdict(g, True) == (M.PERPETUAL, winner_on)


def test_pc_red_checks_are_where_the_issue_says():
    for plies in range(13):
        g = M.pc_red(plies)
        assert O.is_in_check(g.board, -1) == (plies % 2 == 1) and not O.is_in_check(g.board, 1), plies


def test_quiet_shuffle_is_a_draw_under_both_rules():
    for plies in range(12):
        assert M.is_game_over(M.quiet(plies), True) == (False, None)
    g = M.quiet(12)
    assert g.is_game_over() == (True, 0)
    assert M.game_verdict(g, False) == (M.REPETITION, 0) and M.game_verdict(g, True) == (M.REPETITION, 0)


@pytest.mark.parametrize("case", M.synthetic_cases(), ids=[c[0] for c in M.synthetic_cases()])
def test_synthetic_histories(case):
    _, state, off, on = case
    assert M.verdict(*state, perpetual=False) == off
    assert M.verdict(*state, perpetual=True) == on


def test_short_span_counts_only_entries_up_to_E():
    cases = {c[0]: c for c in M.synthetic_cases()}
    board, side, mc, nc, hist = cases["short_span"][1]
    entries = [hist[11 - e] for e in range(12)]
    assert [e for e in range(12) if np.array_equal(entries[e], board)] == [1, 3, 7]
    assert not O.is_in_check(entries[10], -side)       # the quiet board lies beyond E = 7
    assert M.perpetual_winner(board, side, entries) == -1


def _root(game, sims, K, perpetual):
    return M.search(game, sims, K, M.uniform_priors, perpetual)


@pytest.mark.parametrize("K", [1, 4])
def test_search_model_off_is_the_leaf_batch_model(K):
    for g in (M.pc_red(11), M.quiet(11), M.cycle_game(M.MATE_IN_ONE, [], 0)):
        a, b = _root(g, 64, K, False), LB.search(g, 64, K, M.uniform_priors)
        assert list(a["actions"]) == list(b["actions"]) and list(a["visits"]) == list(b["visits"])
        assert [float(x).hex() for x in a["total_value"]] == [float(x).hex() for x in b["total_value"]]


@pytest.mark.parametrize("K", [1, 4])
def test_search_model_backs_the_verdict_up_like_a_mate(K):
    g = M.pc_red(11)
    rep = M.PC_RED_CYCLE[3]
    assert sorted(g.legal_actions().tolist()) == sorted([rep, 76 * 90 + 67])     # K -> (9,4) repeats, K -> (7,4)
    off, on = _root(g, 64, K, False), _root(g, 64, K, True)
    i = list(on["actions"]).index(rep)
    assert off["total_value"][i] == 0.0 and off["visits"][i] > 0
    assert on["total_value"][i] == on["visits"][i] > off["visits"][i]
    mate = _root(M.cycle_game(M.MATE_IN_ONE, [], 0), 64, K, True)
    j = list(mate["actions"]).index(M.MATE_MOVE)
    assert mate["total_value"][j] == mate["visits"][j] > 0         # the same sign: the mover wins
    # the checker's own move completes its perpetual: that child is the mover's loss
    g = M.pc_red_rotated(11)
    rot = _root(g, 64, K, True)
    k = list(rot["actions"]).index(M.PC_RED_CYCLE[0])
    assert rot["visits"][k] > 0 and rot["total_value"][k] == -rot["visits"][k]
