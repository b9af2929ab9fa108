"""CPU checks of the arena-openings host model (tests/arena_openings_model.py) and of `arena.pair_statistics`: with no opening
the model IS the reference's arena (all three recorded sets, game by game), pair partners given the same draws get the same
opening, and the pair statistics on hand-made tables."""
import math

import numpy as np
import pytest

import arena_openings_model as AM
import golden_io as G
from stub_eval import StubEvaluator


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_model_without_opening_reproduces_the_reference_arena(name):
    t = [x for x in G.arena_traces() if x["name"] == name][0]
    new, old = StubEvaluator(peaked=t["new_peaked"]), StubEvaluator(peaked=not t["new_peaked"])
    played = {}                                        # without openings a game is a function of the colour assignment
    for g in t["games"]:
        red = g["game"] % 2 == 0
        if red not in played:
            played[red] = AM.play_game([], new.predict, old.predict, red, t["eval_simulations"], t["max_game_length"])
        assert played[red] == (g["winner"], g["steps"]), (name, g)


def test_partners_with_the_same_stream_get_the_same_opening():
    seen = set()
    for pair in range(12):
        raw = AM.choice_stream(100 + pair, 4)
        a, b = AM.opening_actions(raw, 4), AM.opening_actions(list(raw), 4)      # games 2p and 2p + 1: the same draws
        assert a == b and len(a) == 4
        seen.add(tuple(a))
    assert len(seen) >= 11                             # ~3.7 M four-ply openings: different streams, different openings
    assert AM.opening_actions(AM.choice_stream(7, 4), 0) == []


def test_opening_rule_is_x_mod_count_over_the_ordered_legal_moves():
    from oracle import xq_oracle as O
    g = O.Game()
    legal = [int(a) for a in g.legal_actions()]
    n = len(legal)
    assert AM.opening_actions([0], 1) == [legal[0]]
    assert AM.opening_actions([n + 3], 1) == [legal[3]]
    assert AM.opening_actions([2 ** 64 - 1], 1) == [legal[(2 ** 64 - 1) % n]]


def test_pair_statistics_all_pairs_split():
    from xiangqi_alphazero_amd import arena
    # red wins every game: the new model wins the even game and loses the odd one of every pair
    ps = arena.pair_statistics([1, 1] * 6)
    assert ps["pairs"] == 6 and ps["win_rate"] == 0.5 and ps["win_rate_se"] == 0.0 and ps["win_rate_ci95"] == (0.5, 0.5)
    ps = arena.pair_statistics([-1, -1, 1, 1, 0, 0])
    assert ps["win_rate"] == 0.5 and ps["win_rate_se"] == 0.0


def test_pair_statistics_known_mixed_table():
    from xiangqi_alphazero_amd import arena
    # pair 0: new (red) wins, new (black) wins -> 1.0; pair 1: draw, new (black) loses -> 0.25; pair 2: loses both -> 0.0;
    # pair 3: wins, draw -> 0.75.  mean 0.5; deviations 0.5, -0.25, -0.5, 0.25: sum of squares 0.625; variance (ddof 1) 0.625 / 3;
    # se = sqrt(0.625 / 3 / 4) = sqrt(0.625 / 12)
    ps = arena.pair_statistics([1, -1, 0, 1, -1, 1, 1, 0])
    se = math.sqrt(0.625 / 12.0)
    assert ps["pairs"] == 4 and ps["win_rate"] == 0.5
    assert abs(ps["win_rate_se"] - se) < 1e-15
    assert abs(ps["win_rate_ci95"][0] - (0.5 - 1.96 * se)) < 1e-15 and abs(ps["win_rate_ci95"][1] - (0.5 + 1.96 * se)) < 1e-15
    # the per-game win rate of evaluate_models is the same number
    assert ps["win_rate"] == (3 + 0.5 * 2) / 8
    for bad in ([], [1], [1, 0, -1]):
        with pytest.raises(ValueError):
            arena.pair_statistics(bad)
    assert arena.pair_statistics(np.array([1, -1]))["win_rate_se"] == 0.0     # one pair: no spread to estimate
