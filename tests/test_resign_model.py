"""The per-side resign rule on hand-made sequences (tests/resign_model.py), the package's curve and calibration against the
model's and against answers worked out by hand, and the host draw against the library's (xq_resign_exempt_host).  No GPU."""
import math

import numpy as np
import pytest

import resign_model as RM

LOW, HIGH, T = float(np.float32(-0.95)), 0.5, -0.9      # the values are float32


def _scan(values, K, first=1, t=T):
    r = RM.scan(values, first, K, t)
    return r["resign_index"], r["resigner"], [float(x) for x in r["level"]], r["level_index"]


def test_k1_is_the_plain_comparison():
    assert _scan([HIGH, HIGH, LOW, HIGH], 1) == (2, 1, [LOW, HIGH], [2, 1])
    assert _scan([HIGH, LOW], 1) == (1, -1, [HIGH, LOW], [0, 1])
    assert _scan([HIGH, LOW], 1, first=-1) == (1, 1, [LOW, HIGH], [1, 0])


def test_k2_takes_two_values_of_the_same_side():
    # red: -0.95 at 0 and at 2 -> the window at 2 is low; black is never low
    assert _scan([LOW, HIGH, LOW], 2) == (2, 1, [LOW, math.inf], [2, -1])
    assert _scan([LOW, HIGH, -0.99, HIGH], 2)[:2] == (2, 1)
    assert _scan([LOW, HIGH, -0.99, HIGH], 2)[2] == [LOW, HIGH]            # the window is the larger of the two


def test_k8_needs_fifteen_values():
    seq = [LOW if n % 2 == 0 else HIGH for n in range(15)]
    assert _scan(seq, 8) == (14, 1, [LOW, math.inf], [14, -1])
    assert _scan(seq[:14], 8) == (-1, 0, [math.inf, math.inf], [-1, -1])     # shorter than 2K - 1: no window at all
    assert RM.window(seq, 13, 8) is None and RM.window(seq, 14, 8) == LOW


def test_a_sequence_shorter_than_the_window_never_resigns():
    for K in range(2, 9):
        seq = [LOW] * (2 * K - 2)
        assert _scan(seq, K) == (-1, 0, [math.inf, math.inf], [-1, -1]), K
        assert _scan(seq + [LOW], K)[0] == 2 * K - 2


def test_a_low_run_broken_by_one_value_of_the_same_side_starts_again():
    # red's values: low, low, HIGH, low, low, low with K = 3 -> the first window without the high value is at red's sixth
    seq = []
    for v in (LOW, LOW, HIGH, LOW, LOW, LOW):
        seq += [v, 0.0]
    idx, who, level, where = _scan(seq, 3)
    assert (idx, who) == (10, 1)
    assert level[0] == LOW and where[0] == 10
    # a high value of the OTHER side breaks nothing
    assert _scan([LOW, 0.9, LOW, 0.9, LOW], 3)[:2] == (4, 1)


def test_both_sides_low_on_alternate_plies_fires_per_side_but_not_the_reference():
    # red is low on plies 0, 4, 8, .., black on 2... no: each side is low on every second one of its own plies
    seq = [LOW, LOW, HIGH, HIGH] * 5
    assert RM.reference_rule(seq, 5, T) == -1 and RM.reference_rule(seq, 3, T) == -1
    assert _scan(seq, 2)[0] == -1                                            # nor per side: no side has two low values in a row
    # both sides low on all their plies: both rules fire, the per-side rule as soon as the side to move has K values
    seq = [LOW] * 12
    assert RM.reference_rule(seq, 5, T) == 4
    assert _scan(seq, 5)[:2] == (8, 1)
    assert _scan(seq, 2)[:2] == (2, 1)
    # low values of the two sides interleaved with one high value each: per side K = 2 finds red's pair, the reference's
    # five consecutive values never come
    seq = [LOW, HIGH, LOW, LOW, HIGH, LOW, LOW, HIGH]
    assert RM.reference_rule(seq, 5, T) == -1
    assert _scan(seq, 2)[:2] == (2, 1)


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_one_side_low_for_ever_never_fires_the_reference_rule(K):
    """The point of the option: red judges itself lost at every one of its plies, black judges itself winning.  Consecutive
    values alternate the side, so for K >= 2 the reference's rule never sees K low values in a row; the per-side rule resigns red
    at its K-th value."""
    seq = [LOW if n % 2 == 0 else -LOW for n in range(60)]
    assert RM.reference_rule(seq, K, T) == -1
    assert _scan(seq, K) == (2 * (K - 1), 1, [LOW, -LOW], [2 * (K - 1), 2 * (K - 1) + 1])
    assert RM.reference_rule(seq, 1, T) == 0 and _scan(seq, 1)[:2] == (0, 1)     # K = 1: the two rules are one


def test_equality_at_the_threshold_does_not_resign():
    t = float(np.float32(-0.9))
    assert _scan([t, 0.0, t], 2, t=t)[0] == -1
    below = float(np.nextafter(np.float32(t), np.float32(-np.inf)))
    assert _scan([below, 0.0, below], 2, t=t)[:2] == (2, 1)
    assert _scan([below, 0.0, t], 2, t=t)[0] == -1                           # the window is the larger value
    # the values are float32, the threshold a double: float32(-0.9) lies above the double -0.9 and does not resign under it
    assert _scan([-0.9, 0.0, -0.9], 2, t=-0.9)[0] == -1 and float(np.float32(-0.9)) > -0.9
    assert _scan([below, 0.0, below], 2, t=-0.9)[:2] == (2, 1)


def test_a_nan_never_resigns_and_lowers_no_level():
    nan = float("nan")
    assert _scan([LOW, 0.0, nan], 2) == (-1, 0, [math.inf, math.inf], [-1, -1])
    assert _scan([nan, 0.0, LOW, 0.0, LOW], 2) == (4, 1, [LOW, 0.0], [4, 3])      # the window at 2 holds the NaN, the one at 4 does not
    assert _scan([nan], 1) == (-1, 0, [math.inf, math.inf], [-1, -1])
    assert _scan([LOW, LOW], 1, t=-math.inf)[0] == -1 and _scan([LOW], 1, t=math.inf)[0] == 0


def test_the_levels_go_on_after_the_resignation_index():
    seq = [LOW, 0.0, LOW, 0.0, -0.99, 0.0, -0.99]
    idx, who, level, where = _scan(seq, 2)
    assert (idx, who) == (2, 1) and level[0] == float(np.float32(-0.99)) and where[0] == 6
    r = RM.scan(seq, 1, 2, T, plies=[20 + n for n in range(len(seq))])
    assert r["resign_ply"] == 22 and r["level_ply"] == [26, 23]


# ---- the curve and the calibration ------------------------------------------------------------------------------------------------
def _rows(triples):
    from xiangqi_alphazero_amd.sample_format import RESIGN_ROW_DTYPE
    rows = np.zeros(len(triples), dtype=RESIGN_ROW_DTYPE)
    for i, (red, black, winner) in enumerate(triples):
        rows[i]["slot"], rows[i]["game_seq"] = i, 1
        rows[i]["level"] = (red, black)
        rows[i]["winner"] = winner
    return rows


# red's level, black's level, winner.  Pairs by level: -0.98 red lost; -0.97 black lost; -0.95 red DREW (a false positive);
# -0.9 black lost; -0.8 red WON (a false positive); -0.5 black lost; red of game 3 has no level
HAND = [(-0.98, 0.3, -1), (0.2, -0.97, 1), (-0.95, 0.1, 0), (math.inf, -0.9, 1), (-0.8, -0.5, 1)]


def test_the_curve_on_rows_counted_by_hand():
    from xiangqi_alphazero_amd import resign
    rows = _rows(HAND)
    assert RM.fp(HAND, -0.96) == (2, 0) and RM.fp(HAND, -0.9) == (3, 1) and RM.fp(HAND, -0.7) == (5, 2)
    for t in (-1.0, -0.96, -0.9, RM.successor(-0.9), -0.7, 0.0, 1.0):
        assert resign.rate_below(rows, t) == RM.fp(HAND, t), t
    c = resign.false_positive_curve(rows)
    assert c["pairs"] == 9 and len(c["threshold"]) == 9
    assert c["below"].tolist() == list(range(1, 10))
    assert c["false_positives"].tolist()[:5] == [0, 0, 1, 1, 2]
    for t, n, bad, rate in zip(c["threshold"], c["below"], c["false_positives"], c["rate"]):
        assert RM.fp(HAND, t) == (n, bad) and rate == bad / n
    assert resign.false_positive_curve(_rows([]))["pairs"] == 0


def test_calibrate_on_rows_counted_by_hand():
    from xiangqi_alphazero_amd import resign
    rows = _rows(HAND)
    s = RM.successor
    # no false positive allowed: the largest threshold keeps the two clean pairs below it
    assert resign.calibrate(rows, 0.0, 1, 0.0) == s(-0.97)
    # a quarter allowed: -0.95 alone is 1 of 3 (too many), with -0.9 it is 1 of 4 -- thresholds need not be contiguous
    assert resign.calibrate(rows, 0.25, 1, 0.0) == s(-0.9)
    assert resign.calibrate(rows, 0.34, 1, 0.0) == s(-0.5)                  # 2 of 6 at -0.5, 2 of 5 at -0.8 is too many
    assert resign.calibrate(rows, 0.25, 1, -0.93) == s(-0.97)                # t_max cuts the candidates
    assert resign.calibrate(rows, 1.0, 1, 10.0) == s(0.3)
    # min_pairs not met: nobody resigns
    assert resign.calibrate(rows, 0.0, 3, 0.0) == -math.inf
    assert resign.calibrate(rows, 0.25, 4, 0.0) == s(-0.9) and resign.calibrate(rows, 0.25, 5, -0.85) == -math.inf
    assert resign.calibrate(_rows([]), 0.5, 1, 0.0) == -math.inf
    # all pairs false positives
    wrong = [(-0.99, -0.98, 0), (-0.97, math.inf, 1)]
    assert resign.calibrate(_rows(wrong), 0.5, 1, 0.0) == -math.inf and resign.calibrate(_rows(wrong), 1.0, 1, 0.0) == s(-0.97)
    for target, min_pairs, t_max in ((0.0, 1, 0.0), (0.25, 1, 0.0), (0.34, 2, -0.6), (0.5, 3, 1.0), (0.1, 9, 1.0)):
        assert resign.calibrate(rows, target, min_pairs, t_max) == RM.calibrate(HAND, target, min_pairs, t_max)
    with pytest.raises(ValueError):
        resign.calibrate(rows, 1.5, 1, 0.0)
    with pytest.raises(ValueError):
        resign.calibrate(rows, 0.5, 0, 0.0)


def test_calibrate_equals_the_model_on_random_rows():
    from xiangqi_alphazero_amd import resign
    rng = np.random.default_rng(4)
    for n in (1, 7, 60):
        triples = []
        for _ in range(n):
            red, black = (float(np.float32(x)) for x in np.round(rng.uniform(-1, 0.2, 2), 2))
            triples.append((red if rng.random() < 0.8 else math.inf, black, int(rng.integers(-1, 2))))
        rows = _rows(triples)
        for target, min_pairs, t_max in ((0.05, 2, -0.5), (0.3, 5, 0.0), (0.0, 1, 1.0)):
            assert resign.calibrate(rows, target, min_pairs, t_max) == RM.calibrate(triples, target, min_pairs, t_max)


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", [0.0, 0.1, 1.0])
def test_the_host_draw_equals_the_library(prob):
    from xiangqi_alphazero_amd import hip
    hip.build()
    seed, rank = 0x1234567890ABCDEF, 3
    n = 4096
    got = [hip.resign_exempt(seed, rank, slot, game_seq, prob) for slot in range(64) for game_seq in range(1, 65)]
    want = [RM.exempt(seed, rank, slot, game_seq, prob) for slot in range(64) for game_seq in range(1, 65)]
    assert len(got) == n and got == want
    share = sum(got) / n
    if prob in (0.0, 1.0):
        assert share == prob
    else:
        assert abs(share - prob) <= 4 * math.sqrt(prob * (1 - prob) / n), share
    # another rank and another seed draw other games
    assert [hip.resign_exempt(seed, 0, s, 1, 0.5) for s in range(64)] != [hip.resign_exempt(seed, 1, s, 1, 0.5) for s in range(64)]
    assert [hip.resign_exempt(1, 0, s, 1, 0.5) for s in range(64)] != [hip.resign_exempt(2, 0, s, 1, 0.5) for s in range(64)]


def test_the_draw_is_its_own_stream():
    """Kind 12: the holdout draw is not the start pool's draw (kind 11) of the same game."""
    from xiangqi_alphazero_amd import hip
    hip.build()
    assert hip.RNG_KIND_RESIGN_HOLDOUT == RM.KIND_HOLDOUT == 12 != hip.RNG_KIND_START_POOL
    pool = [hip.start_pool_index(5, 0, s, 1, 1 << 20, 0.5) >= 0 for s in range(256)]
    hold = [hip.resign_exempt(5, 0, s, 1, 0.5) for s in range(256)]
    assert pool != hold
