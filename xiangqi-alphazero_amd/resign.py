"""Calibration of the per-side resign rule from its holdout (xq_engine_resign).  Host arrays only.

A holdout game is exempt from resignation and played out; its row (sample_format.RESIGN_ROW_DTYPE) holds, per side, the lowest
window that side ever had: `level[s]` is below a threshold t exactly when the side would have resigned under t at some ply.  So
the pairs (game, side) with a finite level answer "how often does a side that would have resigned under t not lose?":

    FP(t) = #{pairs with level < t whose side did not lose} / #{pairs with level < t}

where "did not lose" is winner != -side, draws included.  Both functions are deterministic and look at nothing but the rows.
"""
from __future__ import annotations

import numpy as np

from .sample_format import RESIGN_ROW_DTYPE

SIDES = (1, -1)                # level[0] is red's, level[1] black's


def holdout_pairs(rows: np.ndarray):
    """-> (level float32[m], not_lost bool[m]) over the pairs (game, side) with a finite level, sorted by level (stable: rows in
    the order given, red before black)."""
    rows = np.asarray(rows, dtype=RESIGN_ROW_DTYPE).reshape(-1)
    level = rows["level"].astype(np.float32).reshape(-1, 2)
    winner = rows["winner"].astype(np.int64)
    not_lost = np.stack([winner != -s for s in SIDES], axis=1)
    keep = np.isfinite(level)
    lv, nl = level[keep], not_lost[keep]
    order = np.argsort(lv, kind="stable")
    return lv[order], nl[order]


def false_positive_curve(rows: np.ndarray) -> dict:
    """The holdout's curve at every threshold that separates observed levels: `threshold` float64[k] ascending, the float32
    successor of each distinct level (the smallest threshold that level is below); `below` int64[k] the pairs with level <
    threshold; `false_positives` int64[k] those whose side did not lose; `rate` float64[k] their quotient.  `pairs` is the
    number of pairs with a finite level."""
    lv, nl = holdout_pairs(rows)
    distinct = np.unique(lv)
    below = np.searchsorted(lv, distinct, side="right").astype(np.int64)       # levels <= d, i.e. < successor(d)
    cum = np.concatenate([[0], np.cumsum(nl.astype(np.int64))])
    fp = cum[below]
    return dict(threshold=np.nextafter(distinct.astype(np.float32), np.float32(np.inf)).astype(np.float64), below=below,
                false_positives=fp, rate=fp / np.maximum(below, 1), pairs=int(len(lv)))


def rate_below(rows: np.ndarray, threshold: float):
    """-> (pairs with level < threshold, those whose side did not lose) at one threshold."""
    lv, nl = holdout_pairs(rows)
    m = lv.astype(np.float64) < float(threshold)
    return int(m.sum()), int(nl[m].sum())


def calibrate(rows: np.ndarray, target: float, min_pairs: int, t_max: float) -> float:
    """The largest threshold t <= t_max, among the successors of the observed levels, with at least `min_pairs` pairs below it
    and FP(t) <= target; -inf (nobody resigns) when there is none."""
    if not 0.0 <= float(target) <= 1.0:
        raise ValueError(f"calibrate: target must be in [0, 1], got {target!r}")
    if int(min_pairs) < 1:
        raise ValueError(f"calibrate: min_pairs must be at least 1, got {min_pairs!r}")
    c = false_positive_curve(rows)
    ok = (c["threshold"] <= float(t_max)) & (c["below"] >= int(min_pairs)) & (c["false_positives"] <= float(target) * c["below"])
    return float(c["threshold"][ok].max()) if ok.any() else float("-inf")
