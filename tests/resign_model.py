"""The per-side resign rule, its holdout draw, the false-positive curve and the calibration in plain Python and numpy
(include/xq_hip.h: xq_engine_resign; xiangqi-alphazero_amd/resign.py).  Nothing here imports the package."""
import math

import numpy as np

KIND_HOLDOUT = 12
MAX_STEPS = 8
INF = float("inf")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def window(values, n, K):
    """w_n = max(v_n, v_{n-2}, .., v_{n-2(K-1)}); None while n < 2(K-1); NaN when one of them is."""
    if n < 2 * (K - 1):
        return None
    w = [float(values[n - 2 * j]) for j in range(K)]
    return float("nan") if any(math.isnan(x) for x in w) else max(w)


def scan(values, first_side, K, threshold, plies=None):
    """The rule over one sequence of values (float32 widened), the side to move at index 0 being `first_side` (1 red, else black).
    -> dict: resign_index (the first n with w_n < threshold, or -1), resigner (that side, or 0), level [red, black] (float32, +inf
    for none) and level_index [red, black] (where first reached, -1 for none) over the WHOLE sequence.  With `plies` (the game ply
    of every index) also resign_ply and level_ply (0 for none)."""
    assert 1 <= K <= MAX_STEPS
    values = [float(np.float32(v)) for v in values]
    first = 1 if first_side == 1 else -1
    level, level_index = [INF, INF], [-1, -1]
    resign_index, resigner = -1, 0
    for n in range(len(values)):
        w = window(values, n, K)
        if w is None:
            continue
        side = first if n % 2 == 0 else -first
        s = 0 if side == 1 else 1
        if w < level[s]:
            level[s], level_index[s] = w, n
        if resign_index < 0 and w < threshold:
            resign_index, resigner = n, side
    out = dict(resign_index=resign_index, resigner=resigner, level=[np.float32(x) for x in level], level_index=level_index)
    if plies is not None:
        out["resign_ply"] = int(plies[resign_index]) if resign_index >= 0 else -1
        out["level_ply"] = [int(plies[i]) if i >= 0 else 0 for i in level_index]
    return out


def levels_until(values, first_side, K, stop):
    """scan's levels over the first `stop` values only."""
    return scan(values[:stop], first_side, K, -INF)


def reference_rule(values, K, threshold):
    """The reference's rule as the engine runs it (expand_root_finish): the first n where the last K CONSECUTIVE values -- the
    sides alternate -- are all below the threshold, or -1."""
    values = [float(np.float32(v)) for v in values]
    for n in range(len(values)):
        if n + 1 >= K and all(v < threshold for v in values[n + 1 - K:n + 1]):
            return n
    return -1


# ---- the holdout draw: Philox4x32-10 keyed by the seed, counter (slot, kind | sub << 8, ctr, rank) ---------------------------------
M32 = 0xFFFFFFFF


def philox_u64(seed, rank, slot, kind, ctr, sub):
    c = [slot & M32, (kind | (sub << 8)) & M32, ctr & M32, rank & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c[0] << 32) | c[1]


def exempt(seed, rank, slot, game_seq, prob):
    return (philox_u64(seed, rank, slot, KIND_HOLDOUT, game_seq, 0) >> 11) * 2.0 ** -53 < prob


# ---- the curve and the calibration --------------------------------------------------------------------------------------------------
def pairs(rows):
    """[(level, side did not lose)] over the pairs (game, side) with a finite level; rows: (level_red, level_black, winner)."""
    out = []
    for red, black, winner in rows:
        for level, side in ((red, 1), (black, -1)):
            if math.isfinite(level):
                out.append((float(np.float32(level)), winner != -side))
    return out


def fp(rows, t):
    """-> (pairs with level < t, those whose side did not lose)."""
    below = [nl for level, nl in pairs(rows) if level < t]
    return len(below), sum(below)


def successor(level):
    return float(np.nextafter(np.float32(level), np.float32(np.inf)))


def calibrate(rows, target, min_pairs, t_max):
    best = -INF
    for level, _ in pairs(rows):
        t = successor(level)
        n, bad = fp(rows, t)
        if t <= t_max and n >= min_pairs and bad <= target * n:
            best = max(best, t)
    return best
