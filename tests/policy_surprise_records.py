"""Hand-made sample records and logits for the policy-surprise tests (CPU model, ABI and GPU files share them)."""
import numpy as np

from xiangqi_alphazero_amd import sample_format as F

N_MOVES = (0, 1, 2, 63, 64, 65, 128)


def set_policy_stats(smp: np.ndarray, kl, marked, top1=0) -> None:
    """Write xq_sample_policy_stats into bytes 120..127 of every record, in place."""
    ps = np.zeros(len(smp), dtype=F.POLICY_STATS_DTYPE)
    ps["policy_kl"], ps["has_policy_stats"], ps["prior_top1"] = kl, marked, top1
    smp.view(np.uint8).reshape(len(smp), 640)[:, 120:128] = ps.view(np.uint8).reshape(len(smp), 8)


def random_identity(smp: np.ndarray, rng) -> None:
    n = len(smp)
    smp["slot"] = rng.integers(0, 8192, n)
    smp["game_seq"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    smp["ply"] = rng.integers(0, 400, n)


def surprise_records(n: int, seed: int, marked_share: float = 0.6, zero_kl: bool = False) -> np.ndarray:
    """n records with random identities; about `marked_share` of them marked, with exponential KLs (a few past the 64-nat cap, a few
    exactly 0)."""
    rng = np.random.default_rng(seed)
    smp = np.zeros(n, dtype=F.SAMPLE_DTYPE)
    random_identity(smp, rng)
    kl = rng.exponential(0.7, n).astype(np.float32)
    kl[rng.random(n) < 0.05] = 0.0
    kl[rng.random(n) < 0.02] = 100.0
    if zero_kl:
        kl[:] = 0.0
    set_policy_stats(smp, kl, (rng.random(n) < marked_share).astype(np.uint8), rng.integers(0, 2, n))
    return smp


def score_records(n: int, seed: int):
    """-> (records, logits float32[n,128], value float32[n], notes): n records cycling through N_MOVES and through the kinds the
    score kernel must handle; row k's kind is notes[k].  Every record carries root statistics (so byte 116 and the root fields are
    there to be left alone) and a random board."""
    rng = np.random.default_rng(seed)
    smp = np.zeros(n, dtype=F.SAMPLE_DTYPE)
    random_identity(smp, rng)
    logits = np.full((n, 128), np.nan, dtype=np.float32)            # behind m: never read, so poison it
    value = rng.uniform(-1, 1, n).astype(np.float32)
    kinds = ("plain", "zero_visits", "late_temp", "gumbel", "spread80", "nonfinite_inside", "nonfinite_behind", "no_visits", "ties")
    notes = []
    rs = np.zeros(n, dtype=F.ROOT_STATS_DTYPE)
    rs["root_q"], rs["root_visits"], rs["has_root_stats"] = rng.uniform(-1, 1, n), rng.integers(1, 800, n), 1
    smp["pad"] = rs.view(np.uint8).reshape(n, 20)
    for k in range(n):
        m = N_MOVES[k % len(N_MOVES)]
        kind = kinds[(k // len(N_MOVES) + k) % len(kinds)]
        s = smp[k]
        s["board"] = rng.integers(-7, 8, 90)
        s["side"], s["z"], s["n_moves"] = rng.choice([-1, 1]), rng.integers(-1, 2), m
        s["actions"][:m] = rng.choice(8100, m, replace=False)
        vis = rng.integers(1, 200, m)
        lg = rng.normal(0, 2, m)
        if kind == "zero_visits" and m > 1:
            vis[rng.random(m) < 0.5] = 0
            vis[rng.integers(0, m)] = 5
        elif kind == "late_temp":
            s["late_temp"] = 1
            if m > 2:
                vis[1] = 0
        elif kind == "gumbel":
            s["reserved0"] = 1
            p = rng.dirichlet(np.full(m, 0.3)) if m else np.zeros(0)
            vis = np.floor(p * 65535).astype(np.int64)
            if m:
                vis[int(np.argmax(p))] = max(1, vis[int(np.argmax(p))])
        elif kind == "spread80":
            lg = rng.uniform(-80, 80, m)
        elif kind == "no_visits":
            vis[:] = 0
        elif kind == "ties" and m > 2:
            vis[:] = 7
            lg[:] = 0.25
            lg[m // 2] = lg[m - 1] = 3.0                             # the first largest logit is m // 2, the first largest visit 0
        s["visits"][:m] = vis
        logits[k, :m] = lg.astype(np.float32)
        if kind == "nonfinite_inside" and m > 0:
            logits[k, rng.integers(0, m)] = (np.inf, -np.inf, np.nan)[k % 3]
        if kind == "nonfinite_behind" and m < 128:
            logits[k, m] = np.inf
        notes.append(kind)
    return smp, logits, value, notes
