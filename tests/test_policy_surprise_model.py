"""The numpy float64 references of the scoring pass and of the policy-surprise epoch counts (sample_format.sample_scores,
surprise_weights, surprise_counts) on hand-made records, and the host twin xq_surprise_count_host against them.  No GPU."""
import numpy as np
import pytest

from policy_surprise_records import score_records, surprise_records
from xiangqi_alphazero_amd import sample_format as F


def _one(m, visits, late=0):
    s = np.zeros(1, dtype=F.SAMPLE_DTYPE)
    s["n_moves"], s["late_temp"] = m, late
    s["actions"][0, :m] = np.arange(m) + 100
    s["visits"][0, :m] = visits
    return s


def test_kl_is_exactly_zero_for_one_move():
    for lg in (0.0, -37.5, 80.0):
        for late in (0, 1):
            r = F.sample_scores(_one(1, [9], late), np.full((1, 128), lg, np.float32), np.array([0.25], np.float32))[0]
            assert r["valid"] == 1 and r["policy_kl"] == 0.0 and r["policy_ce"] == 0.0 and r["entropy"] == 0.0 and r["top1"] == 1
            assert r["value"] == np.float32(0.25)


def test_kl_vanishes_when_the_logits_are_log_t():
    rng = np.random.default_rng(5)
    for m in (2, 7, 64, 128):
        vis = rng.integers(1, 500, m)
        t = vis / vis.sum()
        lg = np.zeros((1, 128))
        lg[0, :m] = np.log(t) + 3.0                                   # any shift: log_softmax removes it
        r = F.sample_scores(_one(m, vis), lg, np.zeros(1, np.float32))[0]   # float64 logits: the reference keeps them
        assert 0.0 <= r["policy_kl"] <= 1e-12 and abs(r["policy_ce"] - r["entropy"]) <= 1e-12


def test_scores_on_hand_made_records():
    smp, logits, value, notes = score_records(130, 11)
    ref = F.sample_scores(smp, logits, value, 0.3)
    assert set(notes) >= {"plain", "zero_visits", "late_temp", "gumbel", "spread80", "nonfinite_inside", "nonfinite_behind",
                          "no_visits", "ties"}
    seen_valid = set()
    for k, (s, r) in enumerate(zip(smp, ref)):
        m = int(s["n_moves"])
        want_invalid = m == 0 or notes[k] == "no_visits" or (notes[k] == "nonfinite_inside")
        assert r["valid"] == (0 if want_invalid else 1), (k, notes[k], m)
        if want_invalid:
            assert r["policy_kl"] == 0 and r["policy_ce"] == 0 and r["value"] == 0 and r["top1"] == 0 and r["entropy"] == 0
            continue
        seen_valid.add(notes[k])
        assert r["policy_kl"] >= 0.0 and np.isfinite(r["policy_ce"]) and r["value"] == value[k]
        # ce - kl is the target's entropy, whatever the logits
        c = s["visits"][:m].astype(np.float64)
        w = np.where(c > 0, c ** (1 / 0.3), 0.0) if s["late_temp"] else c
        t = w[w > 0] / w.sum()
        h = float(-(t * np.log(t)).sum())
        assert abs((r["policy_ce"] - r["policy_kl"]) - h) <= 1e-12 * (r["policy_ce"] + h + 1.0), (k, notes[k])
        assert abs(r["entropy"] - h) <= 1e-12 * (h + 1.0)
        if notes[k] == "ties" and m > 2:
            assert r["top1"] == 0                                     # first largest logit m // 2, first largest visit 0
    assert seen_valid == set(notes) - {"no_visits", "nonfinite_inside"}
    # logits spread over +-80: the prior sits on one move, the reference stays finite and the KL is large
    k = [i for i, nme in enumerate(notes) if nme == "spread80" and smp[i]["n_moves"] >= 63][0]
    assert np.isfinite(ref[k]["policy_kl"]) and ref[k]["policy_kl"] > 1.0 and np.isfinite(ref[k]["policy_ce"])


def test_a_total_that_overflows_is_invalid():
    """A small T takes visits^(1/T) past float64: the total is inf, every t would be NaN, and the sample must not pass as scored."""
    late = _one(3, [60000, 50000, 7], late=1)
    lg = np.zeros((1, 128), np.float32)
    r = F.sample_scores(late, lg, np.array([0.5], np.float32), 0.01)[0]
    assert r["valid"] == 0 and r["policy_kl"] == 0 and r["policy_ce"] == 0 and r["value"] == 0
    assert F.sample_scores(late, lg, np.array([0.5], np.float32), 0.3)[0]["valid"] == 1
    assert F.sample_scores(_one(3, [60000, 50000, 7], late=0), lg, np.array([0.5], np.float32), 0.01)[0]["valid"] == 1


def test_policy_stats_view_and_dtypes():
    smp = surprise_records(9, 3)
    ps = F.policy_stats(smp)
    assert ps.dtype == F.POLICY_STATS_DTYPE and ps.shape == (9,)
    raw = smp.view(np.uint8).reshape(9, 640)
    assert (ps.view(np.uint8).reshape(9, 8) == raw[:, 120:128]).all()
    assert [F.POLICY_STATS_DTYPE.fields[n][1] for n in ("policy_kl", "has_policy_stats", "prior_top1", "zero")] == [0, 4, 5, 6]
    assert [F.SCORE_DTYPE.fields[n][1] for n in ("policy_kl", "policy_ce", "value", "top1", "valid", "zero")] == [0, 4, 8, 12, 13, 14]
    # the eight bytes lie inside ROOT_STATS_DTYPE's zero bytes: the root fields of the same record read as before
    assert (F.root_stats(smp)["has_root_stats"] == 0).all() and F.POLICY_STATS_OFFSET == 120


@pytest.mark.parametrize("n", [1, 3, 257, 1000])
def test_counts_are_one_without_weight_or_without_marks(n):
    smp = surprise_records(n, n)
    assert (F.surprise_counts(smp, 0.0, 1, 0) == 1).all()                           # alpha = 0
    zero = surprise_records(n, n, zero_kl=True)
    for alpha in (0.5, 1.0):
        assert (F.surprise_counts(zero, alpha, 1, 0) == 1).all()                     # S = 0
        c = F.surprise_counts(smp, alpha, 1, 0)
        assert (c[F.policy_stats(smp)["has_policy_stats"] != 1] == 1).all()          # unmarked records
        assert (c >= 0).all()
    unmarked = surprise_records(n, n, marked_share=0.0)
    assert (F.surprise_counts(unmarked, 1.0, 1, 0) == 1).all()


def test_weights_sum_to_the_marked_count():
    for n, seed in ((10, 1), (1000, 2), (20000, 3)):
        smp = surprise_records(n, seed)
        for alpha in (0.25, 1.0):
            w, marked, M, S = F.surprise_weights(smp, alpha)
            assert M == int(marked.sum()) > 0 and S > 0
            assert abs(float(np.sum(w[marked].astype(np.longdouble))) - M) <= 2.0 ** -40 * M
            assert (w[~marked] == 1.0).all()
            # the cap: 64 nats and no more
            q = F.surprise_q(F.policy_stats(smp)["policy_kl"])
            assert int(q.max()) == (64 << 20 if n >= 1000 else int(q.max())) <= 64 << 20      # 100-nat records are in the large sets
            assert w.max() <= (1 - alpha) + alpha * (64 << 20) * M / S + 1e-9
    assert list(F.surprise_q(np.array([-1.0, np.nan, 0.0, 2.0 ** -21, 3 * 2.0 ** -21, 64.0, 1e9], np.float32))) == \
        [0, 0, 0, 0, 2, 64 << 20, 64 << 20]                                          # ties to even; negatives and NaN count 0


def test_counts_depend_on_seed_and_epoch_and_not_on_place():
    smp = surprise_records(2000, 4)
    a = F.surprise_counts(smp, 0.5, 1, 0)
    assert (a != F.surprise_counts(smp, 0.5, 2, 0)).any() and (a != F.surprise_counts(smp, 0.5, 1, 1)).any()
    assert (a == F.surprise_counts(smp, 0.5, 1, 0)).all()
    perm = np.random.default_rng(0).permutation(len(smp))
    assert (F.surprise_counts(smp[perm], 0.5, 1, 0) == a[perm]).all()                # keyed by identity, not by place
    # expectation: the counts of the marked records add up to about M
    w, marked, M, _ = F.surprise_weights(smp, 1.0)
    assert abs(int(F.surprise_counts(smp, 1.0, 9, 0)[marked].sum()) - M) < 6 * np.sqrt(M)


def test_host_twin_equals_the_reference_on_5000_random_records():
    from xiangqi_alphazero_amd import hip
    hip.build()
    smp = surprise_records(5000, 17)
    ps = F.policy_stats(smp)
    for alpha, seed, epoch in ((0.0, 3, 0), (0.5, 0xFEDCBA9876543210, 7), (1.0, 12345, 2 ** 32 - 1)):
        ref = F.surprise_counts(smp, alpha, seed, epoch)
        _, marked, M, S = F.surprise_weights(smp, alpha)
        got = [hip.surprise_count_host(ps["policy_kl"][i], marked[i], M, S, alpha, seed, epoch, smp["slot"][i], smp["game_seq"][i],
                                       smp["ply"][i]) for i in range(len(smp))]
        assert (np.array(got, dtype=np.int32) == ref).all(), (alpha, seed, epoch)
    assert hip.surprise_count_host(1.0, 1, 5, 0, 1.0, 1, 0, 0, 0, 0) == 1            # S = 0
    assert hip.surprise_count_host(1.0, 0, 5, 50, 1.0, 1, 0, 0, 0, 0) == 1           # unmarked
    with pytest.raises(hip.XqError):
        hip.surprise_count_host(1.0, 1, 5, 50, 1.5, 1, 0, 0, 0, 0)
