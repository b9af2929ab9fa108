"""What the crafted streams of tests/eval_dedup_model.py can tell apart (CPU): the twin's answers on them are the ones the rules
of include/xq_hip.h give by hand, and each of four wrong dedups differs from the twin on the stream made for it -- so a kernel
that agrees with the twin on these streams (tests/test_eval_dedup_kernels_gpu.py) is none of them."""
import numpy as np
import pytest

import eval_dedup_model as M


@pytest.fixture(scope="module")
def lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


@pytest.fixture(scope="module")
def cases(lib):
    return M.cases()


def _run(model, case):
    nib, counts, live = case
    return model.resolve(M.keys_of(nib), counts, live, M.table_size(len(nib)))


class MaxWins(M.DedupModel):                       # a maximum instead of the minimum
    def pick(self, members):
        return max(members)


class BucketIsKey(M.DedupModel):                   # no full-key compare after a bucket hit
    def same_key(self, a, b):
        return True


class CountIgnored(M.DedupModel):
    def same_count(self, a, b):
        return True


class IdleRepresents(M.DedupModel):                # an idle row enters the table and may be chosen
    def enters_table(self, live):
        return True


def test_table_size():
    assert [M.table_size(g) for g in (1, 3, 4, 5, 8, 1024, 1030, 8192)] == [16, 16, 16, 32, 32, 4096, 8192, 32768]
    from xiangqi_alphazero_amd import hip
    assert all(hip.dedup_table_size(g) == M.table_size(g) for g in range(1, 300))


def test_the_twin_on_the_crafted_streams(cases):
    twin = M.DedupModel()
    for n in M.SIZES:
        rep, rows, st = _run(twin, cases[f"identical_{n}"])
        assert rep == {s: 0 for s in range(n)} and rows == [0] and st == dict(requests=n, merged=n - 1, collisions=0, mismatches=0)
        rep, rows, st = _run(twin, cases[f"distinct_{n}"])
        assert rep == {s: s for s in range(n)} and rows == list(range(n))
        assert st["requests"] == n and st["merged"] == 0 and st["mismatches"] == 0
        nib, counts, live = cases[f"mixed_{n}"]
        rep, rows, st = _run(twin, cases[f"mixed_{n}"])
        keys = M.keys_of(nib)
        assert sorted(rep) == np.flatnonzero(live).tolist() and st["requests"] == int(live.sum())
        assert all(live[m] and keys[m] == keys[s] and m <= s for s, m in rep.items())        # a representative is live and equal
        assert st["requests"] - st["merged"] == len(rows) and st["mismatches"] == 0
        if st["collisions"] == 0:                                                             # then every group has one row
            assert len(rows) == len({keys[s] for s in rep})
    assert cases["distinct_1030"][0].shape == (1030, 91) and len(set(M.keys_of(cases["distinct_1030"][0]))) == 1030
    rep, rows, st = _run(twin, cases["idle_twins"])
    assert rep == {1: 1, 2: 2, 3: 1} and rows == [1, 2] and st == dict(requests=3, merged=1, collisions=0, mismatches=0)
    rep, rows, st = _run(twin, cases["nibble_variants"])
    assert len(set(M.keys_of(cases["nibble_variants"][0]))) == 92
    assert rep == {s: s for s in range(92)} and rows == list(range(92)) and st["merged"] == 0 and st["mismatches"] == 0
    rep, rows, st = _run(twin, cases["count_mismatch"])
    assert rep == {0: 0, 1: 1, 2: 0} and rows == [0, 1] and st == dict(requests=3, merged=1, collisions=0, mismatches=1)
    nib = cases["bucket_collision"][0]
    keys = M.keys_of(nib)
    assert len(nib) == 4 and M.table_size(4) == 16 and keys[0] != keys[1] == keys[2] and keys[3] not in keys[:3]
    assert M.lib_bucket(keys[0], 16) == M.lib_bucket(keys[1], 16) != M.lib_bucket(keys[3], 16)
    rep, rows, st = _run(twin, cases["bucket_collision"])
    # both higher rows evaluate themselves: the bucket's minimum holds another key, and nobody else is asked
    assert rep == {0: 0, 1: 1, 2: 2, 3: 3} and rows == [0, 1, 2, 3] and st == dict(requests=4, merged=0, collisions=2, mismatches=0)


@pytest.mark.parametrize("mutant, case", [(MaxWins, "identical_3"), (MaxWins, "identical_1030"), (MaxWins, "mixed_1030"),
                                          (BucketIsKey, "bucket_collision"), (CountIgnored, "count_mismatch"),
                                          (IdleRepresents, "idle_twins"), (IdleRepresents, "mixed_1030")])
def test_the_streams_tell_the_twin_from_the_wrong_ones(cases, mutant, case):
    want = _run(M.DedupModel(), cases[case])
    got = _run(mutant(), cases[case])
    assert got[0] != want[0], f"{mutant.__name__} answers {case} as the twin does"


def test_the_wrong_ones_in_detail(cases):
    assert _run(MaxWins(), cases["identical_3"])[0] == {0: 2, 1: 2, 2: 2}
    rep, rows, st = _run(BucketIsKey(), cases["bucket_collision"])
    assert rep[1] == 0 and rep[2] == 0 and st["collisions"] == 0            # two different positions merged: a wrong answer
    rep, rows, st = _run(CountIgnored(), cases["count_mismatch"])
    assert rep == {0: 0, 1: 0, 2: 0} and st["mismatches"] == 0
    rep, rows, st = _run(IdleRepresents(), cases["idle_twins"])
    assert rep[1] == 0 and rep[3] == 0 and rows == [2]                      # row 0 asks for nothing: nobody evaluates the position
