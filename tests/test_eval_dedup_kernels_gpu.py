"""The request dedup's kernels (csrc/xq_evdedup.hip: k_dedup_keys with wave_evkey, k_dedup_resolve, k_compact_unique) held to the
host twin of tests/eval_dedup_model.py through hip.dedup_requests, the engine's own kernels over rows of the test's own: rep[],
the packed rows[], their number and the four counters, all exactly equal; nothing of an idle row written; the table empty again
after every call, so that a second call on the same object answers the same.  tests/test_eval_dedup_model.py shows what the
streams used here can tell apart."""
import numpy as np
import pytest

import eval_dedup_model as M

pytestmark = pytest.mark.gpu

SENT = -77                                                # what the output arrays hold where nothing may be written
NAMES = [f"{kind}_{n}" for n in M.SIZES for kind in ("identical", "distinct", "mixed")] + \
        ["idle_twins", "nibble_variants", "count_mismatch", "bucket_collision"]


@pytest.fixture(scope="module")
def cases():
    from xiangqi_alphazero_amd import hip
    hip.build()
    c = M.cases()
    assert sorted(c) == sorted(NAMES)
    return c


def _call(hip, torch, table, x, counts, live):
    n = x.shape[0]
    out = tuple(torch.full((k,), SENT, dtype=torch.int32, device="cuda") for k in (n, n, 1))
    rep, rows, n_live = hip.dedup_requests(x, counts, live, table, out=out)
    torch.cuda.synchronize()
    return rep.cpu().numpy(), rows.cpu().numpy(), int(n_live.cpu().numpy()[0])


@pytest.mark.parametrize("name", NAMES)
def test_kernels_against_the_twin(cases, name):
    import torch
    from xiangqi_alphazero_amd import hip
    nib, counts, live = cases[name]
    n = len(nib)
    keys = M.keys_of(nib)
    want_rep, want_rows, want_st = M.DedupModel().resolve(keys, counts, live, M.table_size(n))
    table = hip.DedupTable(n)
    assert table.table_size == M.table_size(n) and (table.table() == M.EMPTY).all().item()
    x = torch.from_numpy(M.planes_of(nib)).cuda()
    counts_d, live_d = torch.from_numpy(counts).cuda(), torch.from_numpy(live).cuda()
    expect_rep = np.full(n, SENT, np.int32)
    for s, m in want_rep.items():
        expect_rep[s] = m
    expect_rows = np.full(n, SENT, np.int32)
    expect_rows[:len(want_rows)] = want_rows
    for call in (1, 2):                                                   # the second call finds the table empty again
        rep, rows, n_live = _call(hip, torch, table, x, counts_d, live_d)
        print(f"{name} call {call}: n_live {n_live}, stats {table.stats()}")
        assert n_live == len(want_rows)
        assert rep.tolist() == expect_rep.tolist()                        # an idle row's entry keeps the sentinel
        assert rows.tolist() == expect_rows.tolist()                      # nothing past n_live is written
        assert table.stats() == {k: call * v for k, v in want_st.items()}
        assert (table.table() == M.EMPTY).all().item()
        got_keys = table.keys().cpu().numpy().view(np.uint32)
        for s in range(n):
            assert got_keys[s].tobytes() == (keys[s] if live[s] else bytes(48)), f"key of row {s}"
    if name == "idle_twins":
        assert all(live[m] for m in rep[live != 0].tolist())              # the representative is live
    if name == "bucket_collision":
        assert table.table_size == 16 and table.stats()["collisions"] == 4 and n_live == 4
    if name == "count_mismatch":
        assert table.stats()["mismatches"] == 2


def test_a_table_serves_fewer_rows_than_it_was_made_for(cases):
    """One object over changing requests, as an engine's is: every answer is the twin's for that call alone."""
    import torch
    from xiangqi_alphazero_amd import hip
    table = hip.DedupTable(1030)
    total = dict.fromkeys(M.COUNTERS, 0)
    for name in ("mixed_1030", "identical_5", "mixed_1030", "idle_twins", "distinct_1030", "count_mismatch"):
        nib, counts, live = cases[name]
        want_rep, want_rows, want_st = M.DedupModel().resolve(M.keys_of(nib), counts, live, table.table_size)
        rep, rows, n_live = _call(hip, torch, table, torch.from_numpy(M.planes_of(nib)).cuda(), torch.from_numpy(counts).cuda(),
                                  torch.from_numpy(live).cuda())
        assert n_live == len(want_rows) and rows[:n_live].tolist() == want_rows
        assert {s: int(rep[s]) for s in want_rep} == want_rep
        total = {k: total[k] + want_st[k] for k in total}
        assert table.stats() == total and (table.table() == M.EMPTY).all().item()
    rep, rows, n_live = hip.dedup_requests(torch.zeros((0, 15, 10, 9), device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                                           torch.zeros(0, dtype=torch.int32, device="cuda"), table,
                                           out=(torch.zeros(0, dtype=torch.int32, device="cuda"),
                                                torch.zeros(0, dtype=torch.int32, device="cuda"),
                                                torch.full((1,), SENT, dtype=torch.int32, device="cuda")))
    assert int(n_live.cpu()[0]) == 0 and table.stats() == total
    with pytest.raises(hip.XqError):
        hip.dedup_requests(torch.zeros((5, 15, 10, 9), device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda"),
                           torch.zeros(5, dtype=torch.int32, device="cuda"), hip.DedupTable(4))
