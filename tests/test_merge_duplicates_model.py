"""CPU checks of merging duplicate positions: the host twin xq_position_key_host against the numpy reference
sample_format.position_key on every corpus board and its mirror image, for both flag values; the pairs that must get different
keys; and the properties of the numpy model of the groups and of the merged targets."""
import numpy as np
import pytest

from golden_io import corpus
from merge_duplicates_records import boundary_pairs, group_buffer, initial_board, make_group, mirror_board, records_of
from xiangqi_alphazero_amd import sample_format as F


@pytest.fixture(scope="module")
def hip():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip


@pytest.fixture(scope="module")
def corpus_keys(hip):
    """(board, image, side) -> host and reference (key, mirrored) for both flag values, computed once."""
    d = corpus()
    boards = d["board"].astype(np.int8)
    images = mirror_board(boards)
    out = {}
    for mirror in (False, True):
        for name, bs in (("board", boards), ("image", images)):
            out[name, mirror, "host"] = [hip.position_key_host(b, int(s), mirror) for b, s in zip(bs, d["side"])]
            out[name, mirror, "ref"] = [F.position_key(b, int(s), mirror) for b, s in zip(bs, d["side"])]
    return boards, images, out


def test_host_twin_equals_the_numpy_reference_on_the_corpus(corpus_keys):
    boards, images, k = corpus_keys
    assert len(boards) == 4819
    for mirror in (False, True):
        for name in ("board", "image"):
            assert k[name, mirror, "host"] == k[name, mirror, "ref"], (name, mirror)
    assert all(m == 0 for _, m in k["board", False, "host"] + k["image", False, "host"])
    symmetric = (boards == images).all(axis=1)
    for i in range(len(boards)):
        (ka, ma), (kb, mb) = k["board", True, "host"][i], k["image", True, "host"][i]
        assert ka == kb, i
        assert (ma, mb) == (0, 0) if symmetric[i] else ma + mb == 1, i
        if not symmetric[i]:                                          # without the flag the two orientations are two positions
            assert k["board", False, "host"][i][0] != k["image", False, "host"][i][0], i
        assert ka == (k["board", False, "host"][i][0] if ma == 0 else k["image", False, "host"][i][0]), i
    # the canonical board's plain key IS the mirror key
    for i in range(0, len(boards), 97):
        c, m = F.canonical_board(boards[i], True)
        assert F.position_key(c, int(corpus()["side"][i]), False)[0] == k["board", True, "ref"][i][0]
        assert np.array_equal(c, images[i] if m else boards[i])


def test_corpus_has_4542_classes_and_4542_keys(hip):
    boards = corpus()["board"].astype(np.int8)
    keys = {hip.position_key_host(b, 1, True)[0] for b in boards}
    canon = {F.canonical_board(b, True)[0].tobytes() for b in boards}
    assert len(keys) == 4542 and len(canon) == 4542


def test_pairs_that_must_get_different_keys(hip):
    for a, sa, b, sb, what in boundary_pairs():
        for mirror in (False, True):
            ka, kb = hip.position_key_host(a, sa, mirror), hip.position_key_host(b, sb, mirror)
            assert ka[0] != kb[0], (what, mirror)
            assert ka == F.position_key(a, sa, mirror) and kb == F.position_key(b, sb, mirror), (what, mirror)
    init = initial_board()
    assert np.array_equal(init, mirror_board(init))
    assert hip.position_key_host(init, 1, True)[1] == 0 and F.position_key(init, 1, True)[1] == 0
    assert hip.position_key_host(init, 1, True)[0] != hip.position_key_host(init, -1, True)[0]


def test_groups_partition_the_records_in_age_order():
    smp, (offsets, members, mirrored), notes = group_buffer(False)
    n = len(smp)
    assert sorted(members.tolist()) == list(range(n)) and offsets[0] == 0 and offsets[-1] == n and len(mirrored) == n
    sizes = np.diff(offsets)
    assert (sizes > 0).all() and sorted(sizes.tolist()) == sorted([2, 3, 64, 65, 200, 3, 5, 3, 1, 1, 1])
    firsts = []
    for g in range(len(sizes)):
        mem = members[offsets[g]:offsets[g + 1]]
        assert (np.diff(mem) > 0).all(), g                               # age order inside a group
        firsts.append(int(mem[0]))
        canon = {(F.canonical_board(smp["board"][r], True)[0].tobytes(), int(smp["side"][r])) for r in mem}
        assert len(canon) == 1, g
        for r, m in zip(mem, mirrored[offsets[g]:offsets[g + 1]]):
            assert m == F.position_key(smp["board"][r], int(smp["side"][r]), True)[1]
    assert firsts == sorted(firsts)                                       # groups numbered by their oldest member
    # without the mirror a position and its image are two groups
    off2, mem2, mir2 = F.position_groups(smp, False)
    assert len(off2) - 1 > len(sizes) and not mir2.any() and sorted(mem2.tolist()) == list(range(n))


def test_equal_keys_of_different_positions_split_a_group_a_b_a():
    d = corpus()
    a, b = d["board"][10].astype(np.int8), d["board"][2000].astype(np.int8)
    smp = records_of(np.array([a, b, a, mirror_board(a), b]), np.array([1, 1, 1, 1, -1], dtype=np.int8))
    keys = np.full(5, 12345, dtype=np.uint64)
    offsets, members, mirrored = F.position_groups(smp, True, keys=keys)
    # predecessor rule over A, B, A, A', B(other side): A | B | A A' | B-
    assert offsets.tolist() == [0, 1, 2, 4, 5] and members.tolist() == [0, 1, 2, 3, 4]
    assert mirrored[2] + mirrored[3] == 1
    # with the real keys the three records of A are one group
    offsets, members, _ = F.position_groups(smp, True)
    assert offsets.tolist() == [0, 3, 4, 5] and members.tolist() == [0, 2, 3, 1, 4]


def test_group_of_one_reproduces_the_dense_reference():
    rng = np.random.default_rng(5)
    d = corpus()
    smp = np.concatenate([make_group(d["board"][50 + 400 * j].astype(np.int8), int(d["side"][50 + 400 * j]), 1, rng, (kind,))
                          for j, kind in enumerate(("plain", "late_temp", "gumbel", "no_visits"))])
    smp["slot"], smp["game_seq"], smp["ply"] = 3, np.arange(len(smp)), 0
    res = np.zeros(len(smp), dtype=F.RESULT_DTYPE)
    res["slot"], res["game_seq"] = smp["slot"], smp["game_seq"]
    for q_mix in (0.0, 0.25):
        dense, _ = F.to_reference_tuples(smp, res, 0.3, augment=True, q_mix=q_mix)
        groups = (np.arange(len(smp) + 1, dtype=np.int32), np.arange(len(smp), dtype=np.int32), np.zeros(len(smp), dtype=np.uint8))
        logical = np.arange(2 * len(smp))
        st, pi, z = F.merged_targets(smp, groups, logical // 2, logical % 2, 0.3, q_mix)
        for j in range(2 * len(smp)):
            assert np.array_equal(st[j], dense[j][0]), j
            np.testing.assert_allclose(pi[j], dense[j][1].astype(np.float32), rtol=2e-7, atol=0, err_msg=str(j))
            if not smp[j // 2]["late_temp"]:
                assert np.array_equal(pi[j], dense[j][1].astype(np.float32)), j
            assert z[j] == np.float32(dense[j][2]) == F.mixed_z(smp[j // 2:j // 2 + 1], q_mix)[0], j
        # a member stored mirrored under flip f is the record under flip 1 - f
        gm = (groups[0], groups[1], np.ones(len(smp), dtype=np.uint8))
        st2, pi2, z2 = F.merged_targets(smp, gm, logical // 2, 1 - logical % 2, 0.3, q_mix)
        assert np.array_equal(st, st2) and np.array_equal(pi, pi2) and np.array_equal(z, z2)


def test_merged_targets_are_means_and_handle_the_edges():
    smp, groups, notes = group_buffer(True)
    offsets, members, mirrored = groups
    n_groups = len(offsets) - 1
    sizes = np.diff(offsets)
    group = np.array(list(range(n_groups)) + [-1, n_groups], dtype=np.int32)
    st, pi, z = F.merged_targets(smp, groups, group, np.zeros(len(group), dtype=np.uint8), 0.3, 0.25)
    assert not st[-2:].any() and not pi[-2:].any() and not z[-2:].any()
    for g in range(n_groups):
        mem = members[offsets[g]:offsets[g + 1]]
        valid = [r for r in mem if smp["visits"][r][:smp["n_moves"][r]].sum() > 0]
        if valid:
            assert abs(float(pi[g].astype(np.float64).sum()) - 1.0) < 1e-5, g
        else:
            assert not pi[g].any(), g
        want_z = np.mean([float(F.mixed_z(smp[r:r + 1], 0.25)[0]) for r in mem])
        assert abs(float(z[g]) - want_z) < 1e-6, g
    all_invalid = [g for g in range(n_groups) if sizes[g] == 3 and not pi[g].any()]
    assert len(all_invalid) == 1
    # an empty group gives zeros too
    big = int(np.argmax(sizes))
    off_e = np.array([offsets[big], offsets[big], offsets[big + 1]], dtype=np.int32)
    st, pi, z = F.merged_targets(smp, (off_e, members, mirrored), np.array([0, 1]), np.zeros(2, dtype=np.uint8), 0.3, 0.0)
    assert not st[0].any() and not pi[0].any() and z[0] == 0 and pi[1].any()
