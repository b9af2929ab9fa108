"""The evaluation mirror's bit without a GPU: the Python transcription (tests/eval_mirror_model.py) against the device's own code
on the host (hip.eval_mirror_bit), and the bit's balance.  The function is fixed, so the balance bounds are conditions: should a
packing land outside them it mixes badly and the packing is what changes, not the bounds."""
import random

import pytest

import eval_mirror_model as M

BASE = dict(seed=9, rank=0, slot=3, game_seq=1, ply=5, is_root=0, sims_done=7, row=0)
EXTREMES = dict(seed=(0, 1, 2 ** 32, 2 ** 64 - 1), rank=(0, 7, 2 ** 31 - 1), slot=(0, 1, 8191), game_seq=(0, 1, 2 ** 32 - 1),
                ply=(0, 1, 199, 65535), is_root=(0, 1), sims_done=(0, 1, 15999), row=(0, 1, 63))


@pytest.fixture(scope="module")
def bit():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.eval_mirror_bit


def test_model_equals_the_host_export(bit):
    rng = random.Random(17)
    tuples = [dict(BASE)]
    for name, values in EXTREMES.items():              # every field at its extremes, the others at the base and at random
        for v in values:
            tuples.append({**BASE, name: v})
            tuples.append({**{n: rng.choice(vs) for n, vs in EXTREMES.items()}, name: v})
    tuples.append({n: vs[-1] for n, vs in EXTREMES.items()})
    for _ in range(3000):
        tuples.append(dict(seed=rng.getrandbits(64), rank=rng.randrange(8), slot=rng.randrange(8192), game_seq=rng.getrandbits(32),
                           ply=rng.randrange(65536), is_root=rng.randrange(2), sims_done=rng.randrange(16000), row=rng.randrange(64)))
    assert len(tuples) > 3000
    ones = 0
    for t in tuples:
        got = bit(**t)
        assert got == M.mirror_bit(**t), t
        ones += got
    assert 0.4 * len(tuples) < ones < 0.6 * len(tuples)


def test_host_export_refuses_out_of_range_arguments(bit):
    from xiangqi_alphazero_amd import hip
    lib = hip.lib()
    ok = (9, 0, 3, 1, 5, 0, 7, 0)
    assert lib.xq_eval_mirror_bit_host(*ok) in (0, 1)
    for i, bad in ((1, -1), (2, -1), (4, -1), (5, 2), (5, -1), (6, -1), (6, 16000), (7, -1), (7, 64)):
        args = list(ok)
        args[i] = bad
        assert lib.xq_eval_mirror_bit_host(*args) == -1, (i, bad)
        with pytest.raises(hip.XqError):
            hip.eval_mirror_bit(*args)
    for seed, gseq in ((-1, 0), (2 ** 64, 0), (0, -1), (0, 2 ** 32)):
        with pytest.raises(hip.XqError):
            hip.eval_mirror_bit(seed, 0, 3, gseq, 5, 0, 7, 0)


def test_balance_over_slots_and_simulations(bit):
    ones = sum(bit(9, 0, slot, 0, 3, 0, sims, 0) for slot in range(64) for sims in range(64))
    print("ones of 4096:", ones)
    assert 1920 <= ones <= 2176                        # 2048 +- 4 sigma, sigma = 32


@pytest.mark.parametrize("field", ["slot", "game_seq", "ply", "sims_done", "seed", "rank"])
def test_balance_of_each_field_varied_alone(bit, field):
    ones = sum(bit(**{**BASE, field: v}) for v in range(256))
    print(field, "ones of 256:", ones)
    assert 96 <= ones <= 160


def test_balance_over_rows_and_root_against_leaf(bit):
    rows = sum(bit(**{**BASE, "row": r}) for r in range(64))
    differ = sum(bit(**{**BASE, "slot": s, "is_root": 1}) != bit(**{**BASE, "slot": s, "is_root": 0}) for s in range(256))
    print("rows: ones of 64:", rows, " root against leaf: differ of 256:", differ)
    assert 16 <= rows <= 48
    assert 96 <= differ <= 160


def test_model_action_mirror_is_the_golden_permutation():
    import os

    import numpy as np
    perm = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flip_perm.npy"))
    assert [M.mirror_action(a) for a in range(8100)] == perm.tolist()
