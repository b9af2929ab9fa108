"""The table as opponent and teacher without a GPU (include/xq_hip.h, xq_tb_play_batch / xq_tb_samples; endgame.py; train_loop's
endgame_playout_* and endgame_teacher_* keys): the exports, the options struct, every argument error before any launch, the
Python layer's refusals by name, the seeded draw of entries, and the loop's option parsing."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import endgame_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xq_tb_play_batch", "xq_tb_samples"]


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _codes(*codes):
    return (C.c_int8 * max(len(codes), 1))(*codes), len(codes)


def test_exports_and_the_options_struct():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert C.sizeof(hip.TbSampleOpts) == 16
    assert re.search(r"typedef struct xq_tb_sample_opts\s*\{\s*int32_t policy;\s*int32_t reserved\[3\];\s*\}", code)
    assert "may alias dev_boards" in header and "ALIASING" in header        # the header says that a walk in place is allowed


def test_play_argument_errors_before_any_launch():
    hip, lib = _lib()
    ra, P = _codes(5, -2)
    bad, PB = _codes(8)
    one = C.c_void_p(64)                            # never dereferenced: every call below is refused or empty

    def call(pieces=ra, n_pieces=P, n=3, hole=None):
        a = [pieces, n_pieces, one, one, one, one, n, one, one, one, one, one, one, one, None]
        if hole is not None:
            a[hole] = None
        return lib.xq_tb_play_batch(*a)

    assert call(n=-1) == -1 and call(pieces=bad, n_pieces=PB) == -1 and call(n_pieces=6) == -1 and call(pieces=None) == -1
    assert call(pieces=bad, n_pieces=PB, n=0) == -1
    for hole in (2, 3, 4, 7, 8, 9, 10, 11, 12, 13):             # every pointer but dev_action
        assert call(hole=hole) == -1, hole
    assert lib.xq_tb_play_batch(ra, P, None, None, None, None, 0, None, None, None, None, None, None, None, None) == 0


def test_samples_argument_errors_before_any_launch():
    hip, lib = _lib()
    ra, P = _codes(5, -2)
    bad, PB = _codes(8)
    one = C.c_void_p(64)
    good = hip.TbSampleOpts(0, (C.c_int32 * 3)(0, 0, 0))

    def call(pieces=ra, n_pieces=P, n=3, opts=good, samples=one, hole=None):
        a = [pieces, n_pieces, one, one, n, None if opts is None else C.byref(opts), samples, one, None]
        if hole is not None:
            a[hole] = None
        return lib.xq_tb_samples(*a)

    assert call(n=-1) == -1 and call(pieces=bad, n_pieces=PB) == -1 and call(n_pieces=6) == -1 and call(pieces=None) == -1
    for hole in (2, 3, 6, 7):
        assert call(hole=hole) == -1, hole
    assert call(opts=None) == -1 and call(opts=None, n=0) == -1
    for misaligned in (72, 65, 68):
        assert call(samples=C.c_void_p(misaligned)) == -1, misaligned
    for policy in (-1, 2, 7):
        assert call(opts=hip.TbSampleOpts(policy, (C.c_int32 * 3)(0, 0, 0))) == -1, policy
    for word in range(3):
        r = [0, 0, 0]
        r[word] = 1
        assert call(opts=hip.TbSampleOpts(0, (C.c_int32 * 3)(*r))) == -1, word
        assert call(opts=hip.TbSampleOpts(0, (C.c_int32 * 3)(*r)), n=0) == -1, word
    assert call(opts=hip.TbSampleOpts(1, (C.c_int32 * 3)(0, 0, 0)), n=0) == 0
    assert lib.xq_tb_samples(ra, P, None, None, 0, C.byref(good), None, None, None) == 0


def test_python_layer_refuses_by_name():
    from xiangqi_alphazero_amd import hip
    table = torch.zeros(88452, dtype=torch.int16)
    boards, side = torch.zeros((2, 90), dtype=torch.int8), torch.ones(2, dtype=torch.int8)
    action = torch.zeros(2, dtype=torch.int16)
    index = torch.zeros(2, dtype=torch.int32)
    for call, word in ((lambda: hip.tb_play_batch("Ra", table[:5], boards, side), "table"),
                       (lambda: hip.tb_play_batch("Rz", table, boards, side), "signature"),
                       (lambda: hip.tb_play_batch("Ra", table, boards[:, :80], side), "boards"),
                       (lambda: hip.tb_play_batch("Ra", table, boards, side.to(torch.int32)), "boards"),
                       (lambda: hip.tb_play_batch("Ra", table, boards, side, action.to(torch.int32)), "action"),
                       (lambda: hip.tb_play_batch("Ra", table, boards, side, action[:1]), "action"),
                       (lambda: hip.tb_play_batch("Ra", table, boards, side, [1, 2]), "action"),
                       (lambda: hip.tb_play_batch("Ra", table, boards, side, out={"boards": boards}), "out"),
                       (lambda: hip.tb_samples("Ra", table[:5], index), "table"),
                       (lambda: hip.tb_samples("Ra", table, index.to(torch.int64)), "index"),
                       (lambda: hip.tb_samples("Ra", table, index.reshape(1, 2)), "index"),
                       (lambda: hip.tb_samples("Ra", table, [1, 2]), "index"),
                       (lambda: hip.tb_samples("Ra", table, index, policy=2), "policy"),
                       (lambda: hip.tb_samples("Ra", table, index, policy=True), "policy")):
        with pytest.raises(hip.XqError, match=word):
            call()
    # empty batches are no-ops with every output present
    out = hip.tb_play_batch("Ra", table, boards[:0], side[:0])
    assert set(out) == {"boards", "side", "played", "value", "move_value", "value_out", "status"}
    assert all(len(v) == 0 for v in out.values()) and out["boards"].shape == (0, 90)
    rows, status = hip.tb_samples("Ra", table, index[:0], policy=1)
    assert rows.shape == (0, 640) and rows.dtype == torch.uint8 and status.shape == (0,)


def _tb(signature):
    from xiangqi_alphazero_amd import endgame
    return endgame.Tablebase(signature, EM.model(signature).table, device="cpu")


def test_endgame_layer_refuses_by_name():
    from xiangqi_alphazero_amd import endgame, hip
    tb = _tb("R")
    m = EM.model("R")
    for call, word in ((lambda: tb.samples([1, 2], invalid="skip"), "invalid"), (lambda: tb.samples([1.5]), "index"),
                       (lambda: tb.play(m.boards[:2], m.sides[:2], [1]), "actions"),
                       (lambda: tb.play(m.boards[:2], m.sides[:2], [1, 70000]), "actions"),
                       (lambda: tb.play(m.boards[:2], m.sides[:3]), "sides"),
                       (lambda: endgame.play_out_with(None, "R", m.boards[:2], m.sides[:2], 4), "tb"),
                       (lambda: endgame.play_out_with(None, tb, m.boards[:2], m.sides[:2], 0), "max_plies"),
                       (lambda: endgame.play_out_with(None, tb, m.boards[:2], m.sides[:2], True), "max_plies"),
                       (lambda: endgame.play_out(None, "R", m.boards[:2], m.sides[:2], 8), "tb"),
                       (lambda: endgame.play_out(None, tb, m.boards[:2], m.sides[:2], 0), "num_simulations"),
                       (lambda: endgame.play_out(None, tb, m.boards[:2], m.sides[:2], 8, max_plies=0), "max_plies"),
                       (lambda: endgame.play_out(None, tb, m.boards[:2], m.sides[:2], 8, chunk=0), "chunk")):
        with pytest.raises(hip.XqError, match=word):
            call()
    # an empty set of positions is played out without a launch
    out = endgame.play_out_with(lambda games: [], tb, m.boards[:0], m.sides[:0], 4)
    assert out["positions"] == 0 and out["conversion_rate"] == 0.0 and out["games"] == []
    assert [out[k] for k in endgame.OUTCOMES] == [0, 0, 0, 0]


def test_entries_of_is_a_seeded_draw():
    from xiangqi_alphazero_amd import endgame, hip
    tb = _tb("Ra")
    t = tb.table.astype(np.int64)
    half = len(t) // 2
    boards, sides, idx = tb.entries_of(n=300, seed=4)
    assert idx.dtype == np.int64 and len(set(idx.tolist())) == 300 and (np.diff(idx) > 0).all()
    assert (t[idx] != endgame.INVALID).all() and (t[idx] != -1).all() and (EM.model("Ra").counts[idx] > 0).all()
    assert {"win", "draw", "loss"} == {("win" if v > 0 else "draw" if v == 0 else "loss") for v in t[idx].tolist()}
    assert (endgame.index_to_board("Ra", idx)[0] == boards).all() and (endgame.index_to_board("Ra", idx)[1] == sides).all()
    assert (tb.entries_of(n=300, seed=4)[2] == idx).all() and (tb.entries_of(n=300, seed=5)[2] != idx).any()
    # kinds, side and min_plies
    assert (t[tb.entries_of(("win",), 100, seed=1)[2]] > 0).all() and (t[tb.entries_of("draw", 100, seed=1)[2]] == 0).all()
    lost = t[tb.entries_of(("loss",), 100, seed=1)[2]]
    assert (lost < -1).all()
    both = t[tb.entries_of(("win", "loss"), 400, seed=2, min_plies=4)[2]]
    assert (both != 0).all() and ((both >= 4) | (-both - 1 >= 4)).all() and (both > 0).any() and (both < 0).any()
    b, s, i = tb.entries_of(("win", "draw"), 50, seed=3, side=-1)
    assert (i >= half).all() and (s == -1).all() and (t[i] >= 0).all()
    assert (tb.entries_of(("win",), 50, seed=3, side=1)[2] < half).all()
    # the whole pool, and one more than it
    pool = int(((t != endgame.INVALID) & (t != -1)).sum())
    assert len(tb.entries_of(n=pool)[2]) == pool
    # "win" alone with min_plies is `positions`
    assert (tb.entries_of(("win",), 60, seed=9, min_plies=3)[2] == tb.positions("win", 60, seed=9, min_plies=3)[2]).all()
    for call, word in ((lambda: tb.entries_of(("won",), 3), "kinds"), (lambda: tb.entries_of((), 3), "kinds"),
                       (lambda: tb.entries_of(n=3, side=0), "side"), (lambda: tb.entries_of(n=-1), "n"),
                       (lambda: tb.entries_of(n=2.5), "n"), (lambda: tb.entries_of(n=3, min_plies=-1), "min_plies"),
                       (lambda: tb.entries_of(n=pool + 1), "entries")):
        with pytest.raises(hip.XqError, match=word):
            call()


def test_loop_reads_and_refuses_the_new_keys(tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=4, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=6, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path))

    def loop(**extra):
        return train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, **extra), device="cpu", seed=1)

    # without the new keys the loop's endgame options are today's, and nothing of the new kind is on
    plain = loop(endgame_signature="R")
    assert plain.endgame == dict(signature="R", positions=256, kind="win", simulations=6, interval=1, rescore=False)
    assert plain.endgame_playout is None and plain.endgame_teacher is None
    off = loop()
    assert off.endgame is None and off.endgame_playout is None and off.endgame_teacher is None
    assert loop(endgame_signature="R", endgame_playout_max_plies=5, endgame_teacher_policy=1).endgame_playout is None
    on = loop(endgame_signature="R", endgame_playout_positions=8, endgame_playout_max_plies=12, endgame_teacher_samples=16,
              endgame_teacher_policy=1)
    assert on.endgame_playout == dict(positions=8, max_plies=12) and on.endgame_teacher == dict(samples=16, policy=1)
    assert on.endgame == plain.endgame
    dflt = loop(endgame_signature="R", endgame_playout_positions=8, endgame_teacher_samples=1)
    assert dflt.endgame_playout == dict(positions=8, max_plies=100) and dflt.endgame_teacher == dict(samples=1, policy=0)
    for extra, key in ((dict(endgame_signature="R", endgame_playout_positions=0), "endgame_playout_positions"),
                       (dict(endgame_signature="R", endgame_playout_positions=2.5), "endgame_playout_positions"),
                       (dict(endgame_signature="R", endgame_playout_positions=True), "endgame_playout_positions"),
                       (dict(endgame_playout_positions=8), "endgame_playout_positions"),            # no signature
                       (dict(endgame_signature="R", endgame_playout_positions=8, endgame_playout_max_plies=0), "endgame_playout_max_plies"),
                       (dict(endgame_playout_max_plies="9"), "endgame_playout_max_plies"),     # checked even while off
                       (dict(endgame_signature="R", endgame_teacher_samples=0), "endgame_teacher_samples"),
                       (dict(endgame_teacher_samples=16), "endgame_teacher_samples"),               # no signature
                       (dict(endgame_signature="R", endgame_teacher_samples=4, endgame_teacher_policy=2), "endgame_teacher_policy"),
                       (dict(endgame_signature="R", endgame_teacher_policy=False), "endgame_teacher_policy")):
        with pytest.raises(hip.XqError, match=key):
            loop(**extra)
