"""The endgame tablebases without a GPU (include/xq_hip.h, xq_tb_*; endgame.py; train_loop's endgame keys): the exports and
constants, the entry counts, every argument error before any launch, the numpy layout, saving and loading, and the loop's option
parsing."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xq_tb_entries", "xq_tb_init", "xq_tb_pass", "xq_tb_probe_batch"]
ENTRIES = {"": 162, "P": 9072, "R": 14742, "C": 14742, "N": 14742, "aa": 5832, "Ra": 88452, "CA": 88452, "Ca": 88452,
           "Pa": 54432, "Nb": 117936, "p": 9072, "Pp": 508032, "RNa": 8049132, "rnA": 8049132, "Raabb": 33965568}


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def _codes(*codes):
    return (C.c_int8 * max(len(codes), 1))(*codes), len(codes)


def test_exports_and_constants():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in hip.EXPORTS and hasattr(lib, name)
    for macro, value in (("XQ_TB_MAX_PIECES", 5), ("XQ_TB_MAX_ENTRIES", 1 << 28), ("XQ_TB_MAX_PASSES", 32000),
                         ("XQ_TB_INVALID", -32768), ("XQ_TB_NO_MOVE", 0xFFFF)):
        text = re.search(r"#define\s+%s\s+(.+)" % macro, code).group(1).strip()
        assert eval(text, {}) == value == getattr(hip, macro[3:]), macro
    assert "IN PLACE IS EXACT" in header          # the header argues why one table suffices


def test_entry_counts():
    hip, lib = _lib()
    from xiangqi_alphazero_amd import endgame
    for sig, n in ENTRIES.items():
        assert hip.tb_entries(sig) == n == endgame.entries(sig), sig
        arr, P = _codes(*endgame.parse_signature(sig))
        assert lib.xq_tb_entries(arr, P) == n
    assert lib.xq_tb_entries(None, 0) == 162
    # refused: codes 1, 8 and 0, six pieces, a NULL list, and a signature beyond 2^28 entries
    for bad in ((1,), (8,), (0,), (-1,), (5, -8), (5, 5, 5, 5, 5, 5)):
        arr, P = _codes(*bad)
        assert lib.xq_tb_entries(arr, P) == 0, bad
    assert lib.xq_tb_entries(None, 1) == 0 and lib.xq_tb_entries(None, -1) == 0
    arr, P = _codes(5, 4, 6, -5, -4)                # "RNCrn"
    assert lib.xq_tb_entries(arr, P) == 0
    with pytest.raises(hip.XqError, match="RNCrn"):
        hip.tb_entries("RNCrn")


def test_signatures():
    from xiangqi_alphazero_amd import endgame, hip
    assert endgame.parse_signature("") == () and endgame.parse_signature("Ra") == (5, -2)
    assert endgame.parse_signature("ABNRC") == (2, 3, 4, 5, 6) and endgame.parse_signature("bnrcp") == (-3, -4, -5, -6, -7)
    assert endgame.parse_signature("EHeh") == (3, 4, -3, -4) and endgame.parse_signature([5, -2]) == (5, -2)
    assert endgame.signature_text((5, -2, -3)) == "Rab" and endgame.signature_text("Eh") == "Bn"
    for bad, word in (("K", "K"), ("Rx", "x"), ("RRRRRR", "6 pieces"), ([1], "codes"), ([5, 8], "codes"), ([2.5], "codes"), (7, "signature")):
        with pytest.raises(hip.XqError, match=word):
            endgame.parse_signature(bad)
    assert [len(endgame.piece_squares(c)) for c in (2, 3, 4, 5, 6, 7)] == [5, 7, 90, 90, 90, 55]
    assert endgame.piece_squares(2).tolist() == [3, 5, 13, 21, 23]
    assert endgame.piece_squares(3).tolist() == [2, 6, 18, 22, 26, 38, 42]
    for c in (2, 3, 7):
        assert endgame.piece_squares(-c).tolist() == sorted(89 - s for s in endgame.piece_squares(c).tolist())


def test_argument_errors_before_any_launch():
    hip, lib = _lib()
    ra, P = _codes(5, -2)
    bad, PB = _codes(8)
    word = C.c_int32(0)
    one = C.c_void_p(64)                            # never dereferenced: every call below is refused or empty
    assert lib.xq_tb_init(ra, P, None, None) == -1
    assert lib.xq_tb_init(bad, PB, one, None) == -1 and lib.xq_tb_init(ra, 6, one, None) == -1
    assert lib.xq_tb_init(None, 2, one, None) == -1
    for k in (0, -1, 32001):
        assert lib.xq_tb_pass(ra, P, one, k, one, None) == -1, k
    assert lib.xq_tb_pass(ra, P, None, 1, one, None) == -1 and lib.xq_tb_pass(ra, P, one, 1, None, None) == -1
    assert lib.xq_tb_pass(bad, PB, one, 1, C.byref(word), None) == -1
    args = [one] * 8
    assert lib.xq_tb_probe_batch(ra, P, one, one, one, -1, *args[:6], None) == -1
    assert lib.xq_tb_probe_batch(bad, PB, one, one, one, 0, *args[:6], None) == -1
    assert lib.xq_tb_probe_batch(ra, P, None, None, None, 0, None, None, None, None, None, None, None) == 0      # an empty batch
    for hole in (2, 3, 4, 6, 7, 8, 10, 11):         # every pointer but dev_move_value
        a = [ra, P, one, one, one, 3, one, one, one, one, one, one, None]
        a[hole] = None
        assert lib.xq_tb_probe_batch(*a) == -1, hole


def test_python_layer_refuses_by_name():
    from xiangqi_alphazero_amd import hip
    table = torch.zeros(88452, dtype=torch.int16)
    flag = torch.zeros(1, dtype=torch.int32)
    boards, side = torch.zeros((2, 90), dtype=torch.int8), torch.ones(2, dtype=torch.int8)
    for call, word in ((lambda: hip.tb_init("Ra", table[:-1]), "table"), (lambda: hip.tb_init("Ra", table.to(torch.int32)), "table"),
                       (lambda: hip.tb_init("Rz", table), "signature"), (lambda: hip.tb_init("Ra", None), "table"),
                       (lambda: hip.tb_pass("Ra", table, 0, flag), "k"), (lambda: hip.tb_pass("Ra", table, 32001, flag), "k"),
                       (lambda: hip.tb_pass("Ra", table, True, flag), "k"),
                       (lambda: hip.tb_pass("Ra", table, 1, flag.to(torch.int64)), "changed"),
                       (lambda: hip.tb_pass("Ra", table, 1, torch.zeros(2, dtype=torch.int32)), "changed"),
                       (lambda: hip.tb_generate("Ra", "cuda", max_passes=0), "max_passes"),
                       (lambda: hip.tb_generate("RNCrn", "cuda"), "RNCrn"),
                       (lambda: hip.tb_probe_batch("Ra", table[:5], boards, side), "table"),
                       (lambda: hip.tb_probe_batch("Ra", table, boards[:, :80], side), "boards"),
                       (lambda: hip.tb_probe_batch("Ra", table, boards, side.to(torch.int32)), "boards"),
                       (lambda: hip.tb_probe_batch("Ra", table, boards, side, move_values=2), "move_values")):
        with pytest.raises(hip.XqError, match=word):
            call()
    # an empty batch is a no-op, with every output present
    out = hip.tb_probe_batch("Ra", table, boards[:0], side[:0])
    assert set(out) == {"value", "moves", "counts", "move_value", "best_action", "status"}
    assert all(len(v) == 0 for v in out.values()) and out["move_value"].shape == (0, hip.MAXM)
    assert "move_value" not in hip.tb_probe_batch("Ra", table, boards[:0], side[:0], move_values=False)


def test_layout_round_trip_over_a_whole_table():
    from xiangqi_alphazero_amd import endgame, hip
    n = endgame.entries("Ra")
    idx = np.arange(n)
    boards, sides, collide = endgame.index_to_board("Ra", idx, return_collisions=True)
    assert boards.shape == (n, 90) and boards.dtype == np.int8 and set(np.unique(sides).tolist()) == {1, -1}
    back = endgame.board_to_index("Ra", boards, sides)
    assert (back[~collide] == idx[~collide]).all()
    # a collision shows the later man only: the board reads as the entry with the earlier man captured, or lacks a king
    assert collide.sum() > 0 and (back[collide] != idx[collide]).all()
    dig = endgame.index_to_digits("Ra", idx)
    assert (dig.max(axis=0) == [1, 8, 8, 90, 5]).all() and (dig[:, 0] == (idx >= n // 2)).all()
    men = (boards != 0).sum(axis=1)
    assert (men[~collide] == 2 + (dig[~collide, 3] < 90) + (dig[~collide, 4] < 5)).all()
    # not covered: a piece the signature lacks, a piece outside its list, a missing king
    b = boards[[1000, 1000, 1000, 1000]].copy()
    assert back[1000] == 1000
    free = int(np.nonzero(b[0] == 0)[0][-1])
    b[1, free] = 7
    b[2, b[2] == 1] = 0
    b[3, b[3] == -2] = 0
    b[3, 44] = -2
    assert endgame.board_to_index("Ra", b, sides[[1000] * 4]).tolist()[:3] == [1000, -1, -1]
    assert endgame.board_to_index("Ra", b, sides[[1000] * 4])[3] == (-1 if (boards[1000] == -2).any() else back[1000])
    with pytest.raises(hip.XqError, match="index"):
        endgame.index_to_board("Ra", [n])
    # two equal pieces: the board names the smaller square first
    b2, s2, c2 = endgame.index_to_board("aa", np.arange(endgame.entries("aa")), return_collisions=True)
    two = endgame.board_to_index("aa", b2, s2)
    d = endgame.index_to_digits("aa", np.arange(endgame.entries("aa")))
    ordered = ~c2 & ((d[:, 3] < d[:, 4]) | ((d[:, 3] == 5) & (d[:, 4] == 5)))
    swapped = ~c2 & (d[:, 3] > d[:, 4]) & (d[:, 4] < 5)
    assert swapped.any() and (two[swapped] != np.nonzero(swapped)[0]).all() and (two[swapped] >= 0).all()
    assert (two[ordered] == np.nonzero(ordered)[0]).all()


def _host_table(sig):
    from xiangqi_alphazero_amd import endgame
    n = endgame.entries(sig)
    t = (np.arange(n) % 7 - 3).astype(np.int16)
    t[::11] = endgame.INVALID
    return t


def test_save_and_load(tmp_path):
    from xiangqi_alphazero_amd import endgame, hip
    t = _host_table("Ra")
    tb = endgame.Tablebase("Ra", t, passes=11, device="cpu")
    path = str(tmp_path / "ra.npz")
    tb.save(path)
    back = endgame.Tablebase.load(path, device="cpu")
    assert back.signature == "Ra" and back.codes == (5, -2) and back.passes == 11 and back.table.dtype == np.int16
    assert back.table.tobytes() == t.tobytes()
    with np.load(path) as z:
        assert set(z.files) == {"signature", "layout_version", "passes", "table"} and int(z["layout_version"]) == endgame.LAYOUT_VERSION
    short = str(tmp_path / "short.npz")
    np.savez(short, signature=np.array([5, -2], dtype=np.int8), layout_version=np.int64(endgame.LAYOUT_VERSION), passes=np.int64(1),
             table=t[:-1])
    with pytest.raises(hip.XqError, match="entries"):
        endgame.Tablebase.load(short, device="cpu")
    other = str(tmp_path / "other.npz")
    np.savez(other, signature=np.array([5, -2], dtype=np.int8), layout_version=np.int64(99), passes=np.int64(1), table=t)
    with pytest.raises(hip.XqError, match="layout version"):
        endgame.Tablebase.load(other, device="cpu")
    with pytest.raises(hip.XqError, match="entries"):
        endgame.Tablebase("Ra", t[:100], device="cpu")
    with pytest.raises(hip.XqError, match="entries"):
        endgame.Tablebase("Ra", t.astype(np.int32), device="cpu")
    # stats and positions read the host table alone
    s = tb.stats()
    half = len(t) // 2
    assert s["entries"] == len(t) and s["passes"] == 11 and s["longest_win"] == 3
    for name, part in (("red", t[:half]), ("black", t[half:])):
        assert s[name] == {"invalid": int((part == endgame.INVALID).sum()), "win": int((part > 0).sum()),
                           "loss": int(((part < 0) & (part != endgame.INVALID)).sum()), "draw": int((part == 0).sum())}
    boards, sides, idx = tb.positions("win", 50, seed=4, side=-1, min_plies=2)
    assert (t[idx] >= 2).all() and (idx >= half).all() and (sides == -1).all() and len(set(idx.tolist())) == 50
    assert (tb.positions("win", 50, seed=4, side=-1, min_plies=2)[2] == idx).all()
    assert (tb.positions("win", 50, seed=5, side=-1, min_plies=2)[2] != idx).any()
    assert (t[tb.positions("loss", 20, seed=1, min_plies=2)[2]] <= -3).all() and (t[tb.positions("draw", 20)[2]] == 0).all()
    assert (endgame.index_to_board("Ra", idx)[0] == boards).all()
    for call, word in ((lambda: tb.positions("won", 3), "kind"), (lambda: tb.positions("win", 3, side=0), "side"),
                       (lambda: tb.positions("win", -1), "n"), (lambda: tb.positions("win", 10 ** 6), "entries")):
        with pytest.raises(hip.XqError, match=word):
            call()


def test_rescore_and_hold_rate_refuse_by_name():
    from xiangqi_alphazero_amd import endgame, hip
    from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE
    tb = endgame.Tablebase("Ra", _host_table("Ra"), device="cpu")
    samples = np.zeros(3, dtype=SAMPLE_DTYPE)
    with pytest.raises(hip.XqError, match="tb"):
        endgame.rescore_samples(samples, None)
    with pytest.raises(hip.XqError, match="SAMPLE_DTYPE"):
        endgame.rescore_samples(np.zeros((3, 640), dtype=np.uint8), tb)
    with pytest.raises(hip.XqError, match="SAMPLE_DTYPE"):
        endgame.rescore_samples([1, 2], tb)
    # nothing the layout covers: no probe, no change, a copy
    out, covered, changed = endgame.rescore_samples(samples, tb)
    assert (covered, changed) == (0, 0) and out is not samples and out.tobytes() == samples.tobytes()
    assert endgame.rescore_samples(samples[:0], tb)[1:] == (0, 0)
    with pytest.raises(hip.XqError, match="tb"):
        endgame.hold_rate(None, "Ra", samples["board"], samples["side"], 8)
    with pytest.raises(hip.XqError, match="num_simulations"):
        endgame.hold_rate(None, tb, samples["board"], samples["side"], 0)
    with pytest.raises(hip.XqError, match="chunk"):
        endgame.hold_rate(None, tb, samples["board"], samples["side"], 8, chunk=0)
    with pytest.raises(hip.XqError, match="chosen"):
        endgame.score({"value": np.zeros(2, dtype=np.int16)}, [1, 2, 3])


def test_loop_reads_and_refuses_the_endgame_keys(tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=4, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=6, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path))

    def loop(**extra):
        return train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, **extra), device="cpu", seed=1)

    assert loop().endgame is None and loop(endgame_signature=None).endgame is None
    assert loop(endgame_positions=3, endgame_rescore=True).endgame is None
    assert loop(endgame_signature="R").endgame == dict(signature="R", positions=256, kind="win", simulations=6, interval=1,
                                                      rescore=False)
    assert loop(endgame_signature="Eh", endgame_positions=16, endgame_kind="draw", endgame_simulations=4, endgame_interval=3,
                endgame_rescore=True).endgame == dict(signature="Bn", positions=16, kind="draw", simulations=4, interval=3,
                                                      rescore=True)
    for extra, key in ((dict(endgame_signature="Rx"), "endgame_signature"), (dict(endgame_signature="RNCrn"), "endgame_signature"),
                       (dict(endgame_signature="RRRRRR"), "endgame_signature"), (dict(endgame_signature=5), "endgame_signature"),
                       (dict(endgame_signature="R", endgame_positions=0), "endgame_positions"),
                       (dict(endgame_positions=2.5), "endgame_positions"),            # checked even while the yardstick is off
                       (dict(endgame_signature="R", endgame_kind="loss"), "endgame_kind"),
                       (dict(endgame_signature="R", endgame_kind=1), "endgame_kind"),
                       (dict(endgame_signature="R", endgame_simulations=0), "endgame_simulations"),
                       (dict(endgame_signature="R", endgame_interval=0), "endgame_interval"),
                       (dict(endgame_signature="R", endgame_interval=True), "endgame_interval"),
                       (dict(endgame_signature="R", endgame_rescore=1), "endgame_rescore")):
        with pytest.raises(hip.XqError, match=key):
            loop(**extra)
