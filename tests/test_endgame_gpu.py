"""The endgame tablebases on the GPU (csrc/xq_tablebase.hip, endgame.py, train_loop's endgame keys): generated tables equal the
CPU model (tests/endgame_model.py) word for word, the probe equals it output for output, one signature beyond the model is held
to its own symmetries on the device, the shipped mate kernel agrees, and hold_rate, rescore_samples and the loop do what they
say."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import endgame_model as EM
import golden_io
from test_baseline_loop_gpu import PLAIN, _config

pytestmark = pytest.mark.gpu

# the smallest signatures that exercise, each for one reason: facing kings; a pawn's two square classes; black's rotated lists;
# captures in both directions; a drawn and a won cannon ending; two equal pieces on one square; a knight's leg blocked by an
# elephant and the longest distance, 31
SIGNATURES = ["", "P", "p", "R", "C", "N", "aa", "Ra", "CA", "Pa", "Nb"]
WPW = 4
ENTRY = {"signature", "kind", "positions", "held", "optimal", "hold_rate", "by_kind", "simulations", "seconds"}


@lru_cache(maxsize=None)
def _table(signature):
    from xiangqi_alphazero_amd import hip
    table, passes = hip.tb_generate(signature, "cuda")
    return table, passes


@pytest.mark.parametrize("signature", SIGNATURES)
def test_generate_equals_the_model(signature):
    from xiangqi_alphazero_amd import hip
    m = EM.model(signature)
    table, passes = _table(signature)
    got = table.cpu().numpy()
    assert got.dtype == np.int16 and got.shape == m.table.shape
    differ = np.nonzero(got != m.table)[0]
    assert len(differ) == 0, (signature, len(differ), differ[:5], got[differ[:5]], m.table[differ[:5]])
    assert passes == m.passes
    again, passes2 = hip.tb_generate(signature, "cuda")
    assert passes2 == passes and again.cpu().numpy().tobytes() == got.tobytes()
    # a capped run stops at the cap and holds the distances up to it
    if m.passes > 3:
        part, k = hip.tb_generate(signature, "cuda", max_passes=2)
        want = np.where(np.isin(m.table, (EM.INVALID, -1, 1, -3)), m.table, 0)
        assert k == 2 and (part.cpu().numpy() == want).all()


def test_a_pass_after_convergence_decides_nothing():
    from xiangqi_alphazero_amd import hip
    table, passes = _table("Ra")
    work = table.clone()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in (passes, passes + 1, passes + 2):
        hip.tb_pass("Ra", work, k, flag)
    assert int(flag.item()) == 0 and torch.equal(work, table)
    # and the flag is set by a pass that decides: pass 1 over pass 0's table
    fresh = torch.empty_like(table)
    hip.tb_init("Ra", fresh)
    assert set(np.unique(fresh.cpu().numpy()).tolist()) == {EM.INVALID, -1, 0}
    hip.tb_pass("Ra", fresh, 1, flag)
    assert int(flag.item()) == 1 and int((fresh == 1).sum()) > 0


def _probe(signature, rows):
    from xiangqi_alphazero_amd import hip
    m = EM.model(signature)
    table, _ = _table(signature)
    boards = torch.from_numpy(m.boards[rows]).cuda()
    sides = torch.from_numpy(m.sides[rows]).cuda()
    out = hip.tb_probe_batch(signature, table, boards, sides)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["moves"], got["best_action"], got["counts"] = got["moves"].view(np.uint16), got["best_action"].view(np.uint16), got["counts"].view(np.uint16)
    return got


@pytest.mark.parametrize("signature", ["Ra", "Nb"])
def test_probe_equals_the_model_over_the_whole_table(signature):
    from xiangqi_alphazero_amd import endgame
    m = EM.model(signature)
    collide = endgame.index_to_board(signature, np.arange(m.entries), return_collisions=True)[2]
    every = np.nonzero(~collide)[0]             # a collision's board shows another entry
    assert (m.table[collide] == EM.INVALID).all()
    for rows in (every[7:8], every[100:100 + WPW - 1], every[-(WPW + 1):], every):
        want = m.probe(rows)
        got = _probe(signature, rows)
        assert set(got) == set(want)
        for key in ("status", "value", "counts", "moves", "move_value", "best_action"):
            bad = np.nonzero((got[key].astype(np.int64) != want[key].astype(np.int64)).reshape(len(rows), -1).any(axis=1))[0]
            assert len(bad) == 0, (signature, key, len(bad), rows[bad[:3]], got[key][bad[:3]], want[key][bad[:3]])
        t = m.table[rows]
        assert ((got["status"] == 4) == (t == EM.INVALID)).all() and (got["value"][t != EM.INVALID] == t[t != EM.INVALID]).all()
        past = np.arange(EM.MAXM)[None, :] >= got["counts"].astype(np.int64)[:, None]
        assert (got["moves"][past] == 0).all() and (got["move_value"][past] == 0).all()
        assert (got["best_action"][got["counts"] == 0] == EM.NO_MOVE).all()
    # without move values the other outputs are the same
    from xiangqi_alphazero_amd import hip
    rows = every[::97]
    table, _ = _table(signature)
    lean = hip.tb_probe_batch(signature, table, torch.from_numpy(m.boards[rows]).cuda(), torch.from_numpy(m.sides[rows]).cuda(),
                              move_values=False)
    full = _probe(signature, rows)
    assert "move_value" not in lean and (lean["value"].cpu().numpy() == full["value"]).all()
    assert (lean["best_action"].cpu().numpy().view(np.uint16) == full["best_action"]).all()


def test_probe_status():
    from xiangqi_alphazero_amd import endgame, hip
    table, _ = _table("Ra")

    def probe(boards, sides):
        out = hip.tb_probe_batch("Ra", table, torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8)).cuda(),
                                 torch.from_numpy(np.ascontiguousarray(sides, dtype=np.int8)).cuda())
        return {k: v.cpu().numpy() for k, v in out.items()}

    # corpus positions hold pieces the signature lacks
    d = golden_io.corpus()
    r = probe(d["board"][:64], d["side"][:64])
    assert (r["status"] == 1).all() and (r["value"] == 0).all() and (r["counts"] == 0).all()
    assert (r["best_action"].view(np.uint16) == EM.NO_MOVE).all() and (r["moves"] == 0).all() and (r["move_value"] == 0).all()
    # K+R v K: the advisor counts as captured, and the value is the "R" table's
    mr = EM.model("R")
    rows = np.nonzero(mr.table != EM.INVALID)[0][::37]
    r = probe(mr.boards[rows], mr.sides[rows])
    assert (r["status"] == 0).all() and (r["value"] == mr.table[rows]).all()
    assert (r["value"] == _table("R")[0].cpu().numpy()[rows]).all()
    want = endgame.board_to_index("Ra", mr.boards[rows], mr.sides[rows])
    assert (EM.model("Ra").table[want] == mr.table[rows]).all()
    # a board without red's king; an advisor outside its list; a second rook
    ma = EM.model("Ra")
    e = int(np.nonzero((ma.table > 0) & ((ma.boards == -2).sum(axis=1) == 1) & ((ma.boards == 5).sum(axis=1) == 1))[0][500])
    b = ma.boards[[e, e, e, e]].copy()
    b[1, b[1] == 1] = 0
    b[2, b[2] == -2] = 0
    b[2, 49] = -2
    b[3, int(np.nonzero(b[3] == 0)[0][40])] = 5
    r = probe(b, ma.sides[[e] * 4])
    assert r["status"].tolist() == [0, 2, 1, 1] and r["value"].tolist() == [int(ma.table[e]), 0, 0, 0]
    assert r["counts"].tolist()[1:] == [0, 0, 0] and (r["best_action"].view(np.uint16)[1:] == EM.NO_MOVE).all()


# ---- one signature beyond the model, held to its own symmetries on the device ----------------------------------------------
def _digits(signature, idx):
    from xiangqi_alphazero_amd import endgame
    out, x = [], idx.clone()
    for r in reversed(endgame.radices(signature)):
        out.append(x % r)
        x = x // r
    return out[::-1]


def _index(signature, digits):
    from xiangqi_alphazero_amd import endgame
    x = torch.zeros_like(digits[0])
    for r, d in zip(endgame.radices(signature), digits):
        x = x * r + d
    return x


def _decode(signature, idx):
    """index_to_board on the device -> boards int8[n, 90], sides int8[n], collide bool[n]."""
    from xiangqi_alphazero_amd import endgame
    dig = _digits(signature, idx)
    n = len(idx)
    rows = torch.arange(n, device=idx.device)
    boards = torch.zeros((n, 90), dtype=torch.int8, device=idx.device)
    boards[rows, torch.from_numpy(endgame.RED_KING_SQUARES).to(idx.device)[dig[1]]] = 1
    boards[rows, torch.from_numpy(endgame.BLACK_KING_SQUARES).to(idx.device)[dig[2]]] = -1
    collide = torch.zeros(n, dtype=torch.bool, device=idx.device)
    for p, code in enumerate(endgame.parse_signature(signature)):
        sqs = torch.from_numpy(endgame.piece_squares(code)).to(idx.device)
        d = dig[3 + p]
        on = d < len(sqs)
        sq = sqs[torch.clamp(d, max=len(sqs) - 1)]
        collide |= on & (boards[rows, sq] != 0)
        boards[rows[on], sq[on]] = code
    sides = torch.where(dig[0] == 0, 1, -1).to(torch.int8)
    return boards, sides, collide


def test_three_pieces_on_the_device_alone():
    from xiangqi_alphazero_amd import endgame, hip
    from xiangqi_alphazero_amd.sample_format import MIR_SQ
    sig = "RNa"
    n = hip.tb_entries(sig)
    assert n == 8049132
    table, passes = _table(sig)
    t64 = table.to(torch.int64)
    assert passes >= 11 and int((table > 0).sum()) > 0 and int((table == 0).sum()) > 0
    # Bellman consistency over the whole table, through the probe
    big = 1 << 40
    for base in range(0, n, 1 << 20):
        idx = torch.arange(base, min(base + (1 << 20), n), device="cuda")
        boards, sides, collide = _decode(sig, idx)
        out = hip.tb_probe_batch(sig, table, boards, sides)
        t = t64[idx]
        keep = ~collide
        assert bool((t[collide] == EM.INVALID).all())
        st, val = out["status"].to(torch.int64), out["value"].to(torch.int64)
        assert bool(((st == 4) == (t == EM.INVALID))[keep].all()) and bool(((st == 0) | (st == 4))[keep].all())
        ok = keep & (st == 0)
        assert bool((val[ok] == t[ok]).all())
        cnt = out["counts"].to(torch.int64)
        mv = out["move_value"].to(torch.int64)
        live = torch.arange(hip.MAXM, device="cuda")[None, :] < cnt[:, None]
        assert bool((mv[~live] == 0).all())
        wins = torch.where(live & (mv > 0), mv, big).amin(dim=1)
        draw = (live & (mv == 0)).any(dim=1)
        loss = torch.where(live, mv, big).amin(dim=1)
        best = torch.where(wins < big, wins, torch.where(draw, 0, loss))
        has = ok & (cnt > 0)
        assert bool((best[has] == val[has]).all()) and bool((val[ok & (cnt == 0)] == -1).all())
        first = (live & (mv == val[:, None])).to(torch.int8).argmax(dim=1)
        act = out["moves"].to(torch.int64)[torch.arange(len(idx), device="cuda"), first]
        assert bool((act[has] == out["best_action"].to(torch.int64)[has]).all())
    # left-right mirror of every digit, and the rotation into "rnA": both are permutations of the index
    idx = torch.arange(n, device="cuda")
    dig = _digits(sig, idx)
    codes = endgame.parse_signature(sig)
    mk = torch.tensor([2, 1, 0, 5, 4, 3, 8, 7, 6], device="cuda")
    mir = [dig[0], mk[dig[1]], mk[dig[2]]]
    rot = [1 - dig[0], 8 - dig[2], 8 - dig[1]]
    for p, code in enumerate(codes):
        sqs = endgame.piece_squares(code)
        of = {int(s): d for d, s in enumerate(sqs)}
        lut = torch.tensor([of[int(MIR_SQ[s])] for s in sqs] + [len(sqs)], device="cuda")
        mir.append(lut[dig[3 + p]])
        rot.append(torch.where(dig[3 + p] == len(sqs), dig[3 + p], len(sqs) - 1 - dig[3 + p]))
    assert torch.equal(table[_index(sig, mir)], table)
    other, other_passes = _table("rnA")
    assert other_passes == passes and torch.equal(other[_index("rnA", rot)], table)
    del other
    # the knight captured: the "Ra" sub-ending is the "Ra" table
    sub = dig[4] == 90
    ra, _ = _table("Ra")
    assert int(sub.sum()) == len(ra) and torch.equal(table[sub], ra[_index("Ra", [dig[0][sub], dig[1][sub], dig[2][sub], dig[3][sub], dig[5][sub]])])


def test_the_mate_kernel_agrees():
    from xiangqi_alphazero_amd import hip
    m = EM.model("N")
    table, _ = _table("N")
    rows = np.sort(np.random.default_rng(7).choice(np.nonzero(m.table != EM.INVALID)[0], size=256, replace=False))
    out = hip.mate_search_batch(torch.from_numpy(m.boards[rows]).cuda(), torch.from_numpy(m.sides[rows]).cuda(), 5,
                                checks_only=False, node_limit=2 ** 31)
    v = table.cpu().numpy()[rows].astype(np.int64)
    want = np.where((v > 0) & (v <= 9), (v + 1) // 2, 0)
    assert (out["status"].cpu().numpy() == 0).all()
    assert (out["best_mate_in"].cpu().numpy() == want).all() and set(want.tolist()) >= {0, 1, 2, 3}


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _rook():
    from xiangqi_alphazero_amd import endgame
    return endgame.Tablebase.generate("R", "cuda")


def test_tablebase_class_on_the_device(tmp_path):
    from xiangqi_alphazero_amd import endgame
    tb = _rook()
    m = EM.model("R")
    assert tb.table.tobytes() == m.table.tobytes() and tb.passes == m.passes and tb.signature == "R"
    s = tb.stats()
    assert (tuple(s["red"].values()), tuple(s["black"].values()), s["longest_win"], s["passes"]) == \
        (m.stats()["red"], m.stats()["black"], 3, 5)
    tb.save(str(tmp_path / "r.npz"))
    back = endgame.Tablebase.load(str(tmp_path / "r.npz"), "cuda")
    boards, sides, idx = back.positions("win", 40, seed=2)
    got, want = back.probe(boards, sides), m.probe(idx)
    for key in want:
        assert (got[key].astype(np.int64) == want[key].astype(np.int64)).all(), key


def test_hold_rate():
    from xiangqi_alphazero_amd import endgame, hip
    from xiangqi_alphazero_amd.model import XiangqiNet
    tb = _rook()
    boards, sides, idx = tb.positions("win", 32, seed=11)
    torch.manual_seed(5)
    net = XiangqiNet(64, 1).cuda().eval()          # the narrowest tower the product evaluator takes
    res = endgame.hold_rate(net, tb, boards, sides, 8, seed=7)
    assert set(res) == {"positions", "held", "optimal", "hold_rate", "by_kind", "simulations", "seconds", "chosen"}
    assert res["positions"] == 32 and 0 <= res["optimal"] <= res["held"] <= 32 and res["hold_rate"] == res["held"] / 32
    assert res["by_kind"] == {"win": [32, res["held"]]} and res["simulations"] == 8 and res["seconds"] > 0
    probe = tb.probe(boards, sides)
    assert {k: v for k, v in endgame.score(probe, res["chosen"]).items()} == {k: res[k] for k in ("positions", "held", "optimal", "hold_rate", "by_kind")}
    # every chosen move is a root move, and chunks smaller than the set give the same moves
    for j, a in enumerate(res["chosen"]):
        assert a in probe["moves"][j, :probe["counts"][j]]
    assert list(endgame.hold_rate(net, tb, boards, sides, 8, seed=7, chunk=5)["chosen"]) == list(res["chosen"])
    # the probe's own best actions hold and are optimal
    best = endgame.score(probe, probe["best_action"])
    assert best["held"] == best["optimal"] == 32 and best["hold_rate"] == 1.0
    # a move that gives the win away holds nothing; a drawn position is held by a drawing move
    worst = [int(probe["moves"][j, int(np.argmin(np.where(np.arange(hip.MAXM) < probe["counts"][j], probe["move_value"][j], 1 << 14)))])
             for j in range(32)]
    bad = endgame.score(probe, worst)
    assert bad["held"] == int(sum(probe["move_value"][j, list(probe["moves"][j]).index(worst[j])] > 0 for j in range(32)))
    db, ds, _ = tb.positions("draw", 8, seed=1)
    dp = tb.probe(db, ds)
    assert endgame.score(dp, dp["best_action"])["by_kind"] == {"draw": [8, 8]}
    # lost positions are refused
    lb, ls, _ = tb.positions("loss", 4, seed=1, min_plies=2)
    with pytest.raises(hip.XqError, match="lost"):
        endgame.hold_rate(net, tb, lb, ls, 8)
    d = golden_io.corpus()
    with pytest.raises(hip.XqError, match="not valid entries"):
        endgame.hold_rate(net, tb, d["board"][:2], d["side"][:2], 8)


def _samples():
    from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE
    tb = _rook()
    rng = np.random.default_rng(3)
    parts = [tb.positions(kind, 20, seed=5) for kind in ("win", "loss", "draw")]
    d = golden_io.corpus()
    boards = np.concatenate([p[0] for p in parts] + [d["board"][200:230]])
    sides = np.concatenate([p[1] for p in parts] + [d["side"][200:230]])
    s = np.zeros(len(boards), dtype=SAMPLE_DTYPE)
    s["board"], s["side"] = boards, sides
    s["z"] = rng.integers(-1, 2, size=len(s))
    s["n_moves"], s["ply"], s["slot"], s["game_seq"] = 3, rng.integers(0, 200, size=len(s)), np.arange(len(s)), 9
    s["actions"], s["visits"], s["pad"] = rng.integers(0, 8100, size=(len(s), 128)), rng.integers(0, 50, size=(len(s), 128)), 7
    exact = np.concatenate([np.sign(tb.table[p[2]].astype(np.int64)) for p in parts])
    return s, exact


def test_rescore_samples():
    from xiangqi_alphazero_amd import endgame
    from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE
    tb = _rook()
    s, exact = _samples()
    assert exact.tolist() == [1] * 20 + [-1] * 20 + [0] * 20
    before = s.tobytes()
    out, covered, changed = endgame.rescore_samples(s, tb)
    assert s.tobytes() == before and out.dtype == SAMPLE_DTYPE and out.shape == s.shape
    assert covered == 60 and changed == int((s["z"][:60] != exact).sum()) and 0 < changed < 60
    assert (out["z"][:60] == exact).all() and (out["z"][60:] == s["z"][60:]).all()
    a, b = np.frombuffer(before, dtype=np.uint8).reshape(-1, 640), out.view(np.uint8).reshape(-1, 640)
    rows, cols = np.nonzero(a != b)
    assert len(rows) == changed and set(cols.tolist()) == {SAMPLE_DTYPE.fields["z"][1]} and rows.max() < 60
    again, covered2, changed2 = endgame.rescore_samples(out, tb)
    assert (covered2, changed2) == (60, 0) and again.tobytes() == out.tobytes()
    # an invalid entry's board is covered by the layout and refused by the probe: it keeps its z
    m = EM.model("R")
    e = int(np.nonzero((m.table == EM.INVALID) & ((m.boards != 0).sum(axis=1) == 3))[0][10])
    one = s[:1].copy()
    one["board"][0], one["side"][0], one["z"][0] = m.boards[e], m.sides[e], 1
    assert endgame.rescore_samples(one, tb)[1:] == (0, 0)


def test_loop_logs_the_hold_rate_and_rescoring(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    cfg = _config(tmp_path / "ck", endgame_signature="R", endgame_positions=16, endgame_simulations=4, endgame_rescore=True)
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    assert loop.endgame["rescore"] and loop._endgame_tb is None
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    assert [s["iteration"] for s in stats] == [1, 2] and len(saved) == 2
    for entry, on_disk in zip(stats, saved):
        assert set(entry) == PLAIN | {"endgame"} == set(on_disk)
        e = on_disk["endgame"]
        assert set(e) == ENTRY and e["signature"] == "R" and e["kind"] == "win"
        assert e["positions"] == 16 and e["simulations"] == 4 and 0 <= e["optimal"] <= e["held"] <= 16
        assert e["hold_rate"] == e["held"] / 16 and e["by_kind"] == {"win": [16, e["held"]]} and e["seconds"] > 0
        sp = on_disk["self_play"]
        assert 0 <= sp["endgame_changed"] <= sp["endgame_covered"] <= sp["new_samples"] // 2
    assert loop._endgame_tb.table.tobytes() == EM.model("R").table.tobytes()


def test_loop_without_rescoring_and_without_the_keys(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    cfg = _config(tmp_path / "a", endgame_signature="R", endgame_positions=16, endgame_simulations=4, endgame_interval=2)
    stats = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3).train()
    assert "endgame" not in stats[0] and set(stats[1]["endgame"]) == ENTRY
    assert not any(k.startswith("endgame") for s in stats for k in s["self_play"])
    plain = _config(tmp_path / "b")
    plain.num_iterations = 1
    loop = train_loop.AlphaZeroLoop(plain, "cuda", seed=3)
    assert loop.endgame is None
    stats = loop.train()
    saved = json.load(open(tmp_path / "b" / "training_stats.json"))
    assert len(stats) == len(saved) == 1 and set(stats[0]) == PLAIN == set(saved[0])
    assert not any(k.startswith("endgame") for k in stats[0]["self_play"]) and loop._endgame_tb is None
