"""Game records as training samples on the GPU (xq_records_sample_counts, xq_records_to_samples, and the path above them).

1. the kernel against tests/supervised_model.py, byte for byte: all 640 bytes of every row, the status and the counts, over an
   empty record, a one-ply record, a 504-ply legal shuffle, a game through a position with 72 legal moves (two ballot rounds), a
   record with an illegal ply in the middle and a malformed record of each kind; n = 1, 4, 5 and 9 (ragged against four waves
   per workgroup), every `movers` value, with and without one mover set per record, both flags; and offsets that do not fit;
2. the engine as witness, no model in between: the records of a self-play engine, converted, carry the engine's own samples'
   board, side, z, ply, n_moves and actions, with the one visit at the recorded move;
3. it trains: 30 Adam steps of a 16x1 network on 32 ladder games lower the policy cross-entropy and raise the top-1 agreement
   that `selfplay.score_samples` measures on the same rows;
4. the loop: a fresh two-iteration AlphaZeroLoop with `pretrain_records` logs "pretrain" in its first entry only.

The largest legal-move count of tests/golden/corpus.npz is 63 (position 517: game 3, ply 133), so no corpus position takes two
ballot rounds on its own; the game of case 1 is that corpus game up to position 517 and two plies more (4179, 5196), found by a
search over its successors, after which the side to move has 72 legal moves.  The test checks both counts against the oracle.
"""
import json
import types

import numpy as np
import pytest

import golden_io as G
import supervised_model as M
from oracle import xq_oracle as O
from test_tree_reuse_gpu import _stub_step

pytestmark = pytest.mark.gpu

_cache = {}


def _record(moves, winner, opening=0, slot=0, game_seq=0):
    from xiangqi_alphazero_amd import hip
    r = np.zeros((), dtype=hip.GAME_RECORD_DTYPE)
    r["n_moves"], r["winner"], r["opening_plies"], r["slot"], r["game_seq"] = len(moves), winner, opening, slot, game_seq
    r["moves"][:len(moves)] = moves
    return r


def _corpus_game():
    """Corpus game 3 up to its position of 63 legal moves, two plies to a position of 72, and one move played there."""
    d = G.corpus()
    i = 517
    assert int(d["ply"][i]) == 133 and len(O.legal_actions(d["board"][i], int(d["side"][i]))) == 63
    moves = [int(a) for a in d["taken"][i - 133:i]] + [4179, 5196]
    g = O.Game()
    for a in moves:
        assert a in g.legal_actions()
        g.make_action(a)
    wide = g.legal_actions()
    assert len(wide) == 72                                     # more than one ballot round of 64 lanes
    return moves + [int(wide[70])]                             # a move the second round finds


def _records():
    """The nine records of case 1, the interesting ones first: n = 1, 4, 5, 9 take a prefix."""
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd.sample_format import iccs_to_action
    if "records" not in _cache:
        act = lambda text: [iccs_to_action(m) for m in text.split()]
        shuffle = act("b0c2 b9c7 h2h1 h7h8 c2b0 c7b9 h1h2 h8h7") * 63          # horses and cannons, back and forth: 504 plies
        short = act("b2e2 h9g7 h0g2 i9h9 e2e6 g7e6")
        illegal = list(short)
        illegal[3] = illegal[1]                                                # the horse has left that square
        long_mal, open_mal, win_mal = _record(short, 1), _record(short, 1, opening=7), _record(short, 2)
        long_mal["n_moves"] = 505
        recs = [_record(_corpus_game(), 1, opening=4, slot=7, game_seq=2), _record(illegal, -1, opening=1, slot=1, game_seq=5),
                _record(shuffle, 0, opening=3, slot=2, game_seq=1), long_mal, _record(short[:1], 1, slot=4), _record([], 0, slot=5),
                open_mal, win_mal, _record(short, -1, opening=2, slot=8, game_seq=0xFFFFFFFF)]
        out = np.array(recs, dtype=hip.GAME_RECORD_DTYPE)
        out.setflags(write=False)
        _cache["records"] = out
    return _cache["records"]


def _model_rows(i, movers, skip_opening, skip_draws):
    """One record's rows and status from the model, computed once per selection and shared."""
    key = ("rows", i, movers, skip_opening, skip_draws)
    if key not in _cache:
        _cache[key] = M.record_rows(_records()[i], movers, skip_opening, skip_draws)
    return _cache[key]


def _expected(n, movers, per, skip_opening, skip_draws):
    rows, status = [], []
    for i in range(n):
        m = movers if per is None else int(per[i])
        r, st = _model_rows(i, m, skip_opening, skip_draws) if 0 <= m <= 3 else (np.zeros(0, dtype=M.SAMPLE_DTYPE), -1)
        rows.append(r.view(np.uint8).reshape(len(r), 640))
        status.append(st)
    counts = [len(r) for r in rows]
    return np.concatenate(rows), np.array(status, dtype=np.int32), np.array(counts, dtype=np.int32)


# ---- 1. the kernel against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 9])
def test_rows_equal_the_model_byte_for_byte(n):
    from xiangqi_alphazero_amd import hip
    records = _records()[:n]
    assert M.record_rows(_records()[0], 0, False, False)[1] == 0 and M.record_rows(_records()[2], 0, False, False)[1] == 0
    assert M.record_rows(_records()[1], 0, False, False)[1] == 4
    for movers in range(4):
        for with_per in (False, True):
            per = None
            if with_per:                                    # another mover set per record; one entry outside [0, 3] from n = 4 on
                per = np.array([(movers + i) % 4 for i in range(n)], dtype=np.uint8)
                if n >= 4:
                    per[2] = 7
            for skip_opening in (False, True):
                for skip_draws in (False, True):
                    what = (n, movers, with_per, skip_opening, skip_draws)
                    rows, status, counts = _expected(n, movers, per, skip_opening, skip_draws)
                    assert counts.tolist() == M.sample_counts(records, movers, per, skip_opening, skip_draws).tolist(), what
                    out = hip.records_to_samples(records, movers, per, skip_opening, skip_draws)
                    offsets = out["offsets"].cpu().numpy()
                    assert offsets.dtype == np.int32 and np.diff(offsets).tolist() == counts.tolist() and offsets[0] == 0, what
                    assert out["status"].cpu().numpy().tolist() == status.tolist(), what
                    got = out["samples"].cpu().numpy()
                    assert got.shape == rows.shape, what
                    if got.tobytes() != rows.tobytes():
                        bad = np.nonzero((got != rows).any(axis=1))[0]
                        raise AssertionError(f"{what}: rows {bad[:8].tolist()} differ; first at bytes "
                                             f"{np.nonzero(got[bad[0]] != rows[bad[0]])[0][:8].tolist()}")
    if n == 9:      # the rows of the whole set under the default selection are not all alike: the comparison has teeth
        rows, status, counts = _expected(9, 0, None, True, False)
        assert counts.tolist() == [132, 5, 501, 0, 1, 0, 0, 0, 4] and status.tolist() == [0, 4, 0, -1, 0, 0, -1, -1, 0]
        s = rows.view(M.SAMPLE_DTYPE).reshape(-1)
        assert s["n_moves"][(s["slot"] == 7) & (s["ply"] == 135)].tolist() == [72]
        assert not rows[132 + 2:132 + 5].any() and rows[132:132 + 2].any(axis=1).all()      # the illegal ply's zero rows


def test_device_records_and_the_empty_batch():
    import torch
    from xiangqi_alphazero_amd import hip
    records = _records()[:5]
    dev = torch.from_numpy(records.view(np.uint8).reshape(5, 1024).copy()).cuda()
    a, b = hip.records_to_samples(dev, 1), hip.records_to_samples(records, 1)
    assert a["samples"].is_cuda and a["samples"].cpu().numpy().tobytes() == b["samples"].cpu().numpy().tobytes()
    assert a["status"].tolist() == b["status"].tolist() and a["offsets"].tolist() == b["offsets"].tolist()
    none = hip.records_to_samples(records[:0])
    assert tuple(none["samples"].shape) == (0, 640) and none["offsets"].tolist() == [0] and tuple(none["status"].shape) == (0,)
    nothing = hip.records_to_samples(records[3:4])         # one malformed record: no row at all
    assert tuple(nothing["samples"].shape) == (0, 640) and nothing["status"].tolist() == [-1]


def test_offsets_that_do_not_fit_leave_their_rows_alone():
    import ctypes as C
    import torch
    from xiangqi_alphazero_amd import hip
    records = _records()[:5]
    dev = torch.from_numpy(records.view(np.uint8).reshape(5, 1024).copy()).cuda()
    counts = M.sample_counts(records, 0, None, False, False)
    assert counts.tolist() == [136, 6, 504, 0, 1]
    right = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cases = [right.copy() for _ in range(3)]
    cases[0][2] -= 1                 # record 1 one row short, record 2 one row long: both refused, the others written
    cases[1][5] -= 1                 # the last record's range is empty and the total one short of its count
    cases[2][1:] += 3                # record 0 three rows long; every later record keeps its size, shifted
    opts = hip.SuperviseOpts(0, 0, 0, 0)
    for k, off in enumerate(cases):
        want = M.records_to_samples(records, 0, None, False, False, offsets=off, fill=0xA5)
        assert (want["status"] == -2).sum() == (2, 1, 1)[k] and want["status"][3] == -1
        rows = torch.full((int(off[5]), 640), 0xA5, dtype=torch.uint8, device="cuda")
        status = torch.full((5,), 9, dtype=torch.int32, device="cuda")
        off_dev = torch.from_numpy(off).cuda()
        hip.check(hip.lib().xq_records_to_samples(dev.data_ptr(), None, off_dev.data_ptr(), 5, C.byref(opts), rows.data_ptr(),
                                                  status.data_ptr(), hip.stream_ptr("cuda")), "xq_records_to_samples")
        assert status.cpu().numpy().tolist() == want["status"].tolist(), k
        assert rows.cpu().numpy().tobytes() == want["samples"].tobytes(), k
        untouched = int((want["samples"] == 0xA5).all(axis=1).sum())       # the refused records' ranges, as the call found them
        assert untouched == (5 + 505, 0, 139)[k], k


# ---- 2. the engine as witness -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resign", [False, True], ids=["no_resign", "resign"])
def test_converted_records_carry_the_engines_samples(resign):
    from xiangqi_alphazero_amd import engine, hip
    n_games = 16
    cfg = engine.make_config(8, 16, seed=13, games_target=n_games, max_game_length=30, random_opening_moves=2,
                             enable_resign=resign, resign_threshold=0.0, resign_check_steps=1)
    eng = engine.SelfPlayEngine(cfg, record_games=True)
    cache = {}
    for s in range(60000):
        _stub_step(eng, True, cache)
        if s % 32 == 31 and eng.stats()["games_finished"] >= n_games:
            break
    st = eng.stats()
    assert st["overflow"] == 0 and st["games_finished"] == n_games
    records = eng.drain_games()
    samples, results = eng.drain()
    assert len(records) == len(results) == n_games and len(samples) > 0
    out = hip.records_to_samples(records, movers=0, skip_opening=True)
    assert not out["status"].any().item()
    rows = out["samples"].cpu().numpy().reshape(-1).view(M.SAMPLE_DTYPE)
    offsets = out["offsets"].cpu().numpy()
    assert np.diff(offsets).tolist() == (records["n_moves"].astype(int) - records["opening_plies"].astype(int)).tolist()
    if resign:
        assert (records["reason"] == 3).any()
    at = {}
    for j, r in enumerate(rows):
        key = (int(r["slot"]), int(r["game_seq"]), int(r["ply"]))
        assert key not in at
        at[key] = j
    rec_of = {(int(r["slot"]), int(r["game_seq"])): r for r in records}
    for j, r in enumerate(rows):                            # the one visit sits at the recorded move
        rec = rec_of[(int(r["slot"]), int(r["game_seq"]))]
        assert r["visits"].sum() == 1 and int(r["actions"][int(np.argmax(r["visits"]))]) == int(rec["moves"][int(r["ply"])])
    for s in samples:                                       # every engine sample has exactly one partner, equal field by field
        r = rows[at[(int(s["slot"]), int(s["game_seq"]), int(s["ply"]))]]
        for field in ("board", "side", "z", "ply", "n_moves", "actions"):
            assert np.asarray(s[field]).tobytes() == np.asarray(r[field]).tobytes(), field
    assert len({(int(s["slot"]), int(s["game_seq"]), int(s["ply"])) for s in samples}) == len(samples) == len(rows)


# ---- 3. it trains -----------------------------------------------------------------------------------------------------------------
def _ladder_games():
    """32 ladder games, depth 2 against depth 2, 4 opening plies, seed 0: played once, shared, never modified."""
    from xiangqi_alphazero_amd import baseline
    if "ladder" not in _cache:
        rec = baseline.play_vs_baseline(2, 32, 2, 0, opening_plies=4, seed=0)["game_records"]
        rec.setflags(write=False)
        _cache["ladder"] = rec
    return _cache["ladder"]


class _LegalLogits:
    """`evaluate_legal` over a torch network: the hand-written evaluator takes 64 channels and up, this test's network has 16."""

    def __init__(self, net):
        self.net = net

    def evaluate_legal(self, x, moves, counts):
        import torch
        was = self.net.training
        self.net.eval()
        with torch.no_grad():
            logits, value = self.net(x)
        self.net.train(was)
        idx = moves.to(torch.int64) & 0xFFFF
        return torch.gather(logits, 1, idx.clamp(max=8099)).float().contiguous(), value.reshape(-1).float().contiguous()


def test_pretraining_lowers_the_policy_loss_and_raises_top1():
    import torch
    from xiangqi_alphazero_amd import hip, model, selfplay, training, weights
    records = _ladder_games()
    rows = hip.records_to_samples(records)["samples"]
    assert rows.shape[0] == int(M.sample_counts(records).sum()) > 500
    net = model.XiangqiNet(16, 1)
    net.load_state_dict(weights.make_state_dict(16, 1, seed=11))
    net = net.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4)
    ev = _LegalLogits(net)
    before = selfplay.score_summary(selfplay.score_samples(ev, rows, write_back=False, chunk=8192), rows)
    batch = -(-2 * int(rows.shape[0]) // 10)                  # ten batches an epoch, three epochs: 30 Adam steps
    cfg = types.SimpleNamespace(min_buffer_size=10 ** 9, num_epochs=7, batch_size=batch)
    info = {}
    epochs = training.pretrain_from_records(net, opt, records, cfg, 3, generator=torch.Generator().manual_seed(5), info=info)
    assert info == {"games": 32, "samples": int(rows.shape[0]), "invalid": 0}
    assert len(epochs) == 3 and all(e["epoch_samples"] == [2 * int(rows.shape[0])] for e in epochs)
    assert opt.param_groups[0]["lr"] == 2e-3                  # a constant rate
    after = selfplay.score_summary(selfplay.score_samples(ev, rows, write_back=False, chunk=8192), rows)
    print("policy loss per epoch", [e["policy_loss"] for e in epochs], "top-1", before["prior_top1_rate"], "->",
          after["prior_top1_rate"], "ce", before["mean_policy_ce"], "->", after["mean_policy_ce"])
    assert before["scored_samples"] == after["scored_samples"] == int(rows.shape[0])
    assert epochs[-1]["policy_loss"] < epochs[0]["policy_loss"]
    assert after["prior_top1_rate"] > before["prior_top1_rate"]


def test_extend_from_records_raises_or_drops():
    from xiangqi_alphazero_amd import hip, training
    records = _records()[[8, 1, 4]]                           # a whole game, one with an illegal ply, a one-ply game
    buf = training.ReplayBuffer(1000)
    with pytest.raises(hip.XqError, match=r"record 1 .*ply 3"):
        buf.extend_from_records(records, skip_opening=False)
    assert len(buf) == 0
    info = buf.extend_from_records(records, invalid="drop", skip_opening=False)
    assert info == {"games": 3, "samples": 7, "invalid": 1} and len(buf) == 14
    want = np.concatenate([M.record_rows(records[0], 0, False, False)[0], M.record_rows(records[2], 0, False, False)[0]])
    assert buf.store[:7].cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(hip.XqError, match="malformed"):
        training.ReplayBuffer(1000).extend_from_records(_records()[[3]])


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------
PLAIN = {"iteration", "time", "self_play", "training", "evaluation"}


def _config(tmp, **extra):
    return types.SimpleNamespace(**{**dict(
        num_channels=64, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=16,
        max_game_length=30, resign_threshold=-0.9, resign_check_steps=5, enable_resign=True, random_opening_moves=4,
        num_iterations=2, batch_size=64, num_epochs=1, learning_rate=0.002, weight_decay=1e-4, lr_milestones=[50, 80],
        lr_gamma=0.1, max_buffer_size=50000, min_buffer_size=100, eval_games=4, eval_win_rate=0.55, eval_simulations=8,
        checkpoint_dir=str(tmp), save_interval=2), **extra})


def test_loop_pretrains_a_fresh_run_once(tmp_path):
    import torch
    from xiangqi_alphazero_amd import train_loop
    from xiangqi_alphazero_amd.sample_format import records_to_text
    records = _ladder_games()
    path = tmp_path / "teacher.txt"
    path.write_text(records_to_text(records))
    cfg = _config(tmp_path / "ck", pretrain_records=str(path), pretrain_epochs=2, batch_size=512)
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    fresh = {k: v.clone() for k, v in loop.best_model.state_dict().items()}
    pre = loop.pretrain_from_records()                        # what train() runs before iteration 1
    assert any(not torch.equal(fresh[k], v) for k, v in loop.best_model.state_dict().items())
    assert all(torch.equal(v, loop.current_model.state_dict()[k]) for k, v in loop.best_model.state_dict().items())
    assert loop.scheduler.last_epoch == 0 and len(loop.buffer) == 0       # neither the loop's scheduler nor its buffer is touched
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    assert [s["iteration"] for s in stats] == [1, 2] and len(saved) == 2
    assert set(saved[0]) == PLAIN | {"pretrain"} and set(saved[1]) == PLAIN
    p = saved[0]["pretrain"]
    assert set(p) == {"games", "samples", "invalid", "epochs", "policy_loss", "value_loss", "seconds"}
    assert (p["games"], p["invalid"], p["epochs"]) == (32, 0, 2) and p["samples"] == int(M.sample_counts(records).sum())
    assert len(p["policy_loss"]) == len(p["value_loss"]) == 2 and p["seconds"] > 0
    assert all(np.isfinite(x) and x > 0 for x in p["policy_loss"] + p["value_loss"] + pre["policy_loss"])
    assert (pre["games"], pre["samples"], pre["invalid"]) == (p["games"], p["samples"], p["invalid"])
    # the same config without the keys: entries of the old form
    plain = train_loop.AlphaZeroLoop(_config(tmp_path / "plain"), "cuda", seed=3)
    assert plain.pretrain is None
    assert all(set(e) == PLAIN for e in plain.train())
