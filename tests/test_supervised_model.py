"""CPU checks of the host model of game records as training samples (tests/supervised_model.py) and of the loop's keys: the
model's counts against a plain loop over a table of headers; its rows on two handcrafted games (the sign of z for both sides, the
place of the one visit, zero tails, the status of an illegal ply); every bad `pretrain_*` key of the loop raising with its name."""
import itertools
import types

import numpy as np
import pytest

import supervised_model as M
from oracle import xq_oracle as O
from xiangqi_alphazero_amd.sample_format import GAME_RECORD_DTYPE, SAMPLE_DTYPE, iccs_to_action, records_to_text

HEADERS = [(n, o, w) for n in (0, 1, 2, 7, 504) for o in sorted({0, 1, n, n + 1}) for w in (-1, 0, 1)] + \
          [(5, 0, 2), (5, 0, -2), (505, 0, 1), (505, 505, 0), (600, 2, -1)]


def _plain_count(n, o, w, movers, skip_opening, skip_draws):
    """The issue's rule, ply by ply."""
    if n > 504 or o > n or w not in (-1, 0, 1):
        return 0
    count = 0
    for p in range(n):
        if skip_opening and p < o:
            continue
        if skip_draws and w == 0:
            continue
        red = p % 2 == 0
        if movers == 1 and not ((w == 1 and red) or (w == -1 and not red)):
            continue
        if movers == 2 and not red:
            continue
        if movers == 3 and red:
            continue
        count += 1
    return count


@pytest.mark.parametrize("movers,skip_opening,skip_draws", list(itertools.product(range(4), (False, True), (False, True))))
def test_counts_against_a_plain_loop(movers, skip_opening, skip_draws):
    records = np.zeros(len(HEADERS), dtype=GAME_RECORD_DTYPE)
    for r, (n, o, w) in zip(records, HEADERS):
        r["n_moves"], r["opening_plies"], r["winner"] = n, o, w
    want = [_plain_count(n, o, w, movers, skip_opening, skip_draws) for n, o, w in HEADERS]
    assert M.sample_counts(records, movers, None, skip_opening, skip_draws).tolist() == want
    # one mover set per record is the same rule record by record; a value outside [0, 3] makes the record malformed
    per = np.full(len(HEADERS), movers, dtype=np.uint8)
    per[::3] = 7
    got = M.sample_counts(records, 0, per, skip_opening, skip_draws).tolist()
    assert got == [0 if i % 3 == 0 else c for i, c in enumerate(want)]
    for (n, o, w) in HEADERS:
        plies, malformed = M.selection(n, o, w, movers, skip_opening, skip_draws)
        assert malformed == (n > 504 or o > n or w not in (-1, 0, 1)) and plies == sorted(plies)


def _game(moves, winner, opening=0, slot=3, game_seq=9):
    r = np.zeros((), dtype=GAME_RECORD_DTYPE)
    acts = [iccs_to_action(m) for m in moves.split()]
    r["n_moves"], r["winner"], r["opening_plies"], r["slot"], r["game_seq"] = len(acts), winner, opening, slot, game_seq
    r["moves"][:len(acts)] = acts
    return r


RED_WINS = _game("b2e2 h9g7 h0g2 i9h9 e2e6", 1, opening=1)
BLACK_WINS = _game("h2e2 b9c7 b0c2 a9b9", -1, slot=4, game_seq=1)


def _check_rows(rec, rows, plies):
    board, side = O.initial_board().reshape(90).copy(), 1
    at = {p: j for j, p in enumerate(plies)}
    for ply in range(int(rec["n_moves"])):
        a = int(rec["moves"][ply])
        if ply in at:
            s = rows[at[ply]]
            legal = O.legal_actions(board, side)
            assert (s["board"] == board).all() and s["side"] == side and s["ply"] == ply
            assert s["z"] == (0 if rec["winner"] == 0 else (1 if rec["winner"] == side else -1))
            assert s["n_moves"] == len(legal) and (s["actions"][:len(legal)] == legal).all()
            assert not s["actions"][len(legal):].any()                         # zero tails
            assert s["visits"].sum() == 1 and s["actions"][int(np.argmax(s["visits"]))] == a
            assert s["late_temp"] == 0 and s["reserved0"] == 0 and s["reserved1"] == 0 and not s["pad"].any()
            assert s["slot"] == rec["slot"] and s["game_seq"] == rec["game_seq"]
        frm, to = divmod(a, 90)
        board[to], board[frm] = board[frm], 0
        side = -side


def test_rows_of_two_handcrafted_games():
    rows, st = M.record_rows(RED_WINS, 0, True, False)
    assert st == 0 and rows.dtype == SAMPLE_DTYPE and rows["ply"].tolist() == [1, 2, 3, 4]
    assert rows["side"].tolist() == [-1, 1, -1, 1] and rows["z"].tolist() == [-1, 1, -1, 1]          # red won
    _check_rows(RED_WINS, rows, [1, 2, 3, 4])
    rows, st = M.record_rows(RED_WINS, 1, False, False)                     # the winner's plies, opening included
    assert st == 0 and rows["ply"].tolist() == [0, 2, 4] and rows["z"].tolist() == [1, 1, 1]
    _check_rows(RED_WINS, rows, [0, 2, 4])
    rows, st = M.record_rows(BLACK_WINS, 0, True, False)
    assert st == 0 and rows["side"].tolist() == [1, -1, 1, -1] and rows["z"].tolist() == [-1, 1, -1, 1]   # black won
    _check_rows(BLACK_WINS, rows, [0, 1, 2, 3])
    rows, st = M.record_rows(BLACK_WINS, 1, True, False)
    assert rows["ply"].tolist() == [1, 3] and rows["z"].tolist() == [1, 1]
    rows, st = M.record_rows(BLACK_WINS, 2, True, False)
    assert rows["ply"].tolist() == [0, 2] and rows["z"].tolist() == [-1, -1]
    drawn = BLACK_WINS.copy()
    drawn["winner"] = 0
    rows, st = M.record_rows(drawn, 0, True, False)
    assert st == 0 and rows["z"].tolist() == [0, 0, 0, 0]
    assert len(M.record_rows(drawn, 1, True, False)[0]) == 0 and len(M.record_rows(drawn, 0, True, True)[0]) == 0


def test_illegal_ply_malformed_records_and_wrong_offsets():
    bad = RED_WINS.copy()
    bad["moves"][2] = iccs_to_action("a0a5")              # a rook through its own pawn
    rows, st = M.record_rows(bad, 0, False, False)
    assert st == 3 and len(rows) == 5
    whole, _ = M.record_rows(RED_WINS, 0, False, False)
    assert rows[:2].tobytes() == whole[:2].tobytes() and not rows[2:].view(np.uint8).any()
    mal = RED_WINS.copy()
    mal["winner"] = 2
    records = np.array([RED_WINS, bad, mal, BLACK_WINS], dtype=GAME_RECORD_DTYPE)
    out = M.records_to_samples(records, skip_opening=False)
    assert out["counts"].tolist() == [5, 5, 0, 4] and out["offsets"].tolist() == [0, 5, 10, 10, 14]
    assert out["status"].tolist() == [0, 3, -1, 0]
    off = np.array([0, 5, 9, 9, 13], dtype=np.int32)      # record 1's gap is one short; record 3 keeps a right-sized range
    out2 = M.records_to_samples(records, skip_opening=False, offsets=off)
    assert out2["status"].tolist() == [0, -2, -1, 0]
    assert (out2["samples"][5:9] == 0xA5).all() and out2["samples"][9:13].tobytes() == out["samples"][10:14].tobytes()


def _config(**kw):
    return types.SimpleNamespace(**kw)


def test_loop_keys_are_checked_by_name(tmp_path):
    from xiangqi_alphazero_amd import hip
    from xiangqi_alphazero_amd.train_loop import _pretrain_options
    path = tmp_path / "games.txt"
    path.write_text(records_to_text(np.array([RED_WINS, BLACK_WINS], dtype=GAME_RECORD_DTYPE)))
    assert _pretrain_options(_config()) is None
    assert _pretrain_options(_config(pretrain_records=None, pretrain_epochs=3)) is None
    assert _pretrain_options(_config(pretrain_records=[])) is None
    p = _pretrain_options(_config(pretrain_records=str(path)))
    assert (p["epochs"], p["movers"], p["skip_draws"], len(p["records"])) == (1, 0, False, 2)
    assert p["records"].tobytes() == np.array([RED_WINS, BLACK_WINS], dtype=GAME_RECORD_DTYPE).tobytes()
    p = _pretrain_options(_config(pretrain_records=[str(path), path], pretrain_epochs=4, pretrain_movers=1, pretrain_skip_draws=True))
    assert (p["epochs"], p["movers"], p["skip_draws"], len(p["records"])) == (4, 1, True, 4)
    for key, values in (("pretrain_epochs", (0, -1, 1.5, True)), ("pretrain_movers", (-1, 4, 0.5, False)),
                        ("pretrain_skip_draws", (1, 0, "yes")), ("pretrain_records", (3, [3], {"a": 1}))):
        for v in values:
            kw = {"pretrain_records": str(path), key: v}
            with pytest.raises(hip.XqError, match=key):
                _pretrain_options(_config(**kw))
            if key != "pretrain_records":                  # a bad value is refused whether or not the feature is on
                with pytest.raises(hip.XqError, match=key):
                    _pretrain_options(_config(**{key: v}))
    with pytest.raises(OSError):
        _pretrain_options(_config(pretrain_records=str(tmp_path / "missing.txt")))
