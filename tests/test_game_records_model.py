"""CPU: the text form of game records (sample_format.records_to_text / records_from_text) round-trips exactly, and the host
model of a game's move list (tests/game_record_model.py) is pinned against the oracle on the four recorded configurations."""
import numpy as np
import pytest

import game_record_model as GR
import golden_io as G
from oracle import xq_oracle as O
from xiangqi_alphazero_amd import sample_format as F

TRACES = G.game_traces()
CORNERS = (0, 8, 81, 89)               # a0, i0, a9, i9


def _record(n_moves, winner, reason, opening, slot, seq, n_samples, moves):
    r = np.zeros((), dtype=F.GAME_RECORD_DTYPE)
    r["n_moves"], r["winner"], r["reason"], r["opening_plies"] = n_moves, winner, reason, opening
    r["slot"], r["game_seq"], r["n_samples"] = slot, seq, n_samples
    r["moves"][:n_moves] = moves
    return r


def _hand_made():
    rng = np.random.default_rng(3)
    corner_moves = [f * 90 + t for f in CORNERS for t in CORNERS if f != t]
    recs = [_record(0, 0, 2, 0, 0, 1, 0, []),
            _record(504, 1, 1, 4, 3, 2, 200, rng.integers(0, 8100, 504)),
            _record(len(corner_moves), -1, 3, 0, 2 ** 32 - 1, 2 ** 32 - 1, 65535, corner_moves),
            _record(3, 1, 4, 16, 7, 9, 0, [1732, 6367, 110])]
    for reason in (1, 2, 3, 4):
        for winner in (1, -1, 0):
            recs.append(_record(2, winner, reason, 1, reason, winner + 5, 2, [1732, 6453]))
    return np.array(recs, dtype=F.GAME_RECORD_DTYPE)


def test_iccs_coordinates():
    assert [F.action_to_iccs(f * 90 + t) for f, t in ((0, 8), (8, 81), (81, 89), (89, 0))] == ["a0i0", "i0a9", "a9i9", "i9a0"]
    assert F.action_to_iccs(19 * 90 + 22) == "b2e2"          # the red cannon from b2 to the central file
    for a in (0, 8099, 1732, 89 * 90 + 88):
        assert F.iccs_to_action(F.action_to_iccs(a)) == a
    for bad in (-1, 8100):
        with pytest.raises(ValueError):
            F.action_to_iccs(bad)
    for bad in ("a0a", "j0a1", "a0a10", "aaa1"):
        with pytest.raises(ValueError):
            F.iccs_to_action(bad)


def test_text_round_trip_is_exact():
    recs = _hand_made()
    assert set(recs["reason"]) == {1, 2, 3, 4} and set(recs["winner"]) == {1, -1, 0} and {0, 504} <= set(recs["n_moves"])
    text = F.records_to_text(recs)
    lines = text.splitlines()
    assert len(lines) == len(recs) and text.endswith("\n")
    assert lines[0] == "1/2-1/2 reason=2 opening_plies=0 n_samples=0 slot=0 game_seq=1"
    assert lines[3] == "b2e2 h7e7 b0c2 1-0 reason=4 opening_plies=16 n_samples=0 slot=7 game_seq=9"
    assert lines[2].split()[:3] == ["a0i0", "a0a9", "a0i9"] and " 0-1 " in lines[2]
    assert len(lines[1].split()) == 504 + 6
    back = F.records_from_text(text)
    assert back.dtype == F.GAME_RECORD_DTYPE and back.tobytes() == recs.tobytes()
    assert F.records_from_text("# a comment\n\n" + text).tobytes() == recs.tobytes()
    assert len(F.records_from_text("")) == 0 and F.records_to_text(recs[:0]) == ""
    for bad in ("a0a1 reason=1 opening_plies=0 n_samples=0 slot=0 game_seq=1", "a0a1 1-0 reason=1", "a0a1 1-0 0-1 reason=1"):
        with pytest.raises(ValueError):
            F.records_from_text(bad)
    broken = recs[:1].copy()
    broken["n_moves"] = 505
    with pytest.raises(ValueError):
        F.records_to_text(broken)


def test_games_to_text_tool(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recs = _hand_made()
    np.save(tmp_path / "games.npy", recs)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "games_to_text.py"), str(tmp_path / "games.npy")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == F.records_to_text(recs)
    raw = recs.view(np.uint8).reshape(len(recs), 1024)      # a drained device tensor saved as bytes reads the same
    np.save(tmp_path / "raw.npy", raw)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "games_to_text.py"), str(tmp_path / "raw.npy"), "-o",
                        str(tmp_path / "games.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "games.txt").read() == F.records_to_text(recs)


@pytest.mark.parametrize("t", TRACES, ids=[t["name"] for t in TRACES])
def test_model_move_list_replays_on_the_oracle(t):
    c = t["cfg"]
    want = GR.expected_record(c, t["stub"] == "peaked", t["seed"])
    assert (want["winner"], want["n_moves"], want["n_samples"]) == (t["winner"], t["steps"], len(t["plies"]))
    assert 0 <= want["opening_plies"] <= c["random_opening_moves"] and len(want["moves"]) == want["n_moves"]
    g = GR.replay_on_oracle(want["moves"])                  # every move legal where it is played
    assert g.move_count == want["n_moves"] and bytes(g.board.reshape(90)) == bytes(want["final_board"])
    over, w = g.is_game_over()
    if over:
        winner = w
    elif g.move_count >= c["max_game_length"]:
        diff = O.material(g.board, 1) - O.material(g.board, -1)
        winner = 1 if diff > 30 else (-1 if diff < -30 else 0)
    else:                                                   # neither rules nor length: the side to move resigned
        assert c["enable_resign"]
        winner = -g.current_player
    assert winner == want["winner"]
    # the samples' boards are the positions the list passes through, at the plies after the opening
    g = O.Game()
    boards = {}
    for a in want["moves"]:
        boards[g.move_count] = bytes(g.board.reshape(90))
        g.make_action(a)
    sampled = [p for p in sorted(boards) if p >= want["opening_plies"]][:len(want["samples"])]
    assert [bytes(s["board"]) for s in want["samples"]] == [boards[p] for p in sampled]


def test_action_between():
    g = O.Game()
    for a in (1732, 6453, 182):
        before = g.board.reshape(90).copy()
        if a not in g.legal_actions():
            a = int(g.legal_actions()[0])
        g.make_action(a)
        assert GR.action_between(before, g.board) == a
