"""CPU pins of the model of the forced-mate search (tests/mate_model.py: the recursion of include/xq_hip.h,
xq_mate_search_batch, over the oracle's move generator), of the FEN reader and writer, and of the puzzle file and the puzzle
filter on the model's labels."""
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import golden_io
import mate_model as M
from oracle import xq_oracle as O

START = "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR w"


@lru_cache(maxsize=None)
def corpus_search(max_moves=5):
    """Every corpus position under checks only: the model's outputs, in corpus order."""
    d = golden_io.corpus()
    return [M.search(d["board"][i], int(d["side"][i]), max_moves) for i in range(len(d["board"]))]


def test_corpus_mates_by_checks():
    """All 4 819 positions at N = 5: how many hold a mate of each length.  The search deepens one move at a time, so a root
    move's label at N = 3 is its label at N = 5 when that is at most 3, and 0 otherwise; the positions with a mate are run at
    N = 3 as well and must say the same.  (The largest visit total of one position is 2 253 under this model; the probe the
    issue quotes said 2 258, with the same counts.)"""
    d = golden_io.corpus()
    res = corpus_search()
    assert len(res) == 4819
    count = Counter(r["best_mate_in"] for r in res)
    assert dict(count) == {0: 4622, 1: 106, 2: 51, 3: 23, 4: 15, 5: 2}
    assert max(int(r["nodes"].sum()) for r in res) == 2253
    assert not any(r["status"] & 4 for r in res) and not any((r["mate_in"] == M.UNKNOWN).any() for r in res)
    three = Counter()
    for i, r in enumerate(res):
        want = np.where(r["mate_in"] <= 3, r["mate_in"], 0)
        three[int(min([m for m in want if m >= 1], default=0))] += 1
        if r["best_mate_in"] >= 1 and i % 3 == 0:
            r3 = M.search(d["board"][i], int(d["side"][i]), 3)
            assert (r3["mate_in"] == want).all() and (r3["nodes"] <= r["nodes"]).all(), i
    assert {m: c for m, c in three.items() if m} == {1: 106, 2: 51, 3: 23}
    # the positions the GPU test names hold mates of every length
    assert sorted({res[i]["best_mate_in"] for i in (503, 527, 539, 543, 847, 1057, 1509, 1511)}) == [1, 2, 3, 4, 5]


def test_corpus_mates_by_any_move():
    d = golden_io.corpus()
    idx = range(0, 4819, 40)
    res = [M.search(d["board"][i], int(d["side"][i]), 2, checks_only=False) for i in idx]
    assert len(res) == 121
    count = Counter(r["best_mate_in"] for r in res)
    assert {m: c for m, c in count.items() if m} == {1: 1, 2: 7}
    # a mate by checks is a mate by any move, and never a quicker one
    for i, r in zip(idx, res):
        c = corpus_search()[i]
        for j in range(r["count"]):
            if 1 <= c["mate_in"][j] <= 2:
                assert r["mate_in"][j] == c["mate_in"][j], (i, j)


def test_visits_and_the_node_limit():
    """A root move that gives no check costs nothing; one that does visits at least its child; a limit of L cuts exactly the
    searches that need more than L visits, and leaves the others as they are."""
    d = golden_io.corpus()
    for i in (527, 539, 543, 1057):
        b, s = d["board"][i], int(d["side"][i])
        free = corpus_search()[i]
        n = free["count"]
        for j in range(n):
            gives = O.is_in_check(M.child(b, int(free["moves"][j])), -s)
            assert (free["nodes"][j] >= 1) == bool(gives)
        for limit in (1, 7, 50):
            cut = M.search(b, s, 5, node_limit=limit)
            over = free["nodes"][:n] > limit
            assert (cut["mate_in"][:n][over] == M.UNKNOWN).all() and (cut["nodes"][:n][over] == limit).all()
            assert (cut["mate_in"][:n][~over] == free["mate_in"][:n][~over]).all()
            assert (cut["nodes"][:n][~over] == free["nodes"][:n][~over]).all()
            assert cut["status"] == (4 if over.any() else 0)


def test_edges():
    from test_alphabeta_model import MATED
    d = golden_io.corpus()
    for i in MATED:
        r = M.search(d["board"][i], int(d["side"][i]), 3)
        assert (r["count"], r["best_mate_in"], r["best_action"], r["status"]) == (0, 0, M.NO_MOVE, 0)
        p = M.search(d["board"][i - 1], int(d["side"][i - 1]), 1, checks_only=False)
        assert p["best_mate_in"] == 1
    b = O.initial_board().reshape(90).copy()
    b[4] = 0
    r = M.search(b, 1, 2)
    assert (r["status"], r["count"], r["best_mate_in"], r["best_action"]) == (2, 0, 0, M.NO_MOVE)
    assert M.best([0, 255, 3, 2, 2, 1], [10, 11, 12, 13, 14, 15], 5) == (2, 13)
    assert M.best([0, 255], [10, 11], 2) == (0, M.NO_MOVE)


# ---- FEN -----------------------------------------------------------------------------------------------------------------------

def test_fen_start_position():
    from xiangqi_alphazero_amd.sample_format import board_from_fen, board_to_fen
    board, side = board_from_fen(START)
    assert side == 1 and board.dtype == np.int8 and (board == O.initial_board().reshape(90)).all()
    assert board_to_fen(O.initial_board(), 1) == START
    assert board_to_fen(board, -1) == START[:-1] + "b"
    # E for B and H for N, r for w, further fields ignored
    other = "rheakaehr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RHEAKAEHR r - - 0 1"
    b2, s2 = board_from_fen(other)
    assert s2 == 1 and (b2 == board).all()
    assert board_from_fen(START[:-1] + "b")[1] == -1


def test_fen_round_trip_of_every_corpus_board():
    from xiangqi_alphazero_amd.sample_format import board_from_fen, board_to_fen
    d = golden_io.corpus()
    for i in range(len(d["board"])):
        text = board_to_fen(d["board"][i], int(d["side"][i]))
        b, s = board_from_fen(text)
        assert s == d["side"][i] and (b == d["board"][i]).all(), i
        assert board_to_fen(b, s) == text


@pytest.mark.parametrize("line", [
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR",              # no side
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR x",            # no such side
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/RNBAKABNR w",              # nine ranks
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/8/RNBAKABNR w",            # a rank of eight files
    "rnbakabnr/9/1c5c2/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR w",            # a rank of ten files
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBQKABNR w",            # no such piece
])
def test_fen_refuses_a_malformed_line(line):
    from xiangqi_alphazero_amd.sample_format import board_from_fen
    with pytest.raises(ValueError) as e:
        board_from_fen(line)
    assert line in str(e.value)


# ---- puzzles -------------------------------------------------------------------------------------------------------------------

def test_puzzle_text_round_trip_and_the_filter():
    from xiangqi_alphazero_amd import tactics
    from xiangqi_alphazero_amd.sample_format import MIR_SQ, SAMPLE_DTYPE
    d = golden_io.corpus()
    idx = list(range(500, 560))
    labelled = M.label(d["board"][idx], d["side"][idx], 5)
    assert (labelled["mate_in"] == [corpus_search()[i]["best_mate_in"] for i in idx]).all()
    text = tactics.puzzles_to_text(labelled, header=["sixty positions"])
    assert text.startswith("# sixty positions\n") and len(text.splitlines()) == 61
    back = tactics.puzzles_from_text(text + "\n# a comment\n\n")
    assert back.dtype == tactics.PUZZLE_DTYPE and len(back) == 60
    assert (back["board"] == labelled["board"]).all() and (back["side"] == labelled["side"]).all()
    assert not back["mate_in"].any() and not back["n_moves"].any()          # reading labels nothing
    # the filter: best mate-in within [min_moves, N], in order
    for lo, hi in ((2, 5), (1, 5), (2, 3), (4, 5)):
        got = tactics.select(labelled, hi, lo, unique=False)
        want = [k for k in range(60) if lo <= labelled["mate_in"][k] <= hi]
        assert len(want) > 0 and (got["board"] == labelled["board"][want]).all()
        assert (got["move_mate_in"] == labelled["move_mate_in"][want]).all()
    # unique: a second copy and a mirror image of a kept puzzle go, the first occurrence stays
    keep = tactics.select(labelled, 5, 2, unique=True)
    twice = np.concatenate([labelled, labelled[:30]])
    mirrored = labelled.copy()
    mirrored["board"] = labelled["board"][:, MIR_SQ]
    assert len(tactics.select(twice, 5, 2, unique=True)) == len(keep)
    both = tactics.select(np.concatenate([labelled, mirrored]), 5, 2, unique=True)
    assert len(both) == len(keep) and (both["board"] == keep["board"]).all()
    assert len(tactics.select(np.concatenate([labelled, mirrored]), 5, 2, unique=False)) == 2 * len(
        tactics.select(labelled, 5, 2, unique=False))
    # samples stand in for boards
    samples = np.zeros(3, dtype=SAMPLE_DTYPE)
    samples["board"], samples["side"] = d["board"][idx[:3]], d["side"][idx[:3]]
    b, s = tactics._positions(samples, None)
    assert (b == d["board"][idx[:3]]).all() and (s == d["side"][idx[:3]]).all()
    # the score of a choice is read off the labels
    solved = tactics.select(labelled, 5, 1, unique=False)
    sc = tactics.score(solved, solved["best_action"])
    assert sc["solved"] == sc["optimal"] == sc["puzzles"] == len(solved) and sc["solve_rate"] == 1.0
    assert sum(c for c, _ in sc["by_mate_in"].values()) == len(solved)
    worst = [int(p["moves"][int(np.argmin(np.where(p["move_mate_in"][:p["n_moves"]] == 0, -1, 0)))]) for p in solved]
    sc = tactics.score(solved, worst)
    assert sc["solved"] == sum(int(tactics.move_label(p, a) >= 1) for p, a in zip(solved, worst)) < len(solved)
