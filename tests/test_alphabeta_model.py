"""CPU pins of the model of the fixed alpha-beta opponent (tests/alphabeta_model.py: the plain minimax of include/xq_hip.h,
xq_alphabeta_batch, over the oracle's move generator): the initial position at depths 0 to 3, the corpus' mates in one, the pick
rule on the host (`baseline.pick` word for word), and the pruned search the kernel runs against the plain one."""
import numpy as np
import pytest

import alphabeta_model as M
import golden_io
from oracle import xq_oracle as O

# corpus positions that are over by "no legal move" (both kings stand); the predecessor of each is index - 1
MATED = (61, 383, 1110, 3179, 3343, 3606, 3692)
# how many root moves of each predecessor mate at once (plain minimax, depth 2): exactly one in five of them; the last two
# positions are endgames in which 4 and 12 different moves leave the other side without a legal move
MATING_MOVES = (1, 1, 1, 1, 1, 4, 12)


def _initial():
    return O.initial_board().reshape(90)


@pytest.mark.parametrize("depth,best,ties,first,nodes", [(1, 40, 2, 1792, 44), (2, -5, 2, 1792, 1964), (3, 35, 2, 1792, 81630)])
def test_initial_position(depth, best, ties, first, nodes):
    r = M.search(_initial(), 1, depth)
    n = r["count"]
    assert n == 44 and r["status"] == 0 and r["best_score"] == best
    reach = [j for j in range(n) if r["scores"][j] == best]
    assert len(reach) == ties and int(r["moves"][reach[0]]) == first == r["best_action"]
    assert int(r["nodes"][:n].sum()) == nodes
    assert (r["scores"][n:] == M.UNSCORED).all() and not r["nodes"][n:].any() and not r["moves"][n:].any()
    if depth == 1:
        # the two best moves are the cannon captures of a horse
        b = _initial()
        for j in reach:
            a = int(r["moves"][j])
            assert b[a // 90] == 6 and b[a % 90] == -4


def test_depth_zero_scores_nothing():
    r = M.search(_initial(), 1, 0)
    assert r["count"] == 44 and (r["scores"][:44] == 0).all() and not r["nodes"].any()
    assert r["best_action"] == int(r["moves"][0]) and r["best_score"] == 0
    assert M.search(_initial(), 1, 0, draw=45)["best_action"] == int(r["moves"][1])


def test_corpus_mates_in_one():
    d = golden_io.corpus()
    assert len(MATED) == 7
    for i, mating in zip(MATED, MATING_MOVES):
        assert d["done"][i] and len(golden_io.moves_of(d, i)) == 0 and M.kings_stand(d["board"][i])
        p = i - 1
        assert d["game"][p] == d["game"][i] and d["ply"][p] == d["ply"][i] - 1
        side = int(d["side"][p])
        r2 = M.search(d["board"][p], side, 2)
        assert r2["best_score"] == M.MATE - 1
        assert int((r2["scores"][:r2["count"]] == M.MATE - 1).sum()) == mating
        # the mating move is the one the game played
        played = M.child(d["board"][p], r2["best_action"]) if mating == 1 else None
        if played is not None:
            assert (played == d["board"][i]).all()
        r1 = M.search(d["board"][p], side, 1)
        assert abs(r1["best_score"]) < M.MATE - M.MAX_DEPTH       # depth 1 sees no mate
        # the mated position itself
        r = M.search(d["board"][i], int(d["side"][i]), 2)
        assert (r["count"], r["best_action"], r["best_score"], r["status"]) == (0, M.NO_MOVE, -M.MATE, 0)


def test_king_missing_is_status_two():
    b = _initial().copy()
    b[4] = 0
    r = M.search(b, 1, 2)
    assert (r["status"], r["count"], r["best_action"], r["best_score"]) == (2, 0, M.NO_MOVE, 0)
    assert (r["scores"] == M.UNSCORED).all()


def test_pick_rule():
    from xiangqi_alphazero_amd import baseline
    scores = [3, 7, -2, 7, 7, 1, 7, 99]            # 99 lies past the count
    for fn in (M.pick, baseline.pick):
        assert fn(scores, 7) == (1, 7)
        assert fn(scores, 7, 0) == (1, 7) and fn(scores, 7, 1) == (3, 7) and fn(scores, 7, 2) == (4, 7)
        assert fn(scores, 7, 3) == (6, 7) and fn(scores, 7, 4) == (1, 7)
        assert fn(scores, 7, 2 ** 32 - 1) == (6, 7)            # 4294967295 % 4 == 3
        assert fn(scores, 8, 5) == (7, 99)
        assert fn(scores, 0) == (None, None) and fn([], 0, 5) == (None, None)
        assert fn([M.UNSCORED + 1, M.UNSCORED + 1], 2, 1) == (1, M.UNSCORED + 1)
    assert baseline.pick(np.array(scores, dtype=np.int32), np.int16(7), np.uint32(2)) == (4, 7)


@pytest.mark.parametrize("index,depth", [(None, 2), (None, 3), (1500, 2), (1500, 3), (3178, 3), (2000, 4)])
def test_pruned_search_gives_the_minimax_score_of_every_root_move(index, depth):
    """Fail-soft alpha-beta in move order below a full-window root child, the leaves of the last level scored at once: the same
    score for every root move, and never more positions than plain minimax visits."""
    d = golden_io.corpus()
    board, side = (_initial(), 1) if index is None else (d["board"][index], int(d["side"][index]))
    r = M.search(board, side, depth)
    n = r["count"]
    scores, nodes = M.alphabeta_root(board, side, depth)
    assert n > 0 and scores == [int(x) for x in r["scores"][:n]]
    assert all(1 <= a <= b for a, b in zip(nodes, r["nodes"][:n]))
