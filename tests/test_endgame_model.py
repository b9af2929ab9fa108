"""The CPU model of the endgame tablebases (tests/endgame_model.py) pinned: published counts per signature, rotation and mirror
symmetry, the forced-mate model as a second opinion, and Bellman consistency.  The counts were computed by an independent
prototype over the oracle; the GPU suite then holds the kernels to this model word for word."""
import numpy as np
import pytest

import endgame_model as EM
import mate_model as MM
from xiangqi_alphazero_amd import endgame
from xiangqi_alphazero_amd.sample_format import MIR_SQ

# signature: entries, red to move (invalid, win, loss, draw), black to move, longest win in plies, passes
FIGURES = {
    "": (162, (27, 0, 0, 54), (27, 0, 0, 54), 0, 1),
    "P": (9072, (1656, 2394, 0, 486), (1467, 0, 2469, 600), 19, 21),
    "R": (14742, (3483, 3834, 0, 54), (2403, 0, 4806, 162), 3, 5),
    "C": (14742, (2403, 0, 0, 4968), (2403, 0, 0, 4968), 0, 1),
    "N": (14742, (2727, 4590, 0, 54), (2403, 0, 4806, 162), 13, 15),
    "aa": (5832, (1404, 0, 0, 1512), (1404, 0, 0, 1512), 0, 1),
    "Ra": (88452, (21576, 22341, 0, 309), (16197, 0, 26880, 1149), 9, 11),
    "CA": (88452, (16293, 22710, 0, 5223), (16197, 0, 22274, 5755), 17, 19),
    "Ca": (88452, (16689, 0, 0, 27537), (16197, 0, 0, 28029), 0, 1),
    "Pa": (54432, (10989, 3498, 0, 12729), (9993, 0, 2832, 14391), 19, 21),
    "Nb": (117936, (22146, 12258, 0, 24564), (19656, 0, 6868, 32444), 31, 32),
}


@pytest.mark.parametrize("signature", list(FIGURES))
def test_counts_per_signature(signature):
    entries, red, black, longest, passes = FIGURES[signature]
    m = EM.model(signature)
    assert m.entries == entries == len(m.table) and m.table.dtype == np.int16
    s = m.stats()
    assert (s["red"], s["black"], s["longest_win"], s["passes"]) == (red, black, longest, passes)
    # wins are odd, losses -(even + 1): every decided value is odd
    decided = m.table[(m.table != 0) & (m.table != EM.INVALID)].astype(np.int64)
    assert (np.abs(decided) % 2 == 1).all()


def _rotated(signature, other):
    """For every entry of `signature` the index of its 180-degree rotation with colours and side swapped, in `other`."""
    boards, sides = endgame.index_to_board(signature, np.arange(endgame.entries(signature)))
    return endgame.board_to_index(other, -boards[:, ::-1], -sides)


def test_pawn_table_rotates_into_the_black_pawns():
    a, b = EM.model("P"), EM.model("p")
    to = _rotated("P", "p")
    # every entry but the collisions is a board, and its rotation is an entry of the other table
    boards_ok = a.table != EM.INVALID
    assert (to[boards_ok] >= 0).all()
    assert (a.table[boards_ok] == b.table[to[boards_ok]]).all()
    # and entry for entry through the digits: the rotation maps digit d of P to the mirrored digit of p
    dig = endgame.index_to_digits("P", np.arange(a.entries))
    rot = np.stack([1 - dig[:, 0], 8 - dig[:, 2], 8 - dig[:, 1], np.where(dig[:, 3] == 55, 55, 54 - dig[:, 3])], axis=1)
    idx = ((rot[:, 0] * 9 + rot[:, 1]) * 9 + rot[:, 2]) * 56 + rot[:, 3]
    assert (a.table == b.table[idx]).all()


@pytest.mark.slow
def test_pawn_against_pawn_is_the_same_for_both_sides():
    m = EM.model("Pp")
    s = m.stats()
    assert m.entries == 508032
    assert s["red"] == s["black"] == (91863, 9075, 2555, 150523) and s["longest_win"] == 21


def test_rook_against_advisor_is_mirror_invariant():
    m = EM.model("Ra")
    boards, sides = endgame.index_to_board("Ra", np.arange(m.entries))
    valid = m.table != EM.INVALID
    to = endgame.board_to_index("Ra", boards[:, MIR_SQ], sides)
    assert (to[valid] >= 0).all() and (m.table[valid] == m.table[to[valid]]).all()
    # a collision's mirror is a collision or another invalid entry
    dig = endgame.index_to_digits("Ra", np.arange(m.entries))
    mk = np.array([2, 1, 0, 5, 4, 3, 8, 7, 6])
    rook = np.where(dig[:, 3] == 90, 90, MIR_SQ[np.minimum(dig[:, 3], 89)])
    adv_sq = endgame.piece_squares(-2)
    adv_of = {int(s): d for d, s in enumerate(adv_sq)}
    adv = np.array([5 if d == 5 else adv_of[int(MIR_SQ[adv_sq[d]])] for d in range(6)])[dig[:, 4]]
    idx = (((dig[:, 0] * 9 + mk[dig[:, 1]]) * 9 + mk[dig[:, 2]]) * 91 + rook) * 6 + adv
    assert (m.table == m.table[idx]).all()


@pytest.mark.parametrize("signature", ["R", pytest.param("N", marks=pytest.mark.slow), "Pa"])      # N: half a minute of search
def test_mate_model_agrees(signature):
    m = EM.model(signature)
    rng = np.random.default_rng(2025)
    rows = np.sort(rng.choice(np.nonzero(m.table != EM.INVALID)[0], size=150, replace=False))
    seen = set()
    for e in rows:
        v = int(m.table[e])
        want = (v + 1) // 2 if 0 < v <= 9 else 0
        got = MM.search(m.boards[e], int(m.sides[e]), 5, checks_only=False)["best_mate_in"]
        assert got == want, (signature, int(e), v)
        seen.add(want)
    if signature == "N":
        assert {1, 2, 3, 4, 5} <= seen


@pytest.mark.parametrize("signature", ["P", "N", "Ra", "Nb"])
def test_bellman_consistency(signature):
    m = EM.model(signature)
    t = m.table.astype(np.int64)
    mv = m.move_values()
    live = m.children >= 0
    has = m.counts > 0
    valid = t != EM.INVALID
    assert (t[valid & ~has] == -1).all() and not (live[~valid]).any()
    # the best of the move values: the quickest win, else a draw, else the slowest loss
    big = np.iinfo(np.int64).max
    wins = np.where(live & (mv > 0), mv, big).min(axis=1)
    draw = (live & (mv == 0)).any(axis=1)
    loss = np.where(live, mv, big).min(axis=1)
    best = np.where(wins < big, wins, np.where(draw, 0, loss))
    rows = valid & has
    assert (best[rows] == t[rows]).all()
    for e in np.nonzero(rows)[0][:: max(1, int(rows.sum()) // 50)]:
        assert EM.best_of(mv[e, :m.counts[e]]) == t[e]
