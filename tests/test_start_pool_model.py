"""The host models of the start-position pool (tests/start_pool_model.py), on the CPU.

* `check_position` gives status 0 or 16 for every position of the corpus, which recorded games reached: 4812 and 7 of the 4819.
  The crafted boards are another matter: the fixture holds boards no game reaches -- boards without a king, the side that is not
  to move in check, and about 390 random "soups" with pieces where they can never stand -- so by the bits' own definitions most of
  them are fatal (417 boards: 238 times 4, 142 times 12, 11 times 2, 8 times 8, 8 times 0, 7 times 20, 3 times 28).  They are
  checked against what the fixture itself records of them: a missing king is bit 2, the recorded check of the side not to move
  is bit 8, the recorded "has no move" is bit 16, and every board whose recorded facts are clean and whose pieces stand where
  they may is 0 or 16;
* each fatal bit has a crafted board that sets it alone;
* from the initial board `play_game_from` is `selfplay_model.play_game` without an opening, on every recorded game.
"""
import numpy as np
import pytest

import golden_io as G
import selfplay_model as SM
import start_pool_model as SP
from draws import Draws
from oracle import xq_oracle as O


def kr_k():
    """K+R against K, red to move: a won ending."""
    b = np.zeros((10, 9), dtype=np.int8)
    b[0, 4], b[9, 3], b[4, 0] = 1, -1, 5
    return b.reshape(90), 1


def bad_boards():
    """name -> (board, side, status): each fatal bit alone, and bit 1 through the side."""
    init = O.initial_board().reshape(90).astype(np.int8)
    out = {}
    b = init.copy(); b[40] = 9
    out["square_out_of_range"] = (b, 1, 1)
    out["side_out_of_range"] = (init.copy(), 0, 1)
    b = init.copy(); b[4], b[13] = 0, 0; b[31] = 1                  # the red king on (3, 4): outside its palace
    out["king_outside_palace"] = (b, 1, 2)
    b = init.copy(); b[4] = 0
    out["no_red_king"] = (b, -1, 2)
    b = init.copy(); b[27], b[28] = 0, 7                            # a red pawn on (3, 1): before the river, an odd column
    out["pawn_on_odd_column"] = (b, 1, 4)
    b = init.copy(); b[40] = 5                                      # a third red rook
    out["three_rooks"] = (b, 1, 4)
    b, _ = kr_k(); b = b.copy(); b[36], b[39] = 0, 5                # the rook on (4, 3) checks the black king, red to move
    out["side_not_to_move_in_check"] = (b, 1, 8)
    return out


def test_corpus_positions_are_accepted():
    c = G.corpus()
    got = np.array([SP.check_position(c["board"][i], c["side"][i]) for i in range(len(c["board"]))])
    assert set(np.unique(got).tolist()) <= {0, 16}
    over_no_move = np.array([not O.has_legal_moves(c["board"][i], int(c["side"][i])) for i in range(len(got))])
    assert ((got == 16) == over_no_move).all() and (got == 16).sum() == 7


def test_crafted_boards_agree_with_their_recorded_facts():
    c = G.crafted()
    seen = set()
    for i in range(len(c["board"])):
        board, side = c["board"][i], int(c["side"][i])
        st = SP.check_position(board, side)
        seen.add(st)
        kings_missing = bool((c["kings"][i] < 0).any())
        if kings_missing:
            assert st == 2, c["names"][i]
        if st & 3:
            assert not st & ~3
            continue
        other_in_check = bool(c["in_check"][i][0 if side == -1 else 1])
        assert bool(st & 8) == other_in_check, c["names"][i]
        assert bool(st & 16) == (not c["has_moves"][i]), c["names"][i]
        if not st & 4 and not other_in_check:
            assert st in (0, 16), c["names"][i]
    assert seen >= {0, 2, 4, 8} and any(s & 16 for s in seen)


@pytest.mark.parametrize("name", sorted(bad_boards()))
def test_each_fatal_bit_alone(name):
    board, side, want = bad_boards()[name]
    assert SP.check_position(board, side) == want and want & SP.FATAL
    assert SP.check_position(*kr_k()) == 0 and SP.check_position(O.initial_board(), 1) == 0


@pytest.mark.parametrize("trace", G.game_traces(), ids=[t["name"] for t in G.game_traces()])
def test_play_game_from_initial_board_is_the_plain_game_without_opening(trace):
    cfg = dict(trace["cfg"], random_opening_moves=0)
    peaked = trace["stub"] == "peaked"
    want, winner, plies, _ = SM.play_game(cfg, peaked, Draws(trace["seed"]))
    got, w, n = SP.play_game_from(cfg, peaked, Draws(trace["seed"]), O.initial_board(), 1)
    assert (w, n, len(got)) == (winner, plies, len(want)) and len(got) > 0
    for a, b in zip(got, want):
        assert bytes(a["board"]) == bytes(b["board"]) and a["player"] == b["player"] and a["z"] == b["z"] and a["late"] == b["late"]
        assert list(a["actions"]) == list(b["actions"]) and list(a["visits"]) == list(b["visits"])
