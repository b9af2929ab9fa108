"""The crafted positions of tests/test_capacity_edges_gpu.py, refereed on the CPU oracle: their move counts, the oracle's own
200-move buffer, and what the searches of the GPU test meet on the way."""
import numpy as np

import capacity_boards as CB
import golden_io as G
from oracle import xq_oracle as O
from stub_eval import predict_from_key, state_key


def test_crafted_boards_have_the_stated_move_counts():
    for k, n in CB.ROOK_COUNTS.items():
        b = CB.rook_board(k)
        assert int((b == 5).sum()) == k and int((b != 0).sum()) == k + 2
        assert O.find_king(b, 1) == (0, 4) and O.find_king(b, -1) == (9, 3)
    assert CB.ROOK_COUNTS == {7: 121, 8: 139, 9: 152}
    for n in CB.ALL_COUNTS:
        b = CB.edge_board(n)
        red, black = O.legal_actions(b, 1), O.legal_actions(b, -1)
        assert len(red) == n and len(red) <= O.MAX_MOVES, n
        assert len(set(red.tolist())) == n                     # distinct actions: a list, not a padded buffer
        assert not O.is_in_check(b, 1), n
        assert len(black) == 1, n
    for n in (127, 128, 129):                                  # one piece away from the k = 8 board
        assert int((CB.edge_board(n) != CB.rook_board(8)).sum()) == 1


def test_crafted_boards_are_not_over():
    for n in CB.ALL_COUNTS:
        g = O.Game()
        g.set_board(CB.edge_board(n), 1)
        assert g.is_game_over() == (False, None), n


def test_planes_round_trip():
    d = G.corpus()
    for i in range(3, len(d["board"]), 611):
        b, side = CB.board_from_planes(O.encode_state(d["board"][i], int(d["side"][i])))
        np.testing.assert_array_equal(b, d["board"][i])
        assert side == int(d["side"][i])


def test_search_from_the_128_move_board_never_meets_a_longer_list():
    """The GPU test expects overflow == 0 from a 64-simulation search of the 128-move board: every position that search
    generates moves for (the root and each evaluated leaf; its other leaves have no king or no move, and it stays too shallow
    for the repetition rule, which needs 6 plies) has at most 128 of them, so nothing is truncated."""
    g = O.Game()
    g.set_board(CB.edge_board(128), 1)
    seen = []

    def predict(state):
        b, side = CB.board_from_planes(state)
        seen.append(len(O.legal_actions(b, side)))
        return predict_from_key(state_key(state), True)

    res = O.mcts_search(g, 64, predict)
    assert res.n_children == 128 and seen[0] == 128
    assert max(seen) <= CB.MAXM and res.max_depth < 6
