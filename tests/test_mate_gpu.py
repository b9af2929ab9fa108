"""The forced-mate search on the GPU (include/xq_hip.h, xq_mate_search_batch) against the CPU model of tests/mate_model.py, word
for word: root moves, counts, every root move's mate-in and visit count, the best move, the best mate-in and the status; the node
limit cuts exactly where the model's does; every output word is written; and the shipped alpha-beta kernel proves the same mates."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import golden_io
import mate_model as M
from test_alphabeta_model import MATED

pytestmark = pytest.mark.gpu

CHECKS = tuple(range(500, 1101)) + tuple(range(1500, 1601))        # mates of every length 1 to 5 among them
NAMED = (503, 527, 539, 543, 847, 1057, 1509, 1511)
ANY = tuple(range(0, 4819, 40))
KEYS = ("moves", "counts", "mate_in", "nodes", "best_action", "best_mate_in", "status")


def _run(boards, sides, max_moves, checks_only=True, node_limit=2 ** 32 - 1):
    """-> xq_mate_search_batch's outputs as numpy arrays (moves / best_action as uint16, nodes as uint32)."""
    import torch
    from xiangqi_alphazero_amd import hip
    b = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 90)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(sides, dtype=np.int8).reshape(-1)).cuda()
    out = {k: v.cpu().numpy() for k, v in hip.mate_search_batch(b, s, max_moves, checks_only, node_limit).items()}
    assert sorted(out) == sorted(KEYS)
    out["moves"], out["best_action"] = out["moves"].view(np.uint16), out["best_action"].view(np.uint16)
    out["nodes"] = out["nodes"].view(np.uint32)
    return out


def _position(index):
    d = golden_io.corpus()
    if isinstance(index, tuple):                           # ('noking', i): position i without red's king
        b = d["board"][index[1]].copy()
        b[b == 1] = 0
        return b, int(d["side"][index[1]])
    return d["board"][index], int(d["side"][index])


@lru_cache(maxsize=None)
def _model(index, max_moves, checks_only=True, node_limit=None):
    board, side = _position(index)
    return M.search(board, side, max_moves, checks_only, node_limit)


def _check(out, row, want, what):
    n = want["count"]
    assert int(out["counts"][row]) == n and int(out["status"][row]) == want["status"], what
    assert (out["moves"][row] == want["moves"]).all(), what                      # zeros past the count
    assert (out["mate_in"][row] == want["mate_in"]).all(), what                  # zeros past the count
    assert (out["nodes"][row].astype(np.int64) == want["nodes"]).all(), what     # exact visits, zeros past the count
    assert int(out["best_mate_in"][row]) == want["best_mate_in"] and int(out["best_action"][row]) == want["best_action"], what


def _batch(indices, max_moves, checks_only=True, node_limit=None):
    pos = [_position(i) for i in indices]
    out = _run(np.stack([p[0] for p in pos]), [p[1] for p in pos], max_moves, checks_only,
               2 ** 32 - 1 if node_limit is None else node_limit)
    for row, i in enumerate(indices):
        _check(out, row, _model(i, max_moves, checks_only, node_limit), (i, max_moves, checks_only, node_limit))
    return out


@pytest.mark.parametrize("max_moves", [5, 1, 3])
def test_checks_only_matches_the_model(max_moves):
    out = _batch(CHECKS, max_moves)
    best = {i: int(out["best_mate_in"][CHECKS.index(i)]) for i in NAMED}
    assert sorted(set(best.values())) == ([] if max_moves == 5 else [0]) + list(range(1, max_moves + 1))
    if max_moves == 5:
        assert sorted(set(out["best_mate_in"].tolist())) == [0, 1, 2, 3, 4, 5] and not out["status"].any()
        again = _batch(CHECKS, 5)                          # the same bytes on a second run
        for k in KEYS:
            assert out[k].tobytes() == again[k].tobytes(), k


def test_all_moves_matches_the_model_and_the_alphabeta_kernel():
    import torch
    from xiangqi_alphazero_amd import hip
    out = _batch(ANY, 2, checks_only=False)
    d = golden_io.corpus()
    count = {m: int((out["best_mate_in"] == m).sum()) for m in (1, 2)}
    assert count == {1: 1, 2: 7}
    # root move j has mate_in m exactly when the depth-4 minimax scores it MATE - (2m - 1); mate_in 0 exactly when below MATE - 3
    idx = list(ANY)
    ab = hip.alphabeta_batch(torch.from_numpy(d["board"][idx].astype(np.int8)).cuda(),
                             torch.from_numpy(d["side"][idx].astype(np.int8)).cuda(), 4)
    scores, counts = ab["scores"].cpu().numpy().astype(np.int64), ab["counts"].cpu().numpy()
    assert (counts == out["counts"].view(np.int16)).all()
    seen = {0: 0, 1: 0, 2: 0}
    for row in range(len(idx)):
        for j in range(int(counts[row])):
            m, sc = int(out["mate_in"][row, j]), int(scores[row, j])
            assert m in (0, 1, 2)
            assert (sc == hip.AB_MATE - (2 * m - 1)) if m else (sc < hip.AB_MATE - 3), (idx[row], j, m, sc)
            seen[m] += 1
    assert all(seen.values())


@pytest.mark.parametrize("node_limit", [1, 7, 50])
def test_node_limit_cuts_where_the_model_does(node_limit):
    deep = [i for i in CHECKS if _model(i, 5)["best_mate_in"] >= 3]
    assert len(deep) >= 8 and set(NAMED) & set(deep)
    out = _batch(deep, 5, node_limit=node_limit)
    cut = kept = finished = 0
    for row, i in enumerate(deep):
        n, free = int(out["counts"][row]), _model(i, 5)
        unknown = out["mate_in"][row, :n] == M.UNKNOWN
        assert (unknown == (free["nodes"][:n] > node_limit)).all()
        assert (out["nodes"][row, :n][unknown] == node_limit).all() and (out["nodes"][row, :n] <= node_limit).all()
        assert (int(out["status"][row]) & 4 != 0) == bool(unknown.any()) and int(out["status"][row]) & 3 == 0
        searched = free["nodes"][:n] >= 1
        cut, kept, finished = cut + int(unknown.sum()), kept + int((~unknown).sum()), finished + int((searched & ~unknown).sum())
    # every searched root move of these positions needs 9 visits or more (the model's figure), so limits 1 and 7 cut them all
    # and leave the moves that give no check; 50 cuts some searches and lets others finish
    assert cut >= 1 and kept >= 1 and (finished >= 1) == (node_limit == 50)


@pytest.mark.parametrize("n", [1, 5])
def test_mixed_batch_writes_every_output(n):
    """One batch with every kind of position (a king missing, a mate in three, a mated side, a midgame, a mate in five), n no
    multiple of the four waves of a workgroup; every output buffer starts full of the byte 0xA5 and every word of it is written,
    up to XQ_MAXM: no legal output element holds that byte in all its bytes (an action is below 8100, a count at most 128, a
    mate-in at most 5 or 255, a status at most 6, a visit count of these positions far below 0xA5A5A5A5)."""
    import torch
    from xiangqi_alphazero_amd import hip
    kinds = [("noking", 800), 503, MATED[0], 800, 1509][:n]
    pos = [_position(k) for k in kinds]
    boards = torch.from_numpy(np.stack([p[0] for p in pos]).astype(np.int8)).cuda()
    sides = torch.tensor([p[1] for p in pos], dtype=torch.int8).cuda()
    shapes = dict(moves=((n, 128), torch.int16), counts=((n,), torch.int16), mate_in=((n, 128), torch.uint8),
                  nodes=((n, 128), torch.int32), best_action=((n,), torch.int16), best_mate_in=((n,), torch.uint8),
                  status=((n,), torch.uint8))
    fill = {torch.int16: -23131, torch.int32: -1515870811, torch.uint8: 0xA5}

    def call(with_nodes=True):
        buf = {k: torch.full(s, fill[dt], dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}
        opts = hip.MateOpts(5, 1, 2 ** 32 - 1, 0)
        rc = hip.lib().xq_mate_search_batch(boards.data_ptr(), sides.data_ptr(), n, C.byref(opts), buf["moves"].data_ptr(),
                                            buf["counts"].data_ptr(), buf["mate_in"].data_ptr(),
                                            buf["nodes"].data_ptr() if with_nodes else None, buf["best_action"].data_ptr(),
                                            buf["best_mate_in"].data_ptr(), buf["status"].data_ptr(),
                                            hip.stream_ptr(boards.device))
        assert rc == 0
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in buf.items()}
        out["moves"], out["best_action"] = out["moves"].view(np.uint16), out["best_action"].view(np.uint16)
        out["nodes"] = out["nodes"].view(np.uint32)
        return out

    out = call()
    for k, v in out.items():                               # no element still holds the byte in all its bytes
        assert not (np.ascontiguousarray(v).view(np.uint8).reshape(-1, v.itemsize) == 0xA5).all(axis=1).any(), k
    for row, k in enumerate(kinds):
        _check(out, row, _model(k, 5), k)
    assert out["status"][0] == 2 and out["counts"][0] == 0 and out["best_action"][0] == M.NO_MOVE and not out["nodes"][0].any()
    if n == 5:
        assert out["counts"][2] == 0 and out["status"][2] == 0 and out["best_action"][2] == M.NO_MOVE
        assert list(out["best_mate_in"]) == [0, 3, 0, 0, 5]
    # without nodes: that buffer is not touched, the rest is the same
    out2 = call(with_nodes=False)
    assert (out2["nodes"] == 0xA5A5A5A5).all()
    for k in KEYS:
        if k != "nodes":
            assert out[k].tobytes() == out2[k].tobytes(), k


def test_mated_roots():
    d = golden_io.corpus()
    out = _run(d["board"][list(MATED)], d["side"][list(MATED)], 3, checks_only=False)
    assert not out["counts"].any() and not out["status"].any() and not out["moves"].any() and not out["nodes"].any()
    assert not out["mate_in"].any() and not out["best_mate_in"].any() and (out["best_action"] == M.NO_MOVE).all()
    pred = [i - 1 for i in MATED]
    out = _run(d["board"][pred], d["side"][pred], 2, checks_only=False)
    assert (out["best_mate_in"] == 1).all()
    for row, i in enumerate(MATED):                        # the move found is a mate: the game's next position has no move
        nxt = M.child(d["board"][i - 1], int(out["best_action"][row]))
        assert len(M.O.legal_actions(nxt, int(d["side"][i]))) == 0
