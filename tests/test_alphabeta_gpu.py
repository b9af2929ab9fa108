"""The fixed alpha-beta opponent on the GPU (include/xq_hip.h, xq_alphabeta_batch; baseline.play_vs_baseline) against the CPU
model of tests/alphabeta_model.py: every root move's score is the plain minimax value, the pick follows the draw, every output
word is written, and a match against it is a reproducible set of legal games."""
from functools import lru_cache

import numpy as np
import pytest

import alphabeta_model as M
import golden_io
from test_alphabeta_model import MATED

pytestmark = pytest.mark.gpu

SENTINEL = {"int16": -23131, "int32": -1515870811, "uint8": 0xA5}       # the byte 0xA5 in every byte of an element


def _run(boards, sides, depth, draws=None):
    """-> xq_alphabeta_batch's outputs as numpy arrays (moves / best_action as uint16)."""
    import torch
    from xiangqi_alphazero_amd import hip
    b = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 90)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(sides, dtype=np.int8).reshape(-1)).cuda()
    out = {k: v.cpu().numpy() for k, v in hip.alphabeta_batch(b, s, depth, draws).items()}
    out["moves"], out["best_action"] = out["moves"].view(np.uint16), out["best_action"].view(np.uint16)
    return out


@lru_cache(maxsize=None)
def _model(index, depth):
    """The model's outputs for corpus position `index` (None: the initial position; ('noking', i): position i without red's king)."""
    board, side = _position(index)
    return M.search(board, side, depth)


def _position(index):
    d = golden_io.corpus()
    if index is None:
        from oracle import xq_oracle as O
        return O.initial_board().reshape(90), 1
    if isinstance(index, tuple):
        b = d["board"][index[1]].copy()
        b[b == 1] = 0
        return b, int(d["side"][index[1]])
    return d["board"][index], int(d["side"][index])


def _check(out, row, index, depth, draw=None):
    """Row `row` of the device's outputs against the model of position `index`."""
    want = _model(index, depth)
    n = want["count"]
    assert int(out["counts"][row]) == n and int(out["status"][row]) == want["status"]
    assert (out["moves"][row] == want["moves"]).all()                          # zeros past the count
    assert (out["scores"][row].astype(np.int64) == want["scores"]).all(), (index, depth)       # XQ_AB_UNSCORED past the count
    got_nodes = out["nodes"][row].astype(np.int64)
    assert not got_nodes[n:].any()
    if depth == 0:
        assert not got_nodes.any()
    else:
        assert (got_nodes[:n] >= 1).all() and (got_nodes[:n] <= want["nodes"][:n]).all(), (index, depth)
    if n == 0:
        assert int(out["best_action"][row]) == M.NO_MOVE and int(out["best_score"][row]) == want["best_score"]
        return
    j, best = M.pick(want["scores"], n, draw)
    assert int(out["best_score"][row]) == best and int(out["best_action"][row]) == int(want["moves"][j]), (index, depth, draw)


def _corpus64():
    d = golden_io.corpus()
    idx = [int(i) for i in np.linspace(0, 4818, 64).astype(int) if not d["done"][i]]
    assert len(idx) >= 62                                  # at most 2 of the 64 are finished games
    return idx


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_corpus_positions_match_the_model(depth):
    d = golden_io.corpus()
    idx = _corpus64()
    boards, sides = d["board"][idx], d["side"][idx]
    out = _run(boards, sides, depth)
    for row, i in enumerate(idx):
        _check(out, row, i, depth)
    # with draws: small ones, the count itself and beyond it, and the largest uint32
    rng = np.random.default_rng(21 + depth)
    counts = np.array([_model(i, depth)["count"] for i in idx], dtype=np.uint64)
    draws = rng.integers(0, 8, size=len(idx), dtype=np.uint64)
    draws[1::4] = counts[1::4] + draws[1::4]
    draws[2::4] = 2 ** 32 - 1 - draws[2::4]
    draws[3::4] = rng.integers(0, 2 ** 32, size=len(draws[3::4]), dtype=np.uint64)
    out2 = _run(boards, sides, depth, draws)
    for row, i in enumerate(idx):
        _check(out2, row, i, depth, int(draws[row]))
    for k in ("moves", "counts", "scores", "nodes", "status", "best_score"):
        assert (out[k] == out2[k]).all(), k                # the draw moves the pick and nothing else
    if depth >= 1:
        assert (out["best_action"] != out2["best_action"]).any()


def test_depth_three_and_four():
    d = golden_io.corpus()
    three, four = [None, 800, 1500], [2000, 1985, 2185]    # the initial position and two midgames; 6, 7 and 7 pieces
    assert all((d["board"][i] != 0).sum() <= 12 for i in four)
    for depth, cases in ((3, three), (4, four)):
        pos = [_position(i) for i in cases]
        out = _run(np.stack([p[0] for p in pos]), [p[1] for p in pos], depth, [5, 1, 2 ** 32 - 1])
        for row, i in enumerate(cases):
            _check(out, row, i, depth, [5, 1, 2 ** 32 - 1][row])
    assert _model(None, 3)["best_score"] == 35 and _model(2000, 4)["nodes"].sum() == 2957
    assert _model(1985, 4)["best_score"] == M.MATE - 3     # a mate in two moves, seen at depth 4 only


@pytest.mark.parametrize("depth", [2, 3])
def test_mates_in_one_and_mated_positions(depth):
    d = golden_io.corpus()
    pred = [i - 1 for i in MATED]
    out = _run(d["board"][pred], d["side"][pred], depth)
    for row, i in enumerate(pred):
        _check(out, row, i, depth)
    assert (out["best_score"] == M.MATE - 1).all()         # depth 3 still prefers the quicker mate
    for row, i in enumerate(MATED):                        # the move found is a mate: the game's next position has no move
        nxt = M.child(d["board"][i - 1], int(out["best_action"][row]))
        assert len(M.O.legal_actions(nxt, int(d["side"][i]))) == 0
    mated = _run(d["board"][list(MATED)], d["side"][list(MATED)], depth)
    assert not mated["counts"].any() and not mated["status"].any() and not mated["moves"].any() and not mated["nodes"].any()
    assert (mated["best_action"] == M.NO_MOVE).all() and (mated["best_score"] == -M.MATE).all()
    assert (mated["scores"] == M.UNSCORED).all()


@pytest.mark.parametrize("n", [1, 5, 7])
def test_mixed_batch_writes_every_output(n):
    """One batch with every kind of position (a midgame, a king missing, a mated side, the initial position, an endgame), n no
    multiple of the four waves of a workgroup; every output buffer starts full of a sentinel and none of it is left.  The check is
    per element, not per byte: one byte of a real action, score or node count may well be 0xA5 (a score of 165 is), a whole
    element cannot (an action is below 8100, a count at most 128, a depth-2 score within the mate scores, a status at most 2)."""
    import torch
    from xiangqi_alphazero_amd import hip
    kinds = [800, ("noking", 800), MATED[0], None, 2000, ("noking", 1500), MATED[3]][:n] if n > 1 else [("noking", 800)]
    depth = 2
    pos = [_position(k) for k in kinds]
    boards = torch.from_numpy(np.stack([p[0] for p in pos]).astype(np.int8)).cuda()
    sides = torch.tensor([p[1] for p in pos], dtype=torch.int8).cuda()
    draws = torch.tensor([3, 0, 9, 2 ** 31 - 1, 1, 4, 4][:n], dtype=torch.int32).cuda()

    def fresh():
        shapes = dict(moves=((n, 128), torch.int16), counts=((n,), torch.int16), scores=((n, 128), torch.int32),
                      nodes=((n, 128), torch.int32), best_action=((n,), torch.int16), best_score=((n,), torch.int32),
                      status=((n,), torch.uint8))
        return {k: torch.full(s, SENTINEL[str(dt).split(".")[1]], dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}

    def call(buf, with_nodes=True, with_draws=True):
        rc = hip.lib().xq_alphabeta_batch(boards.data_ptr(), sides.data_ptr(), n, depth, draws.data_ptr() if with_draws else None,
                                          buf["moves"].data_ptr(), buf["counts"].data_ptr(), buf["scores"].data_ptr(),
                                          buf["nodes"].data_ptr() if with_nodes else None, buf["best_action"].data_ptr(),
                                          buf["best_score"].data_ptr(), buf["status"].data_ptr(), hip.stream_ptr(boards.device))
        assert rc == 0
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in buf.items()}
        out["moves"], out["best_action"] = out["moves"].view(np.uint16), out["best_action"].view(np.uint16)
        return out

    buf = fresh()
    word = {k: int(v.reshape(-1)[0].item()) for k, v in buf.items()}       # the sentinel as one element of each buffer
    assert all(bytes(v.cpu().numpy().tobytes()) == b"\xa5" * (v.numel() * v.element_size()) for v in buf.values())
    out = call(buf)
    for k, v in out.items():
        assert not (v == np.array(word[k]).astype(v.dtype)).any(), k       # no element still holds the sentinel
    for row, k in enumerate(kinds):
        _check(out, row, k, depth, int(draws[row].item()))
        if isinstance(k, tuple):
            assert out["status"][row] == 2 and out["counts"][row] == 0 and out["best_score"][row] == 0
    # without nodes and without draws: the nodes buffer is not touched, the rest is the same but the pick
    buf2 = fresh()
    out2 = call(buf2, with_nodes=False, with_draws=False)
    assert (out2["nodes"] == np.array(word["nodes"]).astype(np.int32)).all()
    for k in ("moves", "counts", "scores", "status", "best_score"):
        assert (out[k] == out2[k]).all(), k
    for row, k in enumerate(kinds):
        want = _model(k, depth)
        if want["count"]:
            assert int(out2["best_action"][row]) == want["best_action"]


@lru_cache(maxsize=None)
def _match(seed):
    import torch
    from xiangqi_alphazero_amd import baseline
    from xiangqi_alphazero_amd.model import XiangqiNet
    torch.manual_seed(5)
    net = XiangqiNet(64, 2).cuda().eval()
    return baseline.play_vs_baseline(net, 8, 2, 16, opening_plies=2, seed=seed, max_game_length=40)


def test_small_match_replays_and_the_baseline_moves_are_its_own():
    import torch
    from xiangqi_alphazero_amd import engine, hip
    res = _match(0)
    rec = res["game_records"]
    assert len(rec) == 8 and res["wins"] + res["losses"] + res["draws"] == 8 and res["pairs"] == 4
    assert res["win_rate"] == (res["wins"] + 0.5 * res["draws"]) / 8 and res["baseline_nodes"] > 0 and res["seconds"] > 0
    assert (rec["slot"] == np.arange(8)).all() and not rec["game_seq"].any() and not rec["n_samples"].any()
    st = {k: v.cpu().numpy() for k, v in engine.replay_games(rec).items()}
    assert not st["status"].any()
    for g in range(8):
        n, reason, winner = int(rec["n_moves"][g]), int(rec["reason"][g]), int(rec["winner"][g])
        assert not rec["moves"][g, n:].any() and n <= 40
        if reason == 2:                                    # not over at max_game_length: a draw
            assert n == 40 and winner == 0 and st["over_kind"][g] == 0
        else:
            assert reason == 1 and st["over_kind"][g] == 1 and st["winner"][g] == winner
    wins = sum(int(rec["winner"][g]) == (1 if g % 2 == 0 else -1) for g in range(8))
    assert wins == res["wins"] and res["draws"] == int((rec["winner"] == 0).sum())
    for p in range(4):                                     # a pair shares its opening
        k = int(rec["opening_plies"][2 * p])
        assert k == rec["opening_plies"][2 * p + 1] and k in (0, 2)
        assert (rec["moves"][2 * p, :k] == rec["moves"][2 * p + 1, :k]).all()
    assert (rec["opening_plies"] == 2).any()
    # one game of each colour, three plies spread over it: the baseline's move is alphabeta_batch's under the logged draw
    drawn = {(int(g), int(ply)): int(u) for g, ply, u in res["baseline_draws"]}
    for g in (0, 1):
        mine = sorted(ply for (gg, ply) in drawn if gg == g)
        assert len(mine) >= 3
        net_red = g % 2 == 0
        assert all((ply % 2 == 1) == net_red for ply in mine)        # the baseline moves when the network does not
        for ply in (mine[0], mine[len(mine) // 2], mine[-1]):
            at = engine.replay_games(rec[g:g + 1], stop_ply=ply)
            out = hip.alphabeta_batch(at["board"], at["side"], 2, [drawn[(g, ply)]])
            assert int(out["best_action"].cpu().numpy().view(np.uint16)[0]) == int(rec["moves"][g, ply]), (g, ply)
    torch.cuda.synchronize()


def test_match_is_a_function_of_its_seed():
    import torch
    from xiangqi_alphazero_amd import baseline
    from xiangqi_alphazero_amd.model import XiangqiNet
    first = _match(0)
    torch.manual_seed(5)
    net = XiangqiNet(64, 2).cuda().eval()
    again = baseline.play_vs_baseline(net, 8, 2, 16, opening_plies=2, seed=0, max_game_length=40)
    assert again["game_records"].tobytes() == first["game_records"].tobytes()
    assert (again["baseline_draws"] == first["baseline_draws"]).all()
    assert _match(1)["game_records"].tobytes() != first["game_records"].tobytes()


def test_baseline_against_baseline():
    from xiangqi_alphazero_amd import baseline, engine
    res = baseline.play_vs_baseline(1, 4, 0, 0, opening_plies=2, seed=3, max_game_length=60)     # depth 1 against depth 0
    rec = res["game_records"]
    assert res["games"] == 4 and res["wins"] + res["losses"] + res["draws"] == 4 and len(res["baseline_draws"]) > 0
    st = {k: v.cpu().numpy() for k, v in engine.replay_games(rec).items()}
    assert not st["status"].any()                          # every move was legal where it was played
    for g in range(4):
        if rec["reason"][g] == 2:
            assert rec["n_moves"][g] == 60 and rec["winner"][g] == 0
        else:
            assert rec["reason"][g] == 1 and st["over_kind"][g] == 1 and st["winner"][g] == rec["winner"][g]
    # both seats draw: one logged draw per move after the opening
    assert len(res["baseline_draws"]) == int((rec["n_moves"].astype(int) - rec["opening_plies"]).sum())
