"""The table as opponent and teacher on the GPU (csrc/xq_tablebase.hip: k_tb_play, k_tb_samples; endgame.py; train_loop's
endgame_playout_* and endgame_teacher_* keys): xq_tb_play_batch and xq_tb_samples equal the CPU model (tests/endgame_play_model.py)
output for output and byte for byte over whole tables, a walk in place on the device takes exactly the table's distance, and
play_out_with, play_out and the loop do what they say.  Every comparison is exact."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import endgame_model as EM
import endgame_play_model as PM
import golden_io
from test_baseline_loop_gpu import PLAIN, _config

pytestmark = pytest.mark.gpu

WPW = 4
PLAY_KEYS = ("status", "value", "played", "move_value", "value_out", "side", "boards")
# the "endgame" entry as tests/test_endgame_gpu.py pins it, and the new entry beside it
ENTRY = {"signature", "kind", "positions", "held", "optimal", "hold_rate", "by_kind", "simulations", "seconds"}
PLAYOUT = {"signature", "positions", "converted", "dropped", "repeated", "unfinished", "conversion_rate", "conversion_se",
           "mean_plies_ratio", "simulations", "max_plies", "seconds"}


@lru_cache(maxsize=None)
def _table(signature):
    from xiangqi_alphazero_amd import hip
    return hip.tb_generate(signature, "cuda")[0]


@lru_cache(maxsize=None)
def _tb(signature):
    from xiangqi_alphazero_amd import endgame
    return endgame.Tablebase.generate(signature, "cuda")


def _actions(actions):
    return torch.from_numpy(np.asarray(actions, dtype=np.int64).astype(np.uint16).view(np.int16)).cuda()


def _host(out):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["played"] = got["played"].view(np.uint16)
    return got


def _play(signature, boards, sides, actions=None, out=None):
    from xiangqi_alphazero_amd import hip
    b = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(sides, dtype=np.int8)).cuda()
    r = hip.tb_play_batch(signature, _table(signature), b, s, None if actions is None else _actions(actions), out)
    torch.cuda.synchronize()
    return _host(r)


def _same(got, want, rows, what):
    for key in PLAY_KEYS:
        bad = np.nonzero((got[key].astype(np.int64) != want[key].astype(np.int64)).reshape(len(rows), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, key, len(bad), rows[bad[:3]], got[key][bad[:3]], want[key][bad[:3]])


@pytest.mark.parametrize("signature", ["Ra", "Nb"])
def test_play_equals_the_model_over_the_whole_table(signature):
    from xiangqi_alphazero_amd import endgame
    pm = PM.play_model(signature)
    m = pm.m
    collide = endgame.index_to_board(signature, np.arange(m.entries), return_collisions=True)[2]
    every = np.nonzero(~collide)[0]             # a collision's board shows another entry
    want = pm.play(every)
    got = _play(signature, m.boards[every], m.sides[every])
    assert set(got) == set(PLAY_KEYS)
    _same(got, want, every, signature)
    t = m.table[every]
    assert ((got["status"] == 4) == (t == EM.INVALID)).all() and ((got["status"] == 8) == (t == -1)).all()
    assert set(np.unique(got["status"]).tolist()) == {0, 4, 8}
    assert (got["value"][got["status"] == 8] == -1).all() and (got["played"][got["status"] != 0] == EM.NO_MOVE).all()
    # an action tensor of NO_MOVE is the table choosing, and batches that end inside a workgroup give the same words
    for lo, hi in ((7, 8), (100, 100 + WPW - 1), (len(every) - (WPW + 1), len(every))):
        part = _play(signature, m.boards[every[lo:hi]], m.sides[every[lo:hi]], [EM.NO_MOVE] * (hi - lo))
        _same(part, {k: v[lo:hi] for k, v in want.items()}, every[lo:hi], (signature, lo, hi))


@lru_cache(maxsize=None)
def _given():
    """512 seeded entries of "Ra" with every legal move of each, one action per row -> (entries per row, actions)."""
    m = EM.model("Ra")
    pool = np.nonzero((m.table != EM.INVALID) & (m.counts > 0))[0]
    picked = np.sort(np.random.default_rng(21).choice(pool, size=512, replace=False))
    rows = np.repeat(picked, m.counts[picked])
    actions = np.concatenate([m.moves[e, :m.counts[e]] for e in picked.tolist()]).astype(np.int64)
    return picked, rows, actions


def test_play_with_a_given_action():
    pm = PM.play_model("Ra")
    m = pm.m
    picked, rows, actions = _given()
    assert len(rows) == int(m.counts[picked].sum()) > 512
    got = _play("Ra", m.boards[rows], m.sides[rows], actions)
    _same(got, pm.play(rows, actions), rows, "given")
    assert (got["status"] == 0).all() and (got["played"] == actions).all() and (got["value"] == m.table[rows]).all()
    c = got["value_out"].astype(np.int64)
    assert (got["move_value"] == np.where(c < 0, -c, np.where(c > 0, -(c + 2), 0))).all()          # the probe's relation
    assert (got["boards"] == np.stack([PM.apply_move(m.boards[e], a) for e, a in zip(rows.tolist(), actions.tolist())])).all()
    assert (got["side"] == -m.sides[rows]).all()
    assert set(np.sign(got["move_value"]).tolist()) == {-1, 0, 1}          # moves that win, draw and lose are all among them
    # a non-move: action 0, and a legal move of another row
    other = []
    for i, e in enumerate(picked.tolist()):
        own = set(m.moves[e, :m.counts[e]].tolist())
        other.append(next(int(a) for f in picked[i + 1:].tolist() + picked[:i].tolist() for a in m.moves[f, :m.counts[f]] if int(a) not in own))
    for acts in ([0] * len(picked), other):
        got = _play("Ra", m.boards[picked], m.sides[picked], acts)
        _same(got, pm.play(picked, acts), picked, "non-move")
        assert (got["status"] == 16).all() and (got["boards"] == m.boards[picked]).all() and (got["side"] == m.sides[picked]).all()
        assert (got["value"] == m.table[picked]).all() and (got["played"] == EM.NO_MOVE).all()
        assert (got["move_value"] == 0).all() and (got["value_out"] == 0).all()
    # corpus positions hold pieces the signature lacks
    d = golden_io.corpus()
    for acts in (None, [0] * 64):
        got = _play("Ra", d["board"][:64], d["side"][:64], acts)
        assert (got["status"] == 1).all() and (got["boards"] == d["board"][:64].reshape(64, 90)).all() and (got["side"] == d["side"][:64]).all()
        assert (got["played"] == EM.NO_MOVE).all()
        assert not got["value"].any() and not got["move_value"].any() and not got["value_out"].any()


def _in_place(boards, side):
    """An `out` of tb_play_batch whose boards and side are the inputs themselves."""
    n = len(side)
    words = {k: torch.zeros(n, dtype=torch.int16, device="cuda") for k in ("played", "value", "move_value", "value_out")}
    return {"boards": boards, "side": side, **words, "status": torch.zeros(n, dtype=torch.uint8, device="cuda")}


def test_aliased_outputs_give_the_same_bytes():
    from xiangqi_alphazero_amd import hip
    m = EM.model("Ra")
    _, rows, actions = _given()
    for acts in (None, actions):
        separate = _play("Ra", m.boards[rows], m.sides[rows], acts)
        boards, side = torch.from_numpy(m.boards[rows]).cuda(), torch.from_numpy(m.sides[rows]).cuda()
        r = hip.tb_play_batch("Ra", _table("Ra"), boards, side, None if acts is None else _actions(acts), _in_place(boards, side))
        torch.cuda.synchronize()
        assert r["boards"] is boards and r["side"] is side
        got = _host(r)
        for key in PLAY_KEYS:
            assert got[key].tobytes() == separate[key].tobytes(), key


def test_the_walk_in_place_takes_the_tables_distance():
    from xiangqi_alphazero_amd import hip
    pm = PM.play_model("Ra")
    m = pm.m
    won = np.nonzero(m.table > 0)[0]
    p = m.table[won].astype(np.int64)
    want_plies, want_values = pm.walk_all(won)
    assert (want_plies == p).all() and int(p.max()) == 9 and len(want_values) == 10
    boards, side = torch.from_numpy(m.boards[won]).cuda(), torch.from_numpy(m.sides[won]).cuda()
    out = _in_place(boards, side)
    plies = np.zeros(len(won), dtype=np.int64)
    for step in range(10):
        prior = boards.clone()
        hip.tb_play_batch("Ra", _table("Ra"), boards, side, None, out)
        status = out["status"].cpu().numpy()
        assert set(np.unique(status).tolist()) <= {0, 8}
        # +p, -p, +(p - 2), ..., +1, -1: the value before every ply, and -1 for good once the defender has no move
        assert (out["value"].cpu().numpy() == want_values[step]).all(), step
        assert ((status == 8) == (step >= p)).all(), step
        assert torch.equal(boards[torch.from_numpy(status == 8).cuda()], prior[torch.from_numpy(status == 8).cuda()])
        plies += status == 0
    assert (status == 8).all() and (plies == p).all()        # the longest game takes 9 steps: the tenth call moves nothing
    assert int((plies == 9).sum()) > 0


# ---- the table as teacher ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signature", ["R", "Nb"])
@pytest.mark.parametrize("policy", [0, 1])
def test_samples_equal_the_model_byte_for_byte(signature, policy):
    from xiangqi_alphazero_amd import hip
    pm = PM.play_model(signature)
    m = pm.m
    index = np.concatenate([[-1, m.entries], np.arange(m.entries)])
    want, want_status = pm.sample_rows(index, policy)
    rows, status = hip.tb_samples(signature, _table(signature), torch.from_numpy(index.astype(np.int32)).cuda(), policy)
    torch.cuda.synchronize()
    got, got_status = rows.cpu().numpy(), status.cpu().numpy()
    assert got.shape == (len(index), 640) and got.dtype == np.uint8
    assert (got_status == want_status).all() and got_status[:2].tolist() == [1, 1] and set(np.unique(got_status).tolist()) >= {0, 1, 4}
    bad = np.nonzero((got != want.view(np.uint8).reshape(-1, 640)).any(axis=1))[0]
    assert len(bad) == 0, (signature, policy, len(bad), index[bad[:3]])
    assert not got[got_status != 0].any()               # the zero-row convention
    # a batch that ends inside a workgroup
    few, few_status = hip.tb_samples(signature, _table(signature), torch.from_numpy(index[:WPW + 3].astype(np.int32)).cuda(), policy)
    assert few.cpu().numpy().tobytes() == got[:WPW + 3].tobytes() and (few_status.cpu().numpy() == got_status[:WPW + 3]).all()


def test_samples_feed_the_training_path():
    from xiangqi_alphazero_amd import endgame, hip
    from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE
    from xiangqi_alphazero_amd.training import ReplayBuffer
    tb = _tb("R")
    m = EM.model("R")
    pm = PM.play_model("R")
    _, _, index = tb.entries_of(n=300, seed=6)
    host = tb.samples(index)
    assert host.dtype == SAMPLE_DTYPE and host.tobytes() == pm.sample_rows(index, 0)[0].tobytes()
    assert tb.samples(index, policy=1).tobytes() == pm.sample_rows(index, 1)[0].tobytes()
    # the exact outcome is already there: rescoring changes none
    again, covered, changed = endgame.rescore_samples(host, tb)
    assert (covered, changed) == (300, 0) and again.tobytes() == host.tobytes()
    # entries that give no sample are refused by name or dropped
    dead = int(np.nonzero(m.table == -1)[0][0])
    mixed = np.concatenate([index[:5], [dead, m.entries, int(np.nonzero(m.table == EM.INVALID)[0][0])], index[5:9]])
    with pytest.raises(hip.XqError, match=f"entry {dead} .* has no legal move"):
        tb.samples(mixed)
    assert tb.samples(mixed, invalid="drop").tobytes() == host[:9].tobytes()
    # the replay buffer takes the device tensor, and the batch kernel reads the rows: pi sums to 1 with mass on optimal moves only
    rows = tb.samples(index, as_tensor=True)
    assert rows.is_cuda and rows.dtype == torch.uint8 and tuple(rows.shape) == (300, 640)
    buf = ReplayBuffer(max_size=1000, device="cuda")
    buf.extend(rows)
    assert len(buf) == 600 and buf.store[:300].cpu().numpy().tobytes() == host.tobytes()
    _, pi, z = buf.batch(torch.arange(0, 600, 2, device="cuda"))         # the un-mirrored sample of every record
    pi, z = pi.cpu().numpy().astype(np.float64), z.cpu().numpy().reshape(-1)
    assert (z == np.sign(m.table[index])).all()
    # at most 128 float32 terms of 1 / k each: the sum is within 128 ulps of 1
    assert (np.abs(pi.sum(axis=1) - 1.0) <= 128 * 2.0 ** -24).all()
    for j, e in enumerate(index.tolist()):
        k = int(m.counts[e])
        best = m.moves[e, :k][pm.optimal(e)].astype(np.int64)
        mass = np.nonzero(pi[j])[0]
        assert sorted(mass.tolist()) == sorted(best.tolist()), e
        assert np.abs(pi[j, best] - 1.0 / len(best)).max() <= 2.0 ** -24


# ---- the table as opponent ---------------------------------------------------------------------------------------------------
def _best(tb):
    def choose(games):
        return tb.probe(np.stack([g.board for g in games]), [g.current_player for g in games], move_values=False)["best_action"]
    return choose


def _check_games(tb, boards, sides, result, max_plies):
    """Every game's move list replayed through Tablebase.play, ply by ply: every move is legal, and the game ended where and why
    its outcome says."""
    from xiangqi_alphazero_amd import endgame
    games = result["games"]
    assert len(games) == result["positions"] == len(boards)
    assert sum(result[o] for o in endgame.OUTCOMES) == len(games)
    assert all(result[o] == sum(g["outcome"] == o for g in games) for o in endgame.OUTCOMES)
    cur = np.asarray(boards, dtype=np.int8).reshape(-1, 90).copy()
    side = np.asarray(sides, dtype=np.int8).copy()
    seen = [[cur[j].tobytes()] for j in range(len(games))]
    last = [None] * len(games)
    ply = 0
    while True:
        live = [j for j, g in enumerate(games) if len(g["moves"]) > ply]
        if not live:
            break
        r = tb.play(cur[live], side[live], [games[j]["moves"][ply] for j in live])
        assert (r["status"] == 0).all(), (ply, [games[j] for j in np.array(live)[r["status"] != 0][:3]])
        for k, j in enumerate(live):
            cur[j], side[j] = r["boards"][k], r["side"][k]
            last[j] = (int(r["move_value"][k]), int(r["value_out"][k]))
            if ply % 2 == 1:
                seen[j].append(cur[j].tobytes())
            elif len(games[j]["moves"]) > ply + 1:
                assert r["move_value"][k] > 0 and r["value_out"][k] != -1        # the game went on: still won, not yet over
        ply += 1
    for j, g in enumerate(games):
        assert g["plies"] == len(g["moves"]) <= max_plies and g["plies"] >= 1, g
        if g["outcome"] == "converted":
            assert g["plies"] % 2 == 1 and last[j][1] == -1 and last[j][0] > 0, g
        elif g["outcome"] == "dropped":
            assert g["plies"] % 2 == 1 and last[j][0] <= 0, g
        elif g["outcome"] == "repeated":
            assert g["plies"] % 2 == 0 and seen[j][-1] in seen[j][:-1] and len(set(seen[j][:-1])) == len(seen[j]) - 1, g
        else:       # still won: after the mover's ply its move kept the win and the defender has a move; after the defender's
            assert g["outcome"] == "unfinished" and g["plies"] == max_plies, g
            assert (last[j][0] > 0 and last[j][1] != -1) if g["plies"] % 2 == 1 else last[j][1] > 0, g
            assert len(set(seen[j])) == len(seen[j]), g


@pytest.mark.parametrize("signature", ["R", "CA"])
def test_the_tables_own_moves_convert_in_the_distance(signature):
    from xiangqi_alphazero_amd import endgame
    tb = _tb(signature)
    boards, sides, index = tb.entries_of(("win",), 64, seed=13)
    out = endgame.play_out_with(_best(tb), tb, boards, sides, 64)
    _check_games(tb, boards, sides, out, 64)
    assert out["converted"] == 64 and out["conversion_rate"] == 1.0 and out["conversion_se"] == 0.0 and out["mean_plies_ratio"] == 1.0
    assert [g["plies"] for g in out["games"]] == [g["distance"] for g in out["games"]] == tb.table[index].tolist()
    if signature == "CA":
        assert max(g["plies"] for g in out["games"]) > 3        # longer than any rook ending
    # max_plies = 1: what one move does not convert is unfinished
    short = endgame.play_out_with(_best(tb), tb, boards, sides, 1)
    _check_games(tb, boards, sides, short, 1)
    assert [g["outcome"] for g in short["games"]] == ["converted" if v == 1 else "unfinished" for v in tb.table[index].tolist()]
    assert short["unfinished"] > 0 and short["dropped"] == short["repeated"] == 0
    # refused: a drawn and a lost position
    from xiangqi_alphazero_amd import hip
    for kind in ("draw", "loss"):
        b, s, _ = tb.entries_of((kind,), 2, seed=1)
        with pytest.raises(hip.XqError, match="drawn or lost"):
            endgame.play_out_with(_best(tb), tb, np.concatenate([boards[:2], b]), np.concatenate([sides[:2], s]), 8)
    d = golden_io.corpus()
    with pytest.raises(hip.XqError, match="not valid entries"):
        endgame.play_out_with(_best(tb), tb, d["board"][:2], d["side"][:2], 8)


def test_the_worst_move_drops_the_win_where_there_is_one_to_drop():
    from xiangqi_alphazero_amd import endgame, hip
    tb = _tb("R")
    pm = PM.play_model("R")
    boards, sides, index = tb.entries_of(("win",), 64, seed=17)

    def worst(games):
        p = tb.probe(np.stack([g.board for g in games]), [g.current_player for g in games])
        live = np.arange(hip.MAXM)[None, :] < p["counts"].astype(np.int64)[:, None]
        return p["moves"][np.arange(len(games)), np.where(live, p["move_value"].astype(np.int64), 1 << 14).argmin(axis=1)]

    out = endgame.play_out_with(worst, tb, boards, sides, 40)
    _check_games(tb, boards, sides, out, 40)
    can_drop = np.array([bool((pm.mv[e, :pm.m.counts[e]] <= 0).any()) for e in index.tolist()])
    got = np.array([g["outcome"] == "dropped" and g["plies"] == 1 for g in out["games"]])
    assert (got == can_drop).all() and can_drop.any()
    assert out["conversion_rate"] == out["converted"] / 64 and out["dropped"] >= int(can_drop.sum())


def test_a_shuttling_rook_repeats():
    from xiangqi_alphazero_amd import endgame
    tb = _tb("R")
    boards, sides, _ = tb.entries_of(("win",), 64, seed=19, side=1, min_plies=3)
    before = {}

    def shuttle(games):
        """The rook goes back where it came from whenever that keeps the win; else its first move that keeps the win; else the
        table's move."""
        p = tb.probe(np.stack([g.board for g in games]), [g.current_player for g in games])
        acts = []
        for k, g in enumerate(games):
            n = int(p["counts"][k])
            keeps = {int(a) for a, v in zip(p["moves"][k, :n], p["move_value"][k, :n]) if v > 0 and g.board[int(a) // 90] == 5}
            back = before.get(id(g))
            if back in keeps:
                a = back
            else:
                a = min(keeps) if keeps else int(p["best_action"][k])
            before[id(g)] = (a % 90) * 90 + a // 90
            acts.append(a)
        return acts

    out = endgame.play_out_with(shuttle, tb, boards, sides, 60)
    _check_games(tb, boards, sides, out, 60)
    assert out["repeated"] > 0 and out["dropped"] == 0
    for g in out["games"]:
        if g["outcome"] == "repeated":
            assert g["plies"] >= 4


def test_play_out_with_a_network():
    from xiangqi_alphazero_amd import endgame
    from xiangqi_alphazero_amd.model import XiangqiNet
    tb = _tb("R")
    boards, sides, _ = tb.entries_of(("win",), 32, seed=11)
    torch.manual_seed(5)
    net = XiangqiNet(64, 1).cuda().eval()          # the narrowest tower the product evaluator takes
    out = endgame.play_out(net, tb, boards, sides, 8, max_plies=12, seed=7)
    assert set(out) == (PLAYOUT - {"signature"}) | {"games"}
    assert out["positions"] == 32 and out["simulations"] == 8 and out["max_plies"] == 12 and out["seconds"] > 0
    assert out["conversion_rate"] == out["converted"] / 32
    _check_games(tb, boards, sides, out, 12)        # every move is legal, converted games end in an entry of value -1
    ratios = [g["plies"] / g["distance"] for g in out["games"] if g["outcome"] == "converted"]
    assert out["mean_plies_ratio"] == (float(np.mean(ratios)) if ratios else 0.0) and all(r >= 1.0 for r in ratios)
    # chunks smaller than the set give the same games
    again = endgame.play_out(net, tb, boards, sides, 8, max_plies=12, seed=7, chunk=5)
    assert again["games"] == out["games"]


# ---- the loop ----------------------------------------------------------------------------------------------------------------
def test_loop_plays_out_and_teaches(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    cfg = _config(tmp_path / "ck", endgame_signature="R", endgame_positions=16, endgame_simulations=4, endgame_playout_positions=8,
                  endgame_playout_max_plies=8, endgame_teacher_samples=16)
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    assert loop.endgame_playout == dict(positions=8, max_plies=8) and loop.endgame_teacher == dict(samples=16, policy=0)
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    assert [s["iteration"] for s in stats] == [1, 2] and len(saved) == 2
    records = 0
    for entry, on_disk in zip(stats, saved):
        assert set(entry) == PLAIN | {"endgame", "endgame_playout"} == set(on_disk)
        assert set(on_disk["endgame"]) == ENTRY
        p = on_disk["endgame_playout"]
        assert set(p) == PLAYOUT and p["signature"] == "R" and p["positions"] == 8 and p["simulations"] == 4 and p["max_plies"] == 8
        assert p["converted"] + p["dropped"] + p["repeated"] + p["unfinished"] == 8 and p["conversion_rate"] == p["converted"] / 8
        assert p["seconds"] > 0 and p == entry["endgame_playout"]
        sp = on_disk["self_play"]
        assert sp["endgame_teacher_samples"] == 16
        # the buffer grew by self-play's records and 16 more (buffer_size and new_samples count a record and its mirror)
        records += sp["new_samples"] // 2 + 16
        assert sp["buffer_size"] == 2 * records
    # the last 16 records of the buffer are the table's: entries_of seeded by seed + iteration, no rank term
    tb = loop._endgame_table()
    want = tb.samples(tb.entries_of(n=16, seed=3 + 2)[2])
    assert loop.buffer.store[records - 16:records].cpu().numpy().tobytes() == want.tobytes()


def test_loop_without_the_new_keys_keeps_its_form(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    cfg = _config(tmp_path / "a", endgame_signature="R", endgame_positions=16, endgame_simulations=4)
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    assert loop.endgame_playout is None and loop.endgame_teacher is None
    stats = loop.train()
    for entry in stats:
        assert set(entry) == PLAIN | {"endgame"} and set(entry["endgame"]) == ENTRY
        assert not any(k.startswith("endgame") for k in entry["self_play"])
    # the yardstick's interval holds for the play-out too
    cfg = _config(tmp_path / "b", endgame_signature="R", endgame_positions=16, endgame_simulations=4, endgame_interval=2,
                  endgame_playout_positions=4, endgame_playout_max_plies=4)
    stats = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3).train()
    assert set(stats[0]) == PLAIN and set(stats[1]) == PLAIN | {"endgame", "endgame_playout"}
    assert not any(k.startswith("endgame") for s in stats for k in s["self_play"])
