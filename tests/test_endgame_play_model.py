"""The CPU model of the table as opponent and teacher (tests/endgame_play_model.py) against itself: the table-against-table walk
takes exactly the table's distance with the values the header states, `play` agrees with the layout, and `sample_rows` is
consistent with `Model.probe`.  The GPU suite then holds xq_tb_play_batch and xq_tb_samples to this model exactly."""
import numpy as np
import pytest

import endgame_model as EM
import endgame_play_model as PM
from xiangqi_alphazero_amd import endgame

SIGNATURES = ["R", "C", "Ra"]


@pytest.mark.parametrize("signature", SIGNATURES)
def test_the_walk_takes_the_tables_distance(signature):
    pm = PM.play_model(signature)
    m = pm.m
    won = np.nonzero(m.table > 0)[0]
    p = m.table[won].astype(np.int64)
    plies, values = pm.walk_all(won)
    assert (plies == p).all()
    assert len(values) == (int(p.max()) if len(p) else 0) + 1
    # +p, -p, +(p - 2), -(p - 2), ..., +1, -1, then the game stands still at -1
    for k, v in enumerate(values):
        want = np.where(k >= p, -1, np.where(k % 2 == 0, p - k, -(p - k + 1)))
        assert (v == want).all(), (signature, k)
    # the last entry has no move, and lost entries take their distance too
    lost = np.nonzero((m.table < 0) & (m.table != EM.INVALID))[0]
    plies, values = pm.walk_all(lost)
    assert (plies == -m.table[lost].astype(np.int64) - 1).all() and (values[-1] == -1).all()
    if signature == "Ra":
        assert int(p.max()) == 9
    if signature == "C":
        assert len(won) == 0 and len(lost) == 0         # a lone cannon wins nothing: every valid entry is a draw


@pytest.mark.parametrize("signature", SIGNATURES)
def test_play_agrees_with_the_layout_and_the_single_walk(signature):
    pm = PM.play_model(signature)
    m = pm.m
    rng = np.random.default_rng(11)
    rows = np.sort(rng.choice(m.entries, size=600, replace=False))
    r = pm.play(rows)
    t = m.table[rows].astype(np.int64)
    assert ((r["status"] == 4) == (t == EM.INVALID)).all() and ((r["status"] == 8) == ((t != EM.INVALID) & (m.counts[rows] == 0))).all()
    assert set(np.unique(r["status"]).tolist()) <= {0, 4, 8}
    ok = r["status"] == 0
    assert (r["child"][ok] == pm.best_child[rows[ok]]).all() and (r["child"][~ok] == -1).all()
    # the board after the move is the child entry's board, and its index is the child's
    assert (r["boards"][ok] == m.boards[r["child"][ok]]).all() and (r["side"][ok] == m.sides[r["child"][ok]]).all()
    assert (endgame.board_to_index(signature, r["boards"][ok], r["side"][ok]) == r["child"][ok]).all()
    assert (r["boards"][~ok] == m.boards[rows[~ok]]).all() and (r["side"][~ok] == m.sides[rows[~ok]]).all()
    assert (r["played"][~ok] == EM.NO_MOVE).all() and (r["move_value"][~ok] == 0).all() and (r["value_out"][~ok] == 0).all()
    assert (r["value"][r["status"] == 8] == -1).all() and (r["value"][r["status"] == 4] == 0).all()
    # the table's own move keeps the value: the probe's relation between a child's word and the move's value
    assert (r["move_value"][ok] == r["value"][ok]).all() and (r["played"][ok] == m.probe(rows[ok])["best_action"]).all()
    c = r["value_out"][ok]
    assert (r["move_value"][ok] == np.where(c < 0, -c, np.where(c > 0, -(c + 2), 0))).all()
    # a given action: every legal move plays, anything else is status 16
    e = int(rows[ok][0])
    k = int(m.counts[e])
    every = pm.play([e] * k, m.moves[e, :k])
    assert (every["status"] == 0).all() and (every["child"] == m.children[e, :k]).all() and (every["move_value"] == pm.mv[e, :k]).all()
    assert pm.play([e], [0])["status"][0] == 16 and pm.play([e], [0])["value"][0] == m.table[e]
    # the single walk is the vectorised one
    decided = rows[ok & (t != 0)][:5]
    for e in decided.tolist():
        path = pm.walk(e)
        plies, values = pm.walk_all([e])
        assert len(path) - 1 == plies[0] and [v for _, v in path] == [int(v[0]) for v in values]


@pytest.mark.parametrize("signature", SIGNATURES)
@pytest.mark.parametrize("policy", [0, 1])
def test_sample_rows_are_consistent(signature, policy):
    pm = PM.play_model(signature)
    m = pm.m
    rng = np.random.default_rng(5)
    rows = np.concatenate([[-1, m.entries], np.sort(rng.choice(m.entries, size=800, replace=False))])
    out, status = pm.sample_rows(rows, policy)
    assert status[:2].tolist() == [1, 1]
    inner = rows[2:]
    t = m.table[inner].astype(np.int64)
    assert (status[2:] == np.where(t == EM.INVALID, 4, np.where(m.counts[inner] == 0, 8, 0))).all()
    assert out[status != 0].tobytes() == bytes(640 * int((status != 0).sum()))
    ok = np.nonzero(status == 0)[0]
    probe = m.probe(rows[ok])
    s = out[ok]
    assert (s["z"] == np.sign(probe["value"])).all() and (s["n_moves"] == probe["counts"]).all() and (s["actions"] == probe["moves"]).all()
    assert (s["board"] == m.boards[rows[ok]]).all() and (s["side"] == m.sides[rows[ok]]).all() and (s["game_seq"] == rows[ok]).all()
    for name in ("ply", "late_temp", "reserved0", "reserved1", "slot", "pad"):
        assert not s[name].any(), name
    live = np.arange(EM.MAXM)[None, :] < probe["counts"][:, None]
    optimal = live & (probe["move_value"] == probe["value"][:, None])
    assert set(np.unique(s["visits"]).tolist()) == {0, 1} and optimal.any(axis=1).all()
    if policy == 0:
        assert ((s["visits"] != 0) == optimal).all()
    else:
        assert (s["visits"].sum(axis=1) == 1).all()
        assert (s["actions"][np.arange(len(ok)), s["visits"].argmax(axis=1)] == probe["best_action"]).all()
