"""The start-position pool on the GPU (csrc/xq_positions.hip, k_start_pool of csrc/xq_engine.hip, xq_engine_init_sp).

1. `positions_check` equals tests/start_pool_model.py on the corpus, on the crafted boards and on the crafted bad boards, n = 1
   included;
2. a pool that holds only the initial position, at prob = 1 and random_opening_moves = 0, gives the samples, results and
   statistics of a plain engine byte for byte -- K = 1, leaves_per_step = 4, tree reuse, and steps replayed from a HIP graph: the
   new kernel's flush and new-game copy against k_select's own;
3. two slots with injected draws and a pool of a midgame position with black to move and a K+R against K ending: the games
   equal `play_game_from` on the entry `index_of` names, and `start_indices()` agrees while they run;
4. prob = 0.5: `index_of` says for every finished game whether it started from the pool, its ply-0 sample holds that entry's
   board and side or the initial position, and `pool_games` counts the pool games;
5. a pool of one position without a legal move finishes its games at ply 0 with no sample;
6. `start_pool=None` is the engine built without the argument;
7. a pool with a fatal entry is refused, by row in Python and with XQ_ERR_ARG by xq_engine_init_sp;
8. `run_games(start_pool=...)` returns samples the batch kernel accepts;
9. a pool drawn by `from_table` from "R" yields samples `endgame.rescore_samples` covers; `from_records` draws positions of
   recorded games.
"""
import ctypes as C
import types
from functools import lru_cache

import numpy as np
import pytest

import golden_io as G
import start_pool_model as SP
from oracle import xq_oracle as O
from test_playout_cap_gpu import _assert_game, _inject_array, _play_stub
from test_start_pool_model import bad_boards, kr_k
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

INIT = O.initial_board().reshape(90).astype(np.int8)


def _check(boards, sides):
    import torch
    from xiangqi_alphazero_amd import hip
    b = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 90)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(sides, dtype=np.int8)).cuda()
    out = hip.positions_check(b, s)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(b),)
    return out.cpu().numpy()


@lru_cache(maxsize=None)
def _corpus_status():
    """The model's status of every corpus position, computed once and shared."""
    c = G.corpus()
    st = np.array([SP.check_position(c["board"][i], c["side"][i]) for i in range(len(c["board"]))], dtype=np.uint8)
    st.setflags(write=False)
    return st


def _midgame(side, count=1, first=0):
    """`count` corpus positions with `side` to move, between plies 16 and 60, neither over nor without a move."""
    c = G.corpus()
    ok = np.nonzero((c["side"] == side) & (c["ply"] >= 16) & (c["ply"] <= 60) & (c["done"] == 0) & (_corpus_status() == 0))[0]
    pick = ok[first::max(1, len(ok) // (count + 1))][:count]
    assert len(pick) == count
    return c["board"][pick].astype(np.int8)


# ---- 1. the check kernel --------------------------------------------------------------------------------------------------------
def test_positions_check_equals_the_model_on_the_corpus():
    c = G.corpus()
    got = _check(c["board"], c["side"])
    assert (got == _corpus_status()).all() and set(np.unique(got).tolist()) == {0, 16}
    # the other side to move on every seventh board: the side that just moved is often in check there, which sets bit 8
    sub = np.arange(0, len(got), 7)
    flipped = [SP.check_position(c["board"][i], -c["side"][i]) for i in sub]
    assert _check(c["board"][sub], -c["side"][sub]).tolist() == flipped and any(f & 8 for f in flipped)


def test_positions_check_equals_the_model_on_crafted_and_bad_boards():
    from xiangqi_alphazero_amd import hip
    c = G.crafted()
    want = [SP.check_position(c["board"][i], c["side"][i]) for i in range(len(c["board"]))]
    assert _check(c["board"], c["side"]).tolist() == want and len(set(want)) >= 6
    bad = bad_boards()
    names = sorted(bad)
    got = _check(np.stack([bad[k][0] for k in names]), [bad[k][1] for k in names])
    assert got.tolist() == [bad[k][2] for k in names] == [SP.check_position(bad[k][0], bad[k][1]) for k in names]
    assert all(int(g) & hip.POSITION_FATAL for g in got)
    for k in names:                                        # n = 1
        assert _check(bad[k][0][None], [bad[k][1]]).tolist() == [bad[k][2]]
    assert _check(INIT[None], [1]).tolist() == [0] and _check(kr_k()[0][None], [1]).tolist() == [0]
    assert _check(np.zeros((0, 90), dtype=np.int8), np.zeros(0, dtype=np.int8)).tolist() == []
    with pytest.raises(hip.XqError, match="positions_check"):
        import torch
        hip.positions_check(torch.zeros((2, 90), dtype=torch.int8).cuda(), torch.zeros(3, dtype=torch.int8).cuda())


# ---- 2. equivalence with the existing path --------------------------------------------------------------------------------------
def _run(eng, n_games, graph=False):
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while True:
        eng.step()
        if eng.steps % 16 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 20000, "games did not finish"
    st = eng.stats()
    assert st["overflow"] == 0
    return st


def _sorted_drain(eng):
    smp, res = eng.drain()
    return np.sort(smp, order=["slot", "game_seq", "ply"]), np.sort(res, order=["slot", "game_seq"])


@pytest.mark.parametrize("kw,graph", [({}, False), (dict(leaves_per_step=4), False), (dict(tree_reuse=True), False), ({}, True),
                                      (dict(solver=True), False), (dict(gumbel=(8, 50.0, 1.0)), False)],
                         ids=["sequential", "leaves4", "tree_reuse", "graph", "solver", "gumbel"])
def test_initial_position_pool_is_the_plain_engine(kw, graph):
    """solver and gumbel: the pool's tail of the option words sits behind the solver's counters or the Gumbel words."""
    from xiangqi_alphazero_amd import engine
    ev = _TorchStub()
    n_games, out = 6, []
    for pool in (None, (INIT[None], np.ones(1, dtype=np.int8), 1.0)):
        cfg = engine.make_config(3, 12, seed=7, games_target=n_games, max_game_length=24, random_opening_moves=0)
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, start_pool=pool, **kw)
        assert eng.start_pool == (None if pool is None else (1, 1.0))
        st = _run(eng, n_games, graph=graph)
        out.append((st,) + _sorted_drain(eng))
        if pool is not None:
            assert eng.start_pool_stats() == dict(pool_games=n_games) and eng.start_indices().tolist() == [0, 0, 0]
    (st0, smp0, res0), (st1, smp1, res1) = out
    assert st0 == st1 and st0["games_finished"] == st0["games_started"] == n_games and len(smp0) > 0
    assert smp0.tobytes() == smp1.tobytes() and res0.tobytes() == res1.tobytes()
    assert len(res0) == n_games and int(res0["n_samples"].sum()) == len(smp0)


# ---- 3. against the model -------------------------------------------------------------------------------------------------------
def test_pool_games_equal_the_host_model():
    from xiangqi_alphazero_amd import engine, start_pool
    c = dict(num_simulations=16, c_puct=1.5, temperature_threshold=4, max_game_length=24, random_opening_moves=3,
             enable_resign=True, resign_threshold=-0.3, resign_check_steps=3)
    pool_b = np.stack([_midgame(-1)[0], kr_k()[0]])
    pool_s = np.array([-1, 1], dtype=np.int8)
    seed = next(s for s in range(1, 64) if sorted(start_pool.index_of(s, 0, k, 1, 2, 1.0) for k in (0, 1)) == [0, 1])
    draw_seeds, inj_len = [21, 22], 8192
    cfg = engine.make_config(2, c["num_simulations"], c_puct=c["c_puct"], temperature_threshold=c["temperature_threshold"],
                             max_game_length=c["max_game_length"], random_opening_moves=c["random_opening_moves"],
                             enable_resign=c["enable_resign"], resign_threshold=c["resign_threshold"],
                             resign_check_steps=c["resign_check_steps"], add_noise=True, inject_len=inj_len, games_target=2, seed=seed)
    eng = engine.SelfPlayEngine(cfg, inject=_inject_array(draw_seeds, inj_len), start_pool=(pool_b, pool_s, 1.0))
    entries = [start_pool.index_of(seed, 0, k, 1, 2, 1.0) for k in (0, 1)]
    assert eng.start_indices().tolist() == [-1, -1]
    from test_tree_reuse_gpu import _stub_step
    cache = {}
    for _ in range(3):
        _stub_step(eng, True, cache)
    assert eng.start_indices().tolist() == entries         # while the games run
    st = _play_stub(eng, True, 2)
    samples, results = eng.drain()
    assert len(results) == 2 and st["games_started"] == 2 and eng.start_pool_stats() == dict(pool_games=2)
    for slot in (0, 1):
        e = entries[slot]
        want, winner, plies = SP.play_game_from(c, True, draw_seeds[slot], pool_b[e], int(pool_s[e]))
        r = results[results["slot"] == slot]
        assert len(r) == 1 and (int(r[0]["winner"]), int(r[0]["steps"]), int(r[0]["n_samples"])) == (winner, plies, len(want))
        mine = samples[samples["slot"] == slot]
        _assert_game(mine, want)
        assert sorted(mine["ply"].tolist()) == list(range(len(want))) and len(want) > 0       # plies count from the pool position


# ---- 4. prob = 0.5 --------------------------------------------------------------------------------------------------------------
def test_half_of_the_games_start_from_the_pool():
    from xiangqi_alphazero_amd import engine, start_pool
    n_games, seed, prob = 8, 3, 0.5
    pool_b = np.concatenate([_midgame(-1, 3), _midgame(1, 2)])
    pool_s = np.array([-1, -1, -1, 1, 1], dtype=np.int8)
    cfg = engine.make_config(4, 8, seed=seed, games_target=n_games, max_game_length=24, random_opening_moves=0)
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), start_pool=(pool_b, pool_s, prob))
    _run(eng, n_games)
    samples, results = eng.drain()
    assert len(results) == n_games and sorted(zip(results["slot"].tolist(), results["game_seq"].tolist())) == \
        [(s, g) for s in range(4) for g in (1, 2)]
    from_pool = 0
    for r in results:
        e = start_pool.index_of(seed, 0, int(r["slot"]), int(r["game_seq"]), len(pool_b), prob)
        first = samples[(samples["slot"] == r["slot"]) & (samples["game_seq"] == r["game_seq"]) & (samples["ply"] == 0)]
        assert len(first) == 1
        board, side = (INIT, 1) if e < 0 else (pool_b[e], int(pool_s[e]))
        assert bytes(first[0]["board"].view(np.int8)) == bytes(board) and int(first[0]["side"]) == side, (int(r["slot"]), e)
        from_pool += e >= 0
    assert 0 < from_pool < n_games and eng.start_pool_stats() == dict(pool_games=from_pool)


# ---- 5. terminal entries --------------------------------------------------------------------------------------------------------
def test_entries_without_a_legal_move_finish_at_ply_zero():
    from xiangqi_alphazero_amd import engine
    c = G.corpus()
    i = int(np.nonzero(_corpus_status() == 16)[0][0])
    n_games = 6
    cfg = engine.make_config(2, 8, seed=2, games_target=n_games, max_game_length=24)
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), start_pool=(c["board"][i][None], c["side"][i:i + 1], 1.0))
    st = _run(eng, n_games)
    samples, results = eng.drain()
    assert len(samples) == 0 and len(results) == n_games and st["samples_written"] == 0 and st["games_started"] == n_games
    assert not results["steps"].any() and not results["n_samples"].any() and (results["reason"] == 1).all()
    assert (results["winner"] == -int(c["side"][i])).all() and eng.start_pool_stats() == dict(pool_games=n_games)


# ---- 6. option off --------------------------------------------------------------------------------------------------------------
def test_none_is_the_engine_without_the_argument():
    from xiangqi_alphazero_amd import engine, hip
    out = []
    for kw in ({}, dict(start_pool=None)):
        cfg = engine.make_config(3, 8, seed=4, games_target=6, max_game_length=24)
        eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), **kw)
        assert eng.start_pool is None
        out.append((_run(eng, 6), eng.workspace_bytes) + _sorted_drain(eng))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2].tobytes() == out[1][2].tobytes() and out[0][3].tobytes() == out[1][3].tobytes() and len(out[0][2]) > 0
    for name in ("start_indices", "start_pool_stats"):
        with pytest.raises(hip.XqError, match="start_pool"):
            getattr(eng, name)()


# ---- 7. fatal entries -----------------------------------------------------------------------------------------------------------
def test_a_fatal_entry_refuses_the_engine():
    import torch
    from xiangqi_alphazero_amd import engine, hip
    bad = bad_boards()["side_not_to_move_in_check"]
    boards = np.stack([INIT, bad[0], kr_k()[0]])
    sides = np.array([1, bad[1], 1], dtype=np.int8)
    cfg = engine.make_config(2, 8, seed=1, games_target=2)
    with pytest.raises(hip.XqError, match=r"start_pool: row 1 .* bits 8"):
        engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), start_pool=(boards, sides, 0.5))
    # the C entry point refuses the same pool by itself: no unchecked board reaches a slot
    lib = hip.lib()
    db, ds = torch.from_numpy(boards).cuda(), torch.from_numpy(sides).cuda()
    pool = hip.StartPool(db.data_ptr(), ds.data_ptr(), 3, 0, 0.5)
    nbytes = lib.xq_engine_workspace_bytes_sp(C.byref(cfg), 1, 0, *([None] * 9), C.byref(pool))
    assert nbytes > 0
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    h = hip.Engine()
    args = (C.byref(h), C.byref(cfg), 1, 0, *([None] * 9))
    tail = ((ws.data_ptr() + 255) & ~255, nbytes, None, hip.stream_ptr("cuda"))
    assert lib.xq_engine_init_sp(*args, C.byref(pool), *tail) == -1 and h.pad0 == 0
    good = hip.StartPool(db.data_ptr(), ds.data_ptr(), 1, 0, 0.5)              # its first row alone is fine
    assert lib.xq_engine_workspace_bytes_sp(C.byref(cfg), 1, 0, *([None] * 9), C.byref(good)) <= nbytes
    assert lib.xq_engine_init_sp(*args, C.byref(good), *tail) == 0 and h.pad0 & (1 << 22)
    torch.cuda.synchronize()


# ---- 8. run_games ---------------------------------------------------------------------------------------------------------------
def _config(**kw):
    return types.SimpleNamespace(**{**dict(num_simulations=8, c_puct=1.5, temperature_threshold=6, max_game_length=16,
                                           random_opening_moves=2, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5),
                                    **kw})


def test_run_games_samples_are_trainable():
    import torch
    from xiangqi_alphazero_amd import selfplay, training
    net, _ = _hip_evaluator()
    pool_b = np.concatenate([_midgame(-1, 2), kr_k()[0][None]])
    pool_s = np.array([-1, -1, 1], dtype=np.int8)
    samples, results, st, _ = selfplay.run_games(net, _config(), 6, n_slots=3, seed=2, start_pool=(pool_b, pool_s, 1.0))
    assert st["start_pool"] == (3, 1.0) and st["start_pool_games"] == 6 == len(results) and st["overflow"] == 0 and len(samples) > 0
    first = samples[samples["ply"] == 0]
    pool_keys = {bytes(b) + bytes([int(s) & 0xFF]) for b, s in zip(pool_b, pool_s)}
    assert len(first) == 6 and all(bytes(f["board"].view(np.int8)) + bytes([int(f["side"]) & 0xFF]) in pool_keys for f in first)
    buf = training.ReplayBuffer(4096, "cuda")
    buf.extend(samples)
    states, pi, z = buf.batch(torch.arange(len(buf), device="cuda"))
    assert len(buf) == 2 * len(samples) and torch.isfinite(pi).all() and torch.isfinite(states).all()
    assert torch.allclose(pi.sum(1), torch.ones(len(buf), device="cuda"), atol=1e-5) and set(z.unique().tolist()) <= {-1.0, 0.0, 1.0}
    _, _, off, _ = selfplay.run_games(net, _config(), 3, n_slots=3, seed=2)
    assert (off["start_pool"], off["start_pool_games"]) == (None, 0)


# ---- 9. the sources that need the device ----------------------------------------------------------------------------------------
def test_table_pool_samples_are_covered_by_the_table():
    from xiangqi_alphazero_amd import endgame, engine, start_pool
    tb = endgame.Tablebase.generate("R", "cuda")
    boards, sides = start_pool.from_table(tb, 16, ("win",), seed=5, min_plies=3)
    assert boards.shape == (16, 90) and boards.dtype == np.int8 and sides.dtype == np.int8
    assert ((boards != 0).sum(axis=1) == 3).all() and _check(boards, sides).tolist() == [0] * 16
    again = start_pool.from_table(tb, 16, ("win",), seed=5, min_plies=3)
    assert again[0].tobytes() == boards.tobytes() and start_pool.from_table(tb, 16, ("win",), seed=6)[0].tobytes() != boards.tobytes()
    n_games = 6
    cfg = engine.make_config(3, 8, seed=9, games_target=n_games, max_game_length=12)
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), start_pool=(boards, sides, 1.0))
    _run(eng, n_games)
    samples, results = eng.drain()
    assert len(results) == n_games and len(samples) > 0
    three = int(((samples["board"] != 0).sum(axis=1) == 3).sum())
    _, covered, _ = endgame.rescore_samples(samples, tb)
    assert covered == three > 0 and (samples[samples["ply"] == 0]["board"] != 0).sum(axis=1).tolist() == [3] * n_games


def test_loop_plays_from_the_file_and_the_table(tmp_path):
    """One iteration of the loop with both sources at prob = 1: every game is a pool game, the pool is the file's positions and
    the table's entries, and the self-play entry of training_stats.json says so; without the keys the entry has neither word."""
    import json
    from test_baseline_loop_gpu import PLAIN, _config as loop_config
    from xiangqi_alphazero_amd import train_loop
    from xiangqi_alphazero_amd.sample_format import board_to_fen
    path = tmp_path / "start.txt"
    path.write_text("# midgame\n" + "\n".join(board_to_fen(b, -1) for b in _midgame(-1, 2)) + "\n")
    cfg = loop_config(tmp_path / "ck", endgame_signature="R", endgame_interval=99, start_positions_file=str(path),
                      start_positions_endgame=6, start_positions_prob=1.0)
    cfg.num_iterations, cfg.num_games_per_iter = 1, 8
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    assert loop.start_pool["endgame"] == 6 and len(loop.start_pool["boards"]) == 2
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    assert len(stats) == len(saved) == 1 and set(saved[0]) == PLAIN
    sp = saved[0]["self_play"]
    assert sp["start_pool_positions"] == 8 and sp["start_pool_games"] == sp["games"] == 8
    plain = loop_config(tmp_path / "b")
    plain.num_iterations, plain.num_games_per_iter = 1, 8
    off = train_loop.AlphaZeroLoop(plain, "cuda", seed=3)
    assert off.start_pool is None
    assert not any(k.startswith("start_pool") for k in off.train()[0]["self_play"])


def test_from_records_draws_positions_of_recorded_games():
    from xiangqi_alphazero_amd import engine, start_pool
    cfg = engine.make_config(3, 8, seed=4, games_target=6, max_game_length=24)
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), record_games=True)
    _run(eng, 6)
    records = eng.drain_games()
    boards, sides = start_pool.from_records(records, 12, seed=1, min_ply=4, max_ply=20)
    assert boards.shape[1] == 90 and 0 < len(boards) <= 12 and len(sides) == len(boards)
    assert not (_check(boards, sides) & 15).any()
    again = start_pool.from_records(records, 12, seed=1, min_ply=4, max_ply=20)
    assert again[0].tobytes() == boards.tobytes() and again[1].tobytes() == sides.tobytes()
    # every position is the record's own at some ply in the range
    out = engine.replay_games(np.repeat(records, 17), stop_ply=np.tile(np.arange(4, 21, dtype=np.int32), len(records)))
    reach = {bytes(b) for b in out["board"].cpu().numpy()}
    assert all(bytes(b) in reach for b in boards)
    assert len(start_pool.from_records(records, 5, min_ply=300, max_ply=400)[0]) == 0          # no record is that long
