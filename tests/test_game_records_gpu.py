"""Game records (xq_engine_init_gr) and their device replay (xq_replay_games_batch) on the GPU.

1. whole games with injected draws and the stub evaluator: the drained record equals tests/game_record_model.py -- moves,
   opening_plies, winner, reason, n_samples; n_moves is the result's steps; the entries past n_moves are 0;
2. records change nothing: the same configuration and seed with the option off and on give byte-identical samples, results and
   statistics, on the K = 1 kernel and with leaves_per_step = 4;
3. self-consistency through the replay kernel, no host model: every record of a tiny run of each option replays legally to
   n_moves plies, the rules' verdict there fits the record's reason, and every drained sample's board and side are its game's
   position at the sample's ply;
4. the replay against the oracle: board, side, move_count, no_capture and hist12 at several stop plies; an illegal action at the
   first, a middle and the last ply; a malformed record; n = 1 and a record without moves;
5. the ring's edges: a full ring drops and counts, a drain into a buffer that is too small consumes nothing, a drained ring
   starts again at row 0 and a row never shows an earlier game's tail;
6. steps replayed from a HIP graph give the records of eager steps;
7. run_games and the arena's entry points return records that pass 3's conditions; off, the new statistics are there and empty.
"""
import ctypes as C
import types

import numpy as np
import pytest

import game_record_model as GR
import golden_io as G
from oracle import xq_oracle as O
from test_playout_cap_gpu import _engine_cfg, _inject_array, _play_stub
from test_tree_reuse_gpu import _TorchStub, _hip_evaluator

pytestmark = pytest.mark.gpu

TRACES = G.game_traces()
NAMES = [t["name"] for t in TRACES]
REASON = dict(resign=3, maxlen=2, natural=1, resign_late=3)       # how each recorded game ends
_played = {}


def _gpu_game(name):
    """Two slots play recorded game `name` on its injected draws with game records on -> (records by slot, samples, results,
    stats); played once, shared, never modified."""
    from xiangqi_alphazero_amd import engine
    if name not in _played:
        t = TRACES[NAMES.index(name)]
        inj_len = 16384
        eng = engine.SelfPlayEngine(_engine_cfg(engine, t["cfg"], 2, inj_len, 2), inject=_inject_array([t["seed"]] * 2, inj_len),
                                    record_games=True)
        assert eng.record_games and eng.max_out_games == eng.cfg.max_out_results
        st = _play_stub(eng, t["stub"] == "peaked", 2)
        records = eng.drain_games()
        samples, results = eng.drain()
        records = records[np.argsort(records["slot"])]
        for a in (records, samples, results):
            a.setflags(write=False)
        _played[name] = (records, samples, results, st, eng.game_records_stats())
    return _played[name]


# ---- 1. against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_records_equal_host_model(name):
    from xiangqi_alphazero_amd import hip
    t = TRACES[NAMES.index(name)]
    want = GR.expected_record(t["cfg"], t["stub"] == "peaked", t["seed"])
    records, samples, results, st, gst = _gpu_game(name)
    assert records.dtype == hip.GAME_RECORD_DTYPE and len(records) == len(results) == 2 and gst == dict(recorded=2, dropped=0)
    for r in records:
        res = results[(results["slot"] == r["slot"]) & (results["game_seq"] == r["game_seq"])]
        assert len(res) == 1 and int(r["n_moves"]) == int(res[0]["steps"]) == want["n_moves"]
        n = int(r["n_moves"])
        assert list(r["moves"][:n]) == want["moves"]
        assert not r["moves"][n:].any()
        assert int(r["opening_plies"]) == want["opening_plies"]
        assert (int(r["winner"]), int(r["n_samples"])) == (want["winner"], want["n_samples"]) == \
            (int(res[0]["winner"]), int(res[0]["n_samples"]))
        assert int(r["reason"]) == int(res[0]["reason"]) == REASON[name]
        assert int(r["game_seq"]) == 1
    assert sorted(records["slot"]) == [0, 1] and st["overflow"] == 0


# ---- 2. records change nothing --------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("K", [1, 4], ids=["sequential", "leaves4"])
def test_records_change_nothing(K):
    from xiangqi_alphazero_amd import engine
    ev = _TorchStub()
    n_games, sims = 6, 12
    out = []
    for on in (False, True):
        cfg = engine.make_config(3, sims, seed=7, games_target=n_games, max_game_length=24)
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=K, record_games=on)
        assert eng.record_games == on
        st = _run(eng, n_games)
        out.append((st,) + _sorted_drain(eng))
        if on:
            rec = eng.drain_games()
            assert len(rec) == n_games and eng.game_records_stats() == dict(recorded=n_games, dropped=0)
    (st0, smp0, res0), (st1, smp1, res1) = out
    assert st0 == st1 and st0["games_finished"] == n_games and len(smp0) > 0
    assert smp0.tobytes() == smp1.tobytes() and res0.tobytes() == res1.tobytes()
    rec = np.sort(rec, order=["slot", "game_seq"])
    assert rec[["slot", "game_seq", "winner", "reason"]].tolist() == res1[["slot", "game_seq", "winner", "reason"]].tolist()
    assert rec["n_moves"].tolist() == res1["steps"].tolist() and rec["n_samples"].tolist() == res1["n_samples"].tolist()


# ---- 3. self-consistency through the replay kernel ------------------------------------------------------------------------------
def _check_records(records, max_game_length, perpetual=False, samples=None):
    """The conditions every run's records meet: legal to the last ply, a verdict that fits the reason, and the samples'
    positions."""
    from xiangqi_alphazero_amd import engine
    assert len(records) > 0
    out = {k: v.cpu().numpy() for k, v in engine.replay_games(records, perpetual_check=perpetual).items()}
    assert not out["status"].any()
    assert out["move_count"].tolist() == records["n_moves"].tolist()
    for r, kind, winner in zip(records, out["over_kind"], out["winner"]):
        n = int(r["n_moves"])
        assert not r["moves"][n:].any() and int(r["opening_plies"]) <= n
        reason = int(r["reason"])
        assert reason in (1, 2, 3, 4)
        if reason in (1, 4):
            assert int(kind) == reason and int(winner) == int(r["winner"])
        else:
            assert int(kind) == 0 and int(winner) == 2
            assert reason == 3 or n >= max_game_length
    if samples is None:
        return out
    assert len(samples) == int(records["n_samples"].sum())
    key = {(int(r["slot"]), int(r["game_seq"])): i for i, r in enumerate(records)}
    idx = np.array([key[(int(s["slot"]), int(s["game_seq"]))] for s in samples])
    at = engine.replay_games(records[idx], stop_ply=samples["ply"].astype(np.int32), perpetual_check=perpetual)
    assert not at["status"].any().item()
    assert at["move_count"].cpu().numpy().tolist() == samples["ply"].tolist()
    assert at["board"].cpu().numpy().tobytes() == np.ascontiguousarray(samples["board"]).tobytes()
    assert at["side"].cpu().numpy().tolist() == samples["side"].tolist()
    assert (samples["ply"] >= records["opening_plies"][idx]).all() and (samples["ply"] < records["n_moves"][idx]).all()
    return out


SELFPLAY_RUNS = [("plain", dict(sims=8, length=12), {}),
                 ("tree_reuse", dict(sims=12, length=20), dict(tree_reuse=True)),
                 ("playout_cap", dict(sims=16, length=24), dict(playout_cap=(0.5, 4))),
                 ("solver", dict(sims=12, length=40), dict(solver=True)),
                 ("gumbel", dict(sims=16, length=16), dict(gumbel=(8, 50.0, 1.0))),
                 ("perpetual_check", dict(sims=8, length=40), dict(perpetual_check=True)),
                 ("leaves4", dict(sims=12, length=20), dict(leaves_per_step=4))]


@pytest.mark.parametrize("name,shape,kw", SELFPLAY_RUNS, ids=[r[0] for r in SELFPLAY_RUNS])
def test_selfplay_records_replay(name, shape, kw):
    from xiangqi_alphazero_amd import engine
    n_games = 6
    cfg = engine.make_config(4, shape["sims"], seed=11, games_target=n_games, max_game_length=shape["length"])
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), record_games=True, **kw)
    _run(eng, n_games)
    records = eng.drain_games_device()
    assert records.is_cuda and tuple(records.shape) == (n_games, 1024)
    samples, results = eng.drain()
    from xiangqi_alphazero_amd import hip
    records = records.cpu().numpy().reshape(-1).view(hip.GAME_RECORD_DTYPE)
    assert sorted(zip(records["slot"].tolist(), records["game_seq"].tolist())) == \
        sorted(zip(results["slot"].tolist(), results["game_seq"].tolist()))
    _check_records(records, shape["length"], perpetual=kw.get("perpetual_check", False), samples=samples)
    searched = records["n_moves"].astype(int) - records["opening_plies"].astype(int)
    if name == "playout_cap":
        assert (records["n_samples"] < searched).any()          # fast moves are in the record and in no sample
    elif name != "solver":                                      # every searched move of these runs is a sample
        assert (records["n_samples"] == searched).all()
    assert eng.game_records_stats() == dict(recorded=n_games, dropped=0) and len(eng.drain_games()) == 0


@pytest.mark.parametrize("openings,solver", [(False, False), (True, False), (True, True)],
                         ids=["default", "paired_openings", "paired_openings_solver"])
def test_arena_records_replay(openings, solver):
    """paired_openings_solver is the fullest region of option words: arena words, solver counters and the records' tail."""
    from xiangqi_alphazero_amd import arena
    n_games, length = 4, 16
    info = {} if openings else None
    kw = dict(opening_plies=4, seed=3, info=info, solver=solver) if openings else {}
    results, records = arena.play_arena(_TorchStub(), _TorchStub(), n_games, 8, length, record_games=True, **kw)
    assert len(results) == len(records) == n_games and records["slot"].tolist() == list(range(n_games))
    assert records["n_moves"].tolist() == results["steps"].tolist() and records["winner"].tolist() == results["winner"].tolist()
    assert records["reason"].tolist() == results["reason"].tolist() and not records["n_samples"].any()
    _check_records(records, length)
    if not openings:
        assert not records["opening_plies"].any()
        return
    op, counts = np.asarray(info["openings"]), np.asarray(info["opening_counts"])
    assert records["opening_plies"].tolist() == counts.tolist() and counts.tolist() == [4] * n_games
    for g in range(n_games):
        assert records["moves"][g, :4].tolist() == op[g, :4].astype(np.uint16).tolist()
    for p in range(n_games // 2):
        assert records["moves"][2 * p, :4].tolist() == records["moves"][2 * p + 1, :4].tolist()


# ---- 4. the replay against the oracle -------------------------------------------------------------------------------------------
def _oracle_at(moves, ply):
    g = O.Game()
    for a in moves[:ply]:
        g.make_action(int(a))
    hist = np.zeros((12, 90), dtype=np.int8)
    h = g.history()[-12:]
    hist[:len(h)] = h
    return g.board.reshape(90).copy(), g.current_player, g.move_count, g.no_capture_count, hist


def _assert_position(out, i, moves, ply):
    board, side, mc, nocap, hist = _oracle_at(moves, ply)
    assert bytes(out["board"][i]) == bytes(board) and int(out["side"][i]) == side
    assert (int(out["move_count"][i]), int(out["no_capture"][i])) == (mc, nocap) and mc == ply
    assert out["hist12"][i].tobytes() == hist.tobytes()          # zeros outside the min(12, ply) valid entries included
    assert not out["hist12"][i][min(12, ply):].any()


@pytest.mark.parametrize("name", NAMES)
def test_replay_equals_oracle(name):
    from xiangqi_alphazero_amd import engine
    rec = _gpu_game(name)[0][:1]
    n = int(rec[0]["n_moves"])
    moves = rec[0]["moves"][:n].tolist()
    stops = [0, 1, 11, 12, 13, n, n + 7]
    batch = np.repeat(rec, len(stops))
    out = {k: v.cpu().numpy() for k, v in engine.replay_games(batch, stop_ply=stops).items()}
    assert not out["status"].any()
    for i, stop in enumerate(stops):
        _assert_position(out, i, moves, min(stop, n))
    full = {k: v.cpu().numpy() for k, v in engine.replay_games(rec).items()}       # n = 1, no stop plies: every move
    _assert_position(full, 0, moves, n)
    g = GR.replay_on_oracle(moves)
    over, w = g.is_game_over()
    assert (int(full["over_kind"][0]), int(full["winner"][0])) == ((1, w) if over else (0, 2))
    neg = engine.replay_games(rec, stop_ply=-3)                                   # clamps to 0: the initial position
    assert int(neg["move_count"][0].item()) == 0 and bytes(neg["board"][0].cpu().numpy()) == bytes(O.initial_board().reshape(90))


def test_replay_reports_illegal_plies_and_malformed_records():
    from xiangqi_alphazero_amd import engine, hip
    rec = _gpu_game("resign")[0][:1]
    n = int(rec[0]["n_moves"])
    moves = rec[0]["moves"][:n].tolist()
    bad = np.repeat(rec, 5).copy()
    mid = n // 2
    for i, k in enumerate((0, mid, n - 1)):
        bad["moves"][i, k] = 0                              # a0a0: no move of any position
    bad["moves"][3, mid] = moves[mid - 1]                   # the previous ply again: its piece has left the square
    bad["n_moves"][4] = 505
    out = {k: v.cpu().numpy() for k, v in engine.replay_games(bad).items()}
    assert out["status"].tolist() == [1, mid + 1, n, mid + 1, -1]
    for i, k in enumerate((0, mid, n - 1, mid)):
        _assert_position(out, i, moves, k)                  # the position before the refused ply
    _assert_position(out, 4, moves, 0)
    assert (int(out["over_kind"][4]), int(out["winner"][4])) == (0, 2)
    empty = np.zeros(1, dtype=hip.GAME_RECORD_DTYPE)        # a record without moves
    out = {k: v.cpu().numpy() for k, v in engine.replay_games(empty).items()}
    assert out["status"].tolist() == [0]
    _assert_position(out, 0, [], 0)
    none = engine.replay_games(empty[:0])                   # n = 0
    assert tuple(none["board"].shape) == (0, 90) and tuple(none["hist12"].shape) == (0, 12, 90)
    # every output but the status may be absent
    import torch
    status = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(rec.view(np.uint8).reshape(1, 1024).copy()).cuda()
    hip.check(hip.lib().xq_replay_games_batch(dev.data_ptr(), None, 1, 0, None, None, None, None, None, status.data_ptr(), None, None,
                                              hip.stream_ptr("cuda")), "xq_replay_games_batch")
    assert status.item() == 0


# ---- 5. the ring's edges --------------------------------------------------------------------------------------------------------
def _one_slot(max_out_games, n_games, sims=8, **cfg_kw):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(1, sims, seed=5, games_target=n_games, **{**dict(max_game_length=16), **cfg_kw})
    return engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), record_games=True, max_out_games=max_out_games)


def test_full_ring_drops_and_counts():
    big, small = _one_slot(8, 3), _one_slot(1, 3)
    st_big, st_small = _run(big, 3), _run(small, 3)
    assert st_big == st_small and st_small["overflow"] == 0 and st_small["games_finished"] == 3
    n = C.c_int()
    from xiangqi_alphazero_amd import hip
    buf = np.zeros(1, dtype=hip.GAME_RECORD_DTYPE)           # too small for the three pending records: nothing is consumed
    rc = big.lib.xq_engine_drain_games(C.byref(big.h), buf.ctypes.data, 1, C.byref(n), hip.stream_ptr(big.device))
    assert rc == -1 and n.value == 3 and not buf.view(np.uint8).any()
    rc = big.lib.xq_engine_drain_games(C.byref(big.h), None, 0, C.byref(n), hip.stream_ptr(big.device))    # the count alone
    assert rc == 0 and n.value == 3
    all_three = big.drain_games()
    assert all_three["game_seq"].tolist() == [1, 2, 3]       # one slot: the games finish in this order
    only = small.drain_games()
    assert len(only) == 1 and only.tobytes() == all_three[:1].tobytes()
    assert small.game_records_stats() == dict(recorded=1, dropped=2) and big.game_records_stats() == dict(recorded=3, dropped=0)
    for a, b in zip(_sorted_drain(big), _sorted_drain(small)):
        assert a.tobytes() == b.tobytes() and len(a) > 0
    assert len(small.drain_games()) == 0 and len(big.drain_games()) == 0 and len(small.drain_games_device()) == 0
    assert small.game_records_stats() == dict(recorded=1, dropped=2)
    with pytest.raises(hip.XqError, match="record_games"):
        from xiangqi_alphazero_amd import engine
        engine.SelfPlayEngine(engine.make_config(1, 8), evaluator=_TorchStub()).drain_games()


def test_drained_ring_restarts_at_row_zero_with_a_clean_tail():
    """One slot, one game at a time, a drain after each: every game lands at row 0.  The stub's values resign games at different
    lengths, so a shorter game follows a longer one; and once the row is filled with 0xFFFF by hand, which stands for the longest
    earlier game there can be."""
    n_games = 8
    eng = _one_slot(4, n_games, enable_resign=True, resign_threshold=0.0, resign_check_steps=1, max_game_length=40)
    ring = eng.game_record_views()["ring"]
    lengths = []
    for g in range(n_games):
        if g == 3:
            ring[0].fill_(-1)
        while eng.stats()["games_finished"] <= g:
            for _ in range(8):
                eng.step()
            assert eng.steps < 20000
        rec = eng.drain_games()
        assert len(rec) == 1 and int(rec[0]["game_seq"]) == g + 1
        n = int(rec[0]["n_moves"])
        assert n > 0 and rec[0]["moves"][:n].all() and not rec[0]["moves"][n:].any()
        row0 = ring[0].cpu().numpy().view(np.uint16)
        assert row0.tobytes() == rec.tobytes()
        lengths.append(n)
    assert any(b < a for a, b in zip(lengths, lengths[1:])), lengths
    assert eng.stats()["overflow"] == 0 and eng.game_records_stats() == dict(recorded=n_games, dropped=0)


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replayed_steps_give_the_same_records():
    from xiangqi_alphazero_amd import engine
    n_games, out = 8, []
    for graph in (False, True):
        cfg = engine.make_config(4, 8, seed=9, games_target=n_games, max_game_length=16)
        eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), record_games=True)
        _run(eng, n_games, graph=graph)
        out.append(np.sort(eng.drain_games(), order=["slot", "game_seq"]))
    assert len(out[0]) == n_games and out[0].tobytes() == out[1].tobytes()


# ---- 7. run_games and the arena -------------------------------------------------------------------------------------------------
def _config(**kw):
    return types.SimpleNamespace(**{**dict(num_simulations=8, c_puct=1.5, temperature_threshold=6, max_game_length=16,
                                           random_opening_moves=2, enable_resign=False, resign_threshold=-0.9, resign_check_steps=5,
                                           eval_games=4, eval_simulations=8, eval_win_rate=0.55), **kw})


def test_run_games_and_evaluate_models_return_records():
    from xiangqi_alphazero_amd import arena, hip, selfplay
    net, _ = _hip_evaluator()
    samples, results, st, _ = selfplay.run_games(net, _config(), 6, n_slots=3, seed=2, record_games=True)
    assert st["record_games"] is True and st["game_records_recorded"] == 6 and st["game_records_dropped"] == 0
    records = st["game_records"]
    assert records.dtype == hip.GAME_RECORD_DTYPE and len(records) == len(results) == 6
    _check_records(records, 16, samples=samples)
    _, _, off, _ = selfplay.run_games(net, _config(), 3, n_slots=3, seed=2)
    assert (off["record_games"], off["game_records"], off["game_records_recorded"], off["game_records_dropped"]) == (False, None, 0, 0)
    _, _, st, _ = selfplay.run_games(net, _config(record_games=True), 3, n_slots=3, seed=2, device_records=True)   # the config key
    assert st["record_games"] and st["game_records"].is_cuda and tuple(st["game_records"].shape) == (3, 1024)
    out = arena.evaluate_models(net, net, _config(), record_games=True)
    records = out["game_records"]
    assert len(records) == 4 and records["slot"].tolist() == [0, 1, 2, 3]
    assert records["n_moves"].tolist() == out["games"]["steps"].tolist() and records["winner"].tolist() == out["games"]["winner"].tolist()
    _check_records(records, 16)
    assert "game_records" not in arena.evaluate_models(net, net, _config())
