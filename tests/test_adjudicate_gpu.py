"""Table adjudication on the GPU (csrc/xq_adjudicate.hip: k_tb_adjudicate, k_adjudicate).

1. `hip.tb_adjudicate_batch` equals tests/adjudicate_model.py word for word -- status, winner, value -- over every entry of "Ra",
   the colour-swapped images, the boards of "Nb" and three off-table boards, with draws and both_colours on and off;
2. `hip.engine_adjudicate` in situ: a plain engine is stepped stage by stage for 40 steps, and after every select the model says
   from the slots' boards and state words what the kernel must write; every other word and byte stays, the counters are the
   model's running sums.  Self-play slots start from a pool (below); an arena engine cannot take a pool, so the arena case runs
   from the initial position, where no slot is covered, and asserts that nothing changes;
3. `SelfPlayEngine(adjudicate=...)` end to end on a pool of won "R" entries: reason 5 after one move (min_ply = 1) or at ply 0
   (min_ply = 0), the exact z, the counters, eager against replayed steps, two tables against one, None against no argument;
4. one iteration of the loop with config.adjudicate_signatures logs the three fields.
"""
from functools import lru_cache

import numpy as np
import pytest

import adjudicate_model as AM
import endgame_model as EM
from test_adjudicate_model import off_table_boards
from test_hip_engine import _stub_batch
from test_tree_reuse_gpu import _TorchStub

pytestmark = pytest.mark.gpu

G, S = 16, 8
SITU_SEED = 14         # chosen with hip.start_pool_index alone (_first_games below): the slots' first games hold every case


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


# ---- 1. the batch call ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _batch_inputs():
    """Boards and sides, on the host and on the device, built once: "Ra" entry by entry (invalid entries included), their
    colour-swapped images, "Nb" entry by entry, and the off-table boards."""
    from xiangqi_alphazero_amd import endgame
    ra = endgame.index_to_board("Ra", np.arange(endgame.entries("Ra")))
    nb = endgame.index_to_board("Nb", np.arange(endgame.entries("Nb")))
    boards = np.concatenate([ra[0], AM.swap_colours(*ra)[0], nb[0], off_table_boards()[0]])
    sides = np.concatenate([ra[1], AM.swap_colours(*ra)[1], nb[1], off_table_boards()[1]])
    boards.setflags(write=False)
    sides.setflags(write=False)
    return boards, sides, _cuda(boards), _cuda(sides), _cuda(EM.model("Ra").table)


@pytest.mark.parametrize("both_colours", [True, False], ids=["both_colours", "own_colours"])
@pytest.mark.parametrize("draws", [True, False], ids=["draws", "no_draws"])
def test_batch_equals_the_model_word_for_word(draws, both_colours):
    import torch
    from xiangqi_alphazero_amd import hip
    boards, sides, dev_boards, dev_sides, table = _batch_inputs()
    want = AM.adjudicate("Ra", EM.model("Ra").table, boards, sides, draws, both_colours)
    status, winner, value = hip.tb_adjudicate_batch("Ra", table, dev_boards, dev_sides, draws=draws, both_colours=both_colours)
    assert (status.dtype, winner.dtype, value.dtype) == (torch.uint8, torch.int8, torch.int16)
    for name, got, exp in zip(("status", "winner", "value"), (status, winner, value), want):
        got = got.cpu().numpy()
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (name, len(bad), int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
    seen = set(np.unique(want[0]).tolist())       # the inputs reach every bit: 16 only with both_colours, 8 only with draws off
    assert {0, 1, 2, 4} <= seen and any(s & 16 for s in seen) == both_colours and any(s & 8 for s in seen) == (not draws)
    # black wins no "Ra" ending of its own: winner -1 comes from the images alone
    assert set(np.unique(want[1]).tolist()) == ({-1, 0, 1} if both_colours else {0, 1})
    # an odd count that is no multiple of the four waves of a workgroup, and one position
    for n in (1, 7):
        part = hip.tb_adjudicate_batch("Ra", table, dev_boards[5000:5000 + n], dev_sides[5000:5000 + n], draws, both_colours)
        assert all((p.cpu().numpy() == w[5000:5000 + n]).all() for p, w in zip(part, want))
    empty = hip.tb_adjudicate_batch("Ra", table, dev_boards[:0], dev_sides[:0])
    assert all(len(e) == 0 for e in empty)


def test_batch_refuses_a_table_of_another_signature():
    import torch
    from xiangqi_alphazero_amd import hip
    _, _, dev_boards, dev_sides, table = _batch_inputs()
    with pytest.raises(hip.XqError, match="tb_adjudicate_batch"):
        hip.tb_adjudicate_batch("Nb", table, dev_boards[:4], dev_sides[:4])
    with pytest.raises(hip.XqError, match="draws"):
        hip.tb_adjudicate_batch("Ra", table, dev_boards[:4], dev_sides[:4], draws=2)
    with pytest.raises(hip.XqError, match="tb_adjudicate_batch"):
        hip.tb_adjudicate_batch("Ra", table, dev_boards[:4], torch.zeros(3, dtype=torch.int8).cuda())


# ---- 2. the engine stage, in situ -----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def situ_pool():
    """The pool of the in-situ run, from the model table of "Ra" alone (no GPU) -> (boards, sides, names).  Two entries each, in
    index order, of: won and drawn entries with either side to move; entries lost for black with a legal move (every move leads
    to a position red has won); drawn entries whose rook is gone (every move keeps the draw); then the colour-swapped image of
    each.  Then two hand-made boards -- a drawn entry plus a red pawn no table covers until it is captured, and an entry whose
    side to move has no legal move -- and the latter's image."""
    from xiangqi_alphazero_amd import endgame
    m = EM.model("Ra")
    t = m.table.astype(np.int64)
    idx = np.arange(m.entries)
    red = idx < m.entries // 2
    rook_gone = endgame.index_to_digits("Ra", idx)[:, 3] == 90
    groups = [("red_win", red & (t >= 3)), ("black_win", ~red & (t >= 3) & (t != EM.INVALID)), ("red_draw", red & (t == 0) & ~rook_gone),
              ("black_draw", ~red & (t == 0) & ~rook_gone), ("black_lost", ~red & (t < -1) & (t != EM.INVALID)),
              ("red_bare_draw", red & (t == 0) & rook_gone), ("black_bare_draw", ~red & (t == 0) & rook_gone)]
    pick, names = [], []
    for name, keep in groups:
        rows = np.nonzero(keep)[0]
        rows = rows[[len(rows) // 3, 2 * len(rows) // 3]] if len(rows) >= 2 else rows
        pick += rows.tolist()
        names += [name] * len(rows)
    boards, sides = endgame.index_to_board("Ra", pick)
    b2, s2 = AM.swap_colours(boards, sides)
    names += [n + "_image" for n in names]
    boards, sides = np.concatenate([boards, b2]), np.concatenate([sides, s2])
    drawn = np.nonzero(~red & (t == 0) & ~rook_gone)[0]
    pawn_board, pawn_side = endgame.index_to_board("Ra", drawn[[len(drawn) // 2]])
    square = next(sq for sq in range(45, 54) if pawn_board[0, sq] == 0 and pawn_board[0, sq + 9] == 0)
    pawn_board[0, square] = 7
    mated, mated_side = endgame.index_to_board("Ra", np.nonzero(~red & (t == -1))[0][:1])
    m2, ms2 = AM.swap_colours(mated, mated_side)
    boards = np.concatenate([boards, pawn_board, mated, m2])
    sides = np.concatenate([sides, pawn_side, mated_side, ms2])
    names += ["extra_pawn", "mated", "mated_image"]
    return boards.astype(np.int8), sides.astype(np.int8), names


def _first_games(seed, prob=0.75):
    """The names of the pool entries the slots' first games start from ("initial" for the initial position), on the host."""
    from xiangqi_alphazero_amd import hip
    names = situ_pool()[2]
    draws = [hip.start_pool_index(seed, 0, slot, 1, len(names), prob) for slot in range(G)]
    return ["initial" if d < 0 else names[d] for d in draws]


def test_the_seed_of_the_in_situ_run_covers_every_case():
    """No GPU work: the draw is a host function.  The first games of the 16 slots hold an entry red must win from, one black must
    win from through the image, a certain draw, a finished position, the board with the extra pawn and the initial position."""
    first = set(_first_games(SITU_SEED))
    assert {"black_lost", "black_lost_image", "initial", "extra_pawn"} <= first, sorted(first)
    assert first & {"red_bare_draw", "black_bare_draw", "red_bare_draw_image", "black_bare_draw_image"}
    assert first & {"mated", "mated_image"}


def _stub_expand(eng):
    """compact -> the stub evaluator of tests/stub_eval.py over the packed rows, on the host -> expand_packed."""
    import torch
    eng.compact()
    n = int(eng.n_live.item())
    ll = np.zeros((eng.G, 128), dtype=np.float32)
    value = np.zeros(eng.G, dtype=np.float32)
    if n:
        probs, value[:n] = _stub_batch(eng.packed_x[:n].cpu().numpy(), [True] * n)
        moves = eng.packed_moves[:n].cpu().numpy().view(np.uint16)
        counts = eng.packed_counts[:n].cpu().numpy()
        for r in range(n):
            ll[r, :counts[r]] = np.log(probs[r, moves[r, :counts[r]]])
    eng.expand_packed(torch.from_numpy(ll).cuda(), torch.from_numpy(value).cuda())


@pytest.mark.parametrize("manual_moves", [0, 2], ids=["selfplay_pool", "arena_initial"])
def test_engine_stage_equals_the_model_per_slot_and_step(manual_moves):
    import torch
    from xiangqi_alphazero_amd import engine, hip
    table = EM.model("Ra").table
    dev_table = _cuda(table)
    if manual_moves == 0:
        boards, sides, _ = situ_pool()
        cfg = engine.make_config(G, S, seed=SITU_SEED, max_game_length=12)
        eng = engine.SelfPlayEngine(cfg, start_pool=(boards, sides, 0.75))
    else:
        cfg = engine.make_config(G, S, seed=SITU_SEED, max_game_length=12, manual_moves=2, add_noise=False, random_opening_moves=0,
                                 enable_resign=False)
        eng = engine.SelfPlayEngine(cfg)
    assert eng.adjudicate_tables is None
    opts = hip.adjudicate_opts(draws=True, both_colours=True, min_ply=1)
    counters = torch.zeros((G, 4), dtype=torch.int64, device="cuda")
    want_counters = np.zeros((G, 4), dtype=np.int64)
    board_view, seen = eng.arena_views()["board"], {}
    for step in range(40):
        eng.select()
        gi = eng.slot_ints.cpu().numpy().copy()
        real = board_view.cpu().numpy().copy()
        want_gi, want_counters, why = AM.engine_step("Ra", table, real, gi, want_counters, True, True, 1)
        hip.engine_adjudicate(eng.h, "Ra", dev_table, opts, counters)
        got_gi = eng.slot_ints.cpu().numpy()
        for slot in range(G):
            assert (got_gi[slot] == want_gi[slot]).all(), (step, slot, why[slot], np.nonzero(got_gi[slot] != want_gi[slot])[0])
        assert (board_view.cpu().numpy() == real).all(), step
        assert (counters.cpu().numpy() == want_counters).all(), step
        for w in why:
            seen[w] = seen.get(w, 0) + 1
        _stub_expand(eng)
    assert eng.stats()["overflow"] == 0
    if manual_moves == 2:
        assert set(seen) <= {"phase", "min_ply", "not_covered"} and seen["not_covered"] > 0 and not want_counters.any()
        return
    swapped = sum(n for w, n in seen.items() if w.endswith("+swapped"))
    decided = {w.split("+")[0] for w in seen}
    assert {"red", "black", "draw", "phase", "status", "min_ply", "not_covered"} <= decided and swapped > 0, seen
    # the games the kernel decided ended as it said: reason 5, one move after the start, and the counters count them
    _, res = eng.drain()
    by_table = res[res["reason"] == hip.REASON_TABLE]
    assert len(by_table) > 0 and (by_table["steps"] >= 1).all()
    for w, col in ((1, "red"), (-1, "black"), (0, "draw")):
        assert int((by_table["winner"] == w).sum()) <= sum(n for k, n in seen.items() if k.split("+")[0] == col)
    assert int(want_counters[:, :2].sum()) >= len(by_table)           # a slot decided in the last steps has not flushed yet


# ---- 3. the option, end to end --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    from xiangqi_alphazero_amd import endgame
    return {sig: endgame.Tablebase.generate(sig, "cuda") for sig in ("R", "Ra")}


@lru_cache(maxsize=None)
def _won_pool():
    """64 won red-to-move entries of "R" that take at least three plies: one move cannot end the game by the rules."""
    from xiangqi_alphazero_amd import endgame
    m = EM.model("R")
    tb = endgame.Tablebase("R", m.table)
    boards, sides, index = tb.positions("win", 64, seed=2, side=1, min_plies=3)
    return boards.astype(np.int8), sides.astype(np.int8), index


def _play(tabs, options, n_games=48, graph=False, seed=9, **kw):
    """-> (samples, results) sorted, stats, engine."""
    from xiangqi_alphazero_amd import engine
    boards, sides, _ = _won_pool()
    cfg = engine.make_config(G, S, seed=seed, games_target=n_games, max_game_length=16)
    if tabs is not None:
        kw["adjudicate"] = (tabs, options)
    eng = engine.SelfPlayEngine(cfg, evaluator=_TorchStub(), start_pool=(boards, sides, 1.0), **kw)
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while True:
        eng.step()
        if eng.steps % 8 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 4000, "games did not finish"
    smp, res = eng.drain()
    return np.sort(smp, order=["slot", "game_seq", "ply"]), np.sort(res, order=["slot", "game_seq"]), eng.stats(), eng


@pytest.fixture(scope="module")
def one_move_games(tables):
    return _play((tables["R"],), dict(min_ply=1))


def test_every_game_ends_after_one_move_with_the_exact_z(one_move_games, tables):
    from xiangqi_alphazero_amd import hip
    smp, res, st, eng = one_move_games
    assert st["overflow"] == 0 and len(res) == 48 == len(smp)
    assert (res["reason"] == hip.REASON_TABLE).all() and (res["steps"] == 1).all() and (res["n_samples"] == 1).all()
    assert (smp["ply"] == 0).all() and (smp["side"] == 1).all()
    assert smp["slot"].tolist() == res["slot"].tolist() and smp["game_seq"].tolist() == res["game_seq"].tolist()
    assert (smp["z"] == res["winner"] * smp["side"]).all()
    # the winner is the table's verdict on the position after the sampled move, whatever that move was: mostly red's win
    assert set(np.unique(res["winner"]).tolist()) <= {1, 0} and int((res["winner"] == 1).sum()) > 24
    # games_target games start and no more, and all of them are finished: the counters' sum is the number of reason-5 results
    adj = eng.adjudication_stats()
    assert adj["adjudicated_decisive"] + adj["adjudicated_drawn"] == int((res["reason"] == hip.REASON_TABLE).sum()) == 48
    assert adj["adjudicated_decisive"] == int((res["winner"] != 0).sum())
    assert adj["adjudicated_swapped"] == 0 and adj["adjudicated_left_alone"] == 0


def test_min_ply_0_ends_games_at_ply_0_with_the_entry_s_value(tables):
    from xiangqi_alphazero_amd import hip
    smp, res, st, eng = _play((tables["R"],), dict(min_ply=0), seed=11)
    _, sides, index = _won_pool()
    assert len(smp) == 0 and len(res) == 48 and (res["steps"] == 0).all() and (res["n_samples"] == 0).all()
    assert (res["reason"] == hip.REASON_TABLE).all()
    value = tables["R"].table[index].astype(np.int64)
    for r in res:
        entry = hip.start_pool_index(11, 0, int(r["slot"]), int(r["game_seq"]), len(index), 1.0)
        assert int(r["winner"]) == int(np.sign(value[entry])) * int(sides[entry]) == 1
    # and the slots that still run say the same of their current games
    gseq = eng.slot_ints[:, hip.GI_GSEQ].cpu().numpy()
    started = eng.start_indices()
    for slot in range(G):
        if started[slot] >= 0:
            assert started[slot] == hip.start_pool_index(11, 0, slot, int(gseq[slot]), len(index), 1.0)


def test_replayed_steps_give_the_same_bytes(one_move_games, tables):
    smp, res, st, eng = one_move_games
    smp_g, res_g, st_g, eng_g = _play((tables["R"],), dict(min_ply=1), graph=True)
    assert smp_g.tobytes() == smp.tobytes() and res_g.tobytes() == res.tobytes() and st_g == st


def test_two_tables_give_the_games_of_the_larger_one(tables):
    """Every position of "R" is an entry of "Ra" with the advisor captured: "Ra" alone, and "Ra" then "R", decide the same."""
    one = _play((tables["Ra"],), dict(min_ply=1))
    two = _play((tables["Ra"], tables["R"]), dict(min_ply=1))
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() and one[2] == two[2]
    assert (one[1]["reason"] == 5).all() and one[3].adjudication_stats() == two[3].adjudication_stats()


def test_none_is_the_engine_without_the_argument():
    """One game per slot: with fewer games than slots, which slots win k_start_pool's race for the quota's tickets differs from run
    to run, and so do the games played."""
    a = _play(None, None, n_games=G)
    b = _play(None, None, n_games=G, adjudicate=None)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and len(a[0]) > 6
    assert not (a[1]["reason"] == 5).any() and a[3].adjudicate_tables is None
    from xiangqi_alphazero_amd import hip
    with pytest.raises(hip.XqError, match="adjudicate"):
        a[3].adjudication_stats()


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------
def test_one_iteration_of_the_loop_logs_the_fields(tmp_path):
    import json
    from test_early_stop_abi import _loop_config
    from xiangqi_alphazero_amd import train_loop
    cfg = _loop_config(tmp_path / "ck", endgame_signature="R", endgame_interval=99, start_positions_endgame=6,
                       start_positions_prob=1.0, adjudicate_signatures=["R"])
    cfg.num_games_per_iter, cfg.num_channels = 8, 64     # 64: the narrowest tower the hand-written evaluator takes
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    sp = saved[0]["self_play"]
    assert len(stats) == len(saved) == 1 and sp["games"] == 8 == sp["start_pool_games"]
    assert 1 <= sp["adjudicated_games"] <= 8 and sp["adjudicated_decisive"] + sp["adjudicated_drawn"] >= sp["adjudicated_games"]
    assert loop._adjudicate_tbs[0] is loop._endgame_table()
    plain = _loop_config(tmp_path / "b")
    plain.num_games_per_iter, plain.num_channels = 4, 64
    assert not any(k.startswith("adjudicated") for k in train_loop.AlphaZeroLoop(plain, "cuda", seed=3).train()[0]["self_play"])
