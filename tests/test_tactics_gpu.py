"""The tactics yardstick on the GPU (tactics.py, train_loop.AlphaZeroLoop's config.tactics_file): the puzzles the device finds
are the model's, the solve rate is what the labels say of the moves a separate search chooses, and two iterations of a tiny loop
log it under "tactics"."""
import json
from functools import lru_cache

import numpy as np
import pytest

import golden_io
import mate_model as M
from test_baseline_loop_gpu import PLAIN, _config

pytestmark = pytest.mark.gpu

SUBSET = tuple(range(500, 600))
ENTRY = {"puzzles", "solved", "optimal", "solve_rate", "by_mate_in", "max_moves", "simulations", "seconds"}


@lru_cache(maxsize=None)
def _labelled():
    d = golden_io.corpus()
    idx = list(SUBSET)
    return M.label(d["board"][idx], d["side"][idx], 5)


def test_find_puzzles_is_the_models_selection():
    from xiangqi_alphazero_amd import tactics
    from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE
    d = golden_io.corpus()
    idx = list(SUBSET)
    want = _labelled()
    got = tactics.label(d["board"][idx], d["side"][idx], 5)
    assert got.dtype == tactics.PUZZLE_DTYPE and got.tobytes() == want.tobytes()
    for kw in (dict(), dict(min_moves=1), dict(min_moves=3, unique=False)):
        found = tactics.find_puzzles(d["board"][idx], d["side"][idx], 5, **kw)
        model = tactics.select(want, 5, kw.get("min_moves", 2), kw.get("unique", True))
        assert len(found) > 0 and found.tobytes() == model.tobytes(), kw
    samples = np.zeros(len(idx), dtype=SAMPLE_DTYPE)
    samples["board"], samples["side"] = d["board"][idx], d["side"][idx]
    assert tactics.find_puzzles(samples, None, 5).tobytes() == tactics.select(want, 5, 2, True).tobytes()
    # N = 3 keeps the mates in two and three only
    three = tactics.find_puzzles(d["board"][idx], d["side"][idx], 3)
    assert sorted(set(three["mate_in"].tolist())) == [2, 3]
    assert (three["board"] == tactics.select(want, 3, 2, True)["board"]).all()


@pytest.mark.parametrize("solver", [False, True])
def test_solve_rate_is_what_the_labels_say_of_the_search(solver):
    import torch
    from xiangqi_alphazero_amd import tactics
    from xiangqi_alphazero_amd.mcts import MCTS, solver_choice
    from xiangqi_alphazero_amd.model import XiangqiNet
    puzzles = tactics.select(_labelled(), 5, 1, unique=True)[:8]
    assert len(puzzles) == 8 and len(set(puzzles["mate_in"].tolist())) >= 2
    torch.manual_seed(5)
    net = XiangqiNet(64, 1).cuda().eval()
    res = tactics.solve_rate(net, puzzles, 16, solver=solver, seed=7)
    assert set(res) == {"puzzles", "solved", "optimal", "solve_rate", "by_mate_in", "simulations", "seconds", "chosen"}
    # a separate search with the same seed
    mcts = MCTS(net, 16, 1.5, "cuda", "hip", seed=7, solver=solver)
    mcts.search_many([tactics._Position(p["board"], p["side"]) for p in puzzles], temperature=1.0, add_noise=False)
    eng = mcts._engine(8, False)
    chosen = []
    for slot in range(8):
        r = eng.read_root(slot)
        if solver:
            chosen.append(solver_choice(r["actions"], r["visits"], eng.read_root_states(slot)["children"]))
        else:
            chosen.append(int(r["actions"][int(np.argmax(r["visits"]))]))
    assert list(res["chosen"]) == chosen
    labels = []
    for p, a in zip(puzzles, chosen):
        j = list(p["moves"][:p["n_moves"]]).index(a)       # the chosen move is a root move
        labels.append(int(p["move_mate_in"][j]))
    solved = [1 <= m <= 5 for m in labels]
    assert res["puzzles"] == 8 and res["solved"] == sum(solved) and res["solve_rate"] == sum(solved) / 8
    assert res["optimal"] == sum(m == int(p["mate_in"]) for m, p in zip(labels, puzzles)) <= res["solved"]
    assert res["simulations"] == 16 and res["seconds"] > 0
    by = res["by_mate_in"]
    assert sum(c for c, _ in by.values()) == 8 and sum(s for _, s in by.values()) == res["solved"]
    for m, (c, s) in by.items():
        assert c == int((puzzles["mate_in"] == m).sum()) and s == sum(ok for ok, p in zip(solved, puzzles) if p["mate_in"] == m)
    again = tactics.solve_rate(net, puzzles, 16, solver=solver, seed=7)
    assert list(again["chosen"]) == chosen
    # chunks smaller than the set give the same moves
    assert list(tactics.solve_rate(net, puzzles, 16, solver=solver, seed=7, chunk=3)["chosen"]) == chosen


def test_loop_logs_the_solve_rate(tmp_path):
    from xiangqi_alphazero_amd import tactics, train_loop
    labelled = _labelled()
    kept = tactics.select(labelled, 3, 1, unique=False)
    some = np.concatenate([kept[:6], labelled[labelled["mate_in"] == 0][:2], labelled[labelled["mate_in"] > 3][:1]])
    path = tmp_path / "puzzles.txt"
    path.write_text(tactics.puzzles_to_text(some, header=["nine positions, six of them mates within three"]))
    cfg = _config(tmp_path / "ck", tactics_file=str(path), tactics_max_moves=3, tactics_simulations=8)
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    assert loop.baseline is None
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    assert [s["iteration"] for s in stats] == [1, 2] and len(saved) == 2
    for entry, on_disk in zip(stats, saved):
        assert set(entry) == PLAIN | {"tactics"} == set(on_disk)
        t = on_disk["tactics"]
        assert set(t) == ENTRY and t == entry["tactics"]
        assert t["puzzles"] == 6 and t["max_moves"] == 3 and t["simulations"] == 8 and t["seconds"] > 0
        assert 0 <= t["optimal"] <= t["solved"] <= 6 and t["solve_rate"] == t["solved"] / 6
        assert sum(c for c, _ in t["by_mate_in"].values()) == 6 and set(t["by_mate_in"]) <= {"1", "2", "3"}
    assert loop.tactics["dropped"] == 3 and len(loop._tactics_puzzles) == 6


def test_loop_without_the_key_keeps_its_form(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    cfg = _config(tmp_path)
    cfg.num_iterations = 1
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    assert loop.tactics is None
    stats = loop.train()
    saved = json.load(open(tmp_path / "training_stats.json"))
    assert len(stats) == len(saved) == 1 and set(stats[0]) == PLAIN == set(saved[0])
