"""The baseline gate in the training loop (train_loop.AlphaZeroLoop, config.baseline_games): two iterations of a tiny loop log
the match against the fixed alpha-beta opponent under "baseline"; without the key the entries keep their form."""
import json
import os
import types

import pytest

pytestmark = pytest.mark.gpu

PLAIN = {"iteration", "time", "self_play", "training", "evaluation"}


def _config(tmp, **extra):
    return types.SimpleNamespace(
        num_channels=64, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=16,
        max_game_length=30, resign_threshold=-0.9, resign_check_steps=5, enable_resign=True, random_opening_moves=4,
        num_iterations=2, batch_size=64, num_epochs=1, learning_rate=0.002, weight_decay=1e-4, lr_milestones=[50, 80],
        lr_gamma=0.1, max_buffer_size=50000, min_buffer_size=100, eval_games=4, eval_win_rate=0.55, eval_simulations=8,
        checkpoint_dir=str(tmp), save_interval=2, **extra)


def test_loop_logs_the_baseline_match(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    cfg = _config(tmp_path / "ck", baseline_games=4, baseline_interval=1, baseline_depth=1, baseline_opening_plies=2,
                  game_records_dir=str(tmp_path / "records"))
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    stats = loop.train()
    saved = json.load(open(tmp_path / "ck" / "training_stats.json"))
    assert [s["iteration"] for s in stats] == [1, 2] and len(saved) == 2
    for entry, on_disk in zip(stats, saved):
        assert set(entry) == PLAIN | {"baseline"} == set(on_disk)
        b = on_disk["baseline"]
        assert set(b) == {"depth", "games", "wins", "losses", "draws", "win_rate", "win_rate_se", "seconds"}
        assert b["depth"] == 1 and b["games"] == 4 and b["wins"] + b["losses"] + b["draws"] == 4
        assert b["win_rate"] == (b["wins"] + 0.5 * b["draws"]) / 4 and b["win_rate_se"] >= 0 and b["seconds"] > 0
        assert b == entry["baseline"]
    # the match's records are written whatever config.record_games says; the other stages keep none without it
    assert sorted(os.listdir(tmp_path / "records")) == ["iter0001_baseline_rank0.txt", "iter0002_baseline_rank0.txt"]
    assert len(open(tmp_path / "records" / "iter0001_baseline_rank0.txt").read().splitlines()) >= 4


def test_loop_without_the_key_keeps_its_form(tmp_path):
    from xiangqi_alphazero_amd import train_loop
    loop = train_loop.AlphaZeroLoop(_config(tmp_path), "cuda", seed=3)
    assert loop.baseline is None
    stats = loop.train()
    saved = json.load(open(tmp_path / "training_stats.json"))
    assert len(stats) == len(saved) == 2
    for entry, on_disk in zip(stats, saved):
        assert set(entry) == PLAIN == set(on_disk)
    assert set(stats[1]["evaluation"]) == {"new_wins", "old_wins", "draws", "win_rate", "model_updated"}
