"""CPU checks of the fixed alpha-beta opponent's boundary (include/xq_hip.h, xq_alphabeta_batch): the export in the header, in
hip.EXPORTS and in the library; the four constants; every argument error before any launch; the keywords of the Python layer;
the baseline gate's config keys in AlphaZeroLoop."""
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_export_declared_listed_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "xq_alphabeta_batch" in hip.EXPORTS and hasattr(lib, "xq_alphabeta_batch")
    assert re.search(r"\bint xq_alphabeta_batch\s*\(", header)
    for line, value in (("#define XQ_AB_MAX_DEPTH 4", hip.AB_MAX_DEPTH), ("#define XQ_AB_MATE      30000", hip.AB_MATE),
                        ("#define XQ_AB_UNSCORED  INT32_MIN", hip.AB_UNSCORED), ("#define XQ_AB_NO_MOVE   0xFFFF", hip.AB_NO_MOVE)):
        assert line in header, line
    assert (hip.AB_MAX_DEPTH, hip.AB_MATE, hip.AB_UNSCORED, hip.AB_NO_MOVE) == (4, 30000, -2 ** 31, 0xFFFF)
    from xiangqi_alphazero_amd import baseline
    assert (baseline.MAX_DEPTH, baseline.MATE, baseline.UNSCORED, baseline.NO_MOVE) == (4, 30000, -2 ** 31, 0xFFFF)


def test_argument_errors_come_back_without_a_gpu():
    """Host buffers stand in for device memory: a refused call launches nothing and writes nothing."""
    _, lib = _lib()
    boards, side = np.zeros((2, 90), dtype=np.int8), np.ones(2, dtype=np.int8)
    outs = dict(moves=np.full((2, 128), 7, np.uint16), counts=np.full(2, 7, np.uint16), scores=np.full((2, 128), 7, np.int32),
                nodes=np.full((2, 128), 7, np.uint32), best_action=np.full(2, 7, np.uint16), best_score=np.full(2, 7, np.int32),
                status=np.full(2, 7, np.uint8))
    draws = np.zeros(2, dtype=np.uint32)
    order = ("moves", "counts", "scores", "nodes", "best_action", "best_score", "status")

    def call(n=2, depth=2, b=boards, s=side, d=draws, **drop):
        ptr = [None if drop.get(k) else outs[k].ctypes.data for k in order]
        return lib.xq_alphabeta_batch(None if b is None else b.ctypes.data, None if s is None else s.ctypes.data, n, depth,
                                      None if d is None else d.ctypes.data, *ptr, None)

    assert call(n=-1) == -1
    assert call(depth=-1) == -1 and call(depth=5) == -1
    assert call(n=0, depth=5) == -1 and call(n=-1, depth=0) == -1          # the range is checked whatever n is
    assert call(b=None) == -1 and call(s=None) == -1
    for k in order:
        if k != "nodes":
            assert call(**{k: True}) == -1, k
    assert all((v == 7).all() for v in outs.values())
    # n == 0 is a no-op, whatever the pointers; every depth of the range is accepted
    for depth in range(5):
        assert lib.xq_alphabeta_batch(None, None, 0, depth, None, None, None, None, None, None, None, None, None) == 0
    assert call(n=0) == 0 and all((v == 7).all() for v in outs.values())


def test_python_layer_keywords():
    hip, _ = _lib()
    from xiangqi_alphazero_amd import baseline
    assert list(inspect.signature(hip.alphabeta_batch).parameters) == ["boards", "side", "depth", "draws"]
    assert inspect.signature(hip.alphabeta_batch).parameters["draws"].default is None
    sig = inspect.signature(baseline.play_vs_baseline).parameters
    assert list(sig) == ["model_or_evaluator", "num_games", "depth", "num_simulations", "opening_plies", "seed", "max_game_length",
                         "c_puct", "perpetual_check", "solver", "device", "evaluator_kind"]
    want = dict(opening_plies=4, seed=0, max_game_length=200, c_puct=1.5, perpetual_check=False, solver=False, device="cuda",
                evaluator_kind="hip")
    assert {k: sig[k].default for k in want} == want
    assert list(inspect.signature(baseline.pick).parameters) == ["scores", "count", "draw"]
    # refusals that need no GPU: the depth, and a match's shape
    import torch
    with pytest.raises(hip.XqError, match="depth"):
        hip.alphabeta_batch(torch.zeros((1, 90), dtype=torch.int8), torch.ones(1, dtype=torch.int8), 5)
    for kw, word in ((dict(num_games=3), "num_games"), (dict(num_games=0), "num_games"), (dict(depth=5), "depth"),
                     (dict(opening_plies=17), "opening_plies"), (dict(max_game_length=505), "max_game_length"),
                     (dict(model_or_evaluator=7), "depth")):
        args = {**dict(model_or_evaluator=1, num_games=4, depth=1, num_simulations=4), **kw}
        with pytest.raises(hip.XqError, match=word):
            baseline.play_vs_baseline(**args)


def test_loop_reads_and_refuses_the_baseline_keys(tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=4, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=6, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path))

    def loop(**extra):
        return train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, **extra), device="cpu", seed=1)

    assert loop().baseline is None and loop(baseline_games=0).baseline is None and loop(baseline_games=None).baseline is None
    assert loop(baseline_games=0, baseline_depth=3, baseline_interval=1).baseline is None
    assert loop(baseline_games=8).baseline == dict(games=8, depth=2, simulations=6, opening_plies=4, interval=2)
    assert loop(baseline_games=2, baseline_depth=0, baseline_simulations=3, baseline_opening_plies=16,
                baseline_interval=1).baseline == dict(games=2, depth=0, simulations=3, opening_plies=16, interval=1)
    assert loop(baseline_games=2, baseline_depth=4, baseline_opening_plies=0).baseline["depth"] == 4
    for extra, key in ((dict(baseline_games=-2), "baseline_games"), (dict(baseline_games=3), "baseline_games"),
                       (dict(baseline_games=2.5), "baseline_games"),
                       (dict(baseline_games=4, baseline_depth=5), "baseline_depth"),
                       (dict(baseline_games=4, baseline_depth=-1), "baseline_depth"),
                       (dict(baseline_depth=9), "baseline_depth"),                      # checked even while the gate is off
                       (dict(baseline_games=4, baseline_opening_plies=17), "baseline_opening_plies"),
                       (dict(baseline_games=4, baseline_opening_plies=-1), "baseline_opening_plies"),
                       (dict(baseline_games=4, baseline_interval=0), "baseline_interval"),
                       (dict(baseline_games=4, baseline_simulations=0), "baseline_simulations")):
        with pytest.raises(hip.XqError, match=key):
            loop(**extra)
