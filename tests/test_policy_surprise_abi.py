"""CPU checks of the scoring pass and the policy-surprise epoch counts (include/xq_hip.h: xq_samples_to_requests, xq_score_samples,
xq_surprise_counts, xq_surprise_count_host): header text, struct sizes, exports; every refusal returns XQ_ERR_ARG before any
launch, with no GPU present; the record dtypes existing tests pin are unchanged; train_network refuses the option on a buffer
without a scored record, with the option's name in the message; the config keys of AlphaZeroLoop and train_network."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

from policy_surprise_records import surprise_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_samples_to_requests", "xq_score_samples", "xq_surprise_counts", "xq_surprise_count_host")
FAKE = C.c_void_p(1 << 20)            # never dereferenced: the argument checks come first


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    for text in ("typedef struct xq_score_opts { double late_temperature; int32_t write_back; int32_t reserved; } xq_score_opts;",
                 "typedef struct xq_surprise_opts { double alpha; uint64_t seed; uint32_t epoch; uint32_t reserved; } xq_surprise_opts;",
                 "typedef struct xq_sample_score {", "typedef struct xq_sample_policy_stats {",
                 "#define XQ_SAMPLE_POLICY_STATS_OFFSET 120", "#define XQ_SURPRISE_SCRATCH_BYTES 16",
                 # the arithmetic, written out
                 "logp_i = l_i - M - log(sum_j exp(l_j - M))", "policy_ce = -sum_{t_i > 0} t_i * logp_i",
                 "policy_kl = max(0, sum_{t_i > 0} t_i * (log t_i - logp_i))",
                 "q_i = llrint(min(policy_kl_i, 64.0f) * 2^20) as uint64",
                 "w_i = (1 - alpha) + alpha * (((double)q_i * (double)M) / (double)S)",
                 "u_i = (double)(philox_u64(seed, epoch, slot, 10, game_seq, ply) >> 11) * 2^-53",
                 "c_i = floor(w_i) + (u_i < w_i - floor(w_i))", "exactly as xq_samples_to_batch forms them"):
        assert text in header, text
    assert C.sizeof(hip.ScoreOpts) == 16 and C.sizeof(hip.SampleScore) == 16
    assert C.sizeof(hip.SamplePolicyStats) == 8 and C.sizeof(hip.SurpriseOpts) == 24
    assert hip.ScoreOpts.write_back.offset == 8 and hip.ScoreOpts.reserved.offset == 12
    assert [getattr(hip.SampleScore, f).offset for f in ("policy_kl", "policy_ce", "value", "top1", "valid", "zero")] == [0, 4, 8, 12, 13, 14]
    assert [getattr(hip.SamplePolicyStats, f).offset for f in ("policy_kl", "has_policy_stats", "prior_top1", "zero")] == [0, 4, 5, 6]
    assert [getattr(hip.SurpriseOpts, f).offset for f in ("alpha", "seed", "epoch", "reserved")] == [0, 8, 16, 20]
    assert hip.POLICY_STATS_OFFSET == 120 and hip.SCORE_BYTES == 16 and hip.SURPRISE_SCRATCH_BYTES == 16
    # the stream kind is the source's and nobody else's
    src = open(os.path.join(ROOT, "xiangqi-alphazero_amd", "csrc", "xq_score.hip")).read()
    assert "XQ_RNG_KIND_SURPRISE" in src and "#define XQ_RNG_KIND_SURPRISE 10" in header and hip.RNG_KIND_SURPRISE == 10
    assert "static_assert(XQ_SAMPLE_POLICY_STATS_OFFSET >= XQ_SAMPLE_ROOT_STATS_OFFSET + offsetof(xq_sample_root_stats, zero)" in src


def test_pinned_record_layouts_are_unchanged():
    from xiangqi_alphazero_amd import sample_format as F
    assert F.SAMPLE_DTYPE == np.dtype([("board", np.int8, 90), ("side", np.int8), ("z", np.int8), ("n_moves", np.uint8),
                                       ("late_temp", np.uint8), ("ply", np.uint16), ("reserved0", np.uint16),
                                       ("reserved1", np.uint16), ("slot", np.uint32), ("game_seq", np.uint32), ("pad", np.uint8, 20),
                                       ("actions", np.uint16, 128), ("visits", np.uint16, 128)])
    assert F.ROOT_STATS_DTYPE == np.dtype([("root_q", np.float32), ("root_visits", np.uint32), ("has_root_stats", np.uint8),
                                           ("zero", np.uint8, 11)])
    assert F.SAMPLE_DTYPE.itemsize == 640 and F.ROOT_STATS_DTYPE.itemsize == 20 and F.SAMPLE_DTYPE.fields["pad"][1] == 108
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "    uint8_t has_root_stats;\n    uint8_t zero[11];\n} xq_sample_root_stats;" in header


def test_samples_to_requests_argument_errors():
    _, lib = _lib()

    def call(n=4, samples=FAKE, index=FAKE, planes=FAKE, moves=FAKE, counts=FAKE):
        return lib.xq_samples_to_requests(samples, index, n, planes, moves, counts, None)

    assert call(n=-1) == -1
    for k in ("samples", "planes", "moves", "counts"):
        assert call(**{k: None}) == -1, k
    assert call(planes=C.c_void_p((1 << 20) + 4)) == -1 and call(moves=C.c_void_p((1 << 20) + 2)) == -1
    assert call(n=0) == 0 and lib.xq_samples_to_requests(None, None, 0, None, None, None, None) == 0       # n = 0 is a no-op


def test_score_samples_argument_errors():
    hip, lib = _lib()

    def call(opts, n=4, samples=FAKE, index=None, logits=FAKE, value=FAKE, scores=FAKE):
        return lib.xq_score_samples(samples, index, n, logits, value, None if opts is None else C.byref(opts), scores, None)

    good = hip.ScoreOpts(0.3, 0, 0)
    assert call(None) == -1 and call(None, n=0) == -1
    assert call(hip.ScoreOpts(0.3, 0, 1)) == -1 and call(hip.ScoreOpts(0.3, 1, -1)) == -1           # a reserved word
    for wb in (2, -1, 256):
        assert call(hip.ScoreOpts(0.3, wb, 0)) == -1, wb
    for t in (0.0, -0.3, float("nan"), float("inf"), -float("inf")):
        assert call(hip.ScoreOpts(t, 0, 0)) == -1 and call(hip.ScoreOpts(t, 1, 0), n=0) == -1, t
    assert call(good, n=-1) == -1
    for k in ("samples", "logits", "value", "scores"):
        assert call(good, **{k: None}) == -1, k
    on = hip.ScoreOpts(0.3, 1, 0)
    assert call(on, n=0, scores=None) == 0 and call(good, n=0) == 0                                   # n = 0 is a no-op
    for k in ("samples", "logits", "value"):                                                          # scores may be NULL when writing back
        assert call(on, scores=None, **{k: None}) == -1, k
    assert call(good, scores=C.c_void_p((1 << 20) + 2)) == -1 and call(good, samples=C.c_void_p((1 << 20) + 1)) == -1


def test_surprise_counts_argument_errors():
    hip, lib = _lib()

    def call(opts, n=4, samples=FAKE, counts=FAKE, scratch=FAKE):
        return lib.xq_surprise_counts(samples, n, None if opts is None else C.byref(opts), counts, scratch, None)

    good = hip.SurpriseOpts(0.5, 1, 0, 0)
    assert call(None) == -1
    for a in (-0.1, 1.5, float("nan"), float("inf")):
        assert call(hip.SurpriseOpts(a, 1, 0, 0)) == -1 and call(hip.SurpriseOpts(a, 1, 0, 0), n=0) == -1, a
    assert call(hip.SurpriseOpts(0.5, 1, 0, 1)) == -1                                                 # the reserved word
    assert call(good, n=-1) == -1
    for k in ("samples", "counts", "scratch"):
        assert call(good, **{k: None}) == -1, k
    assert call(good, scratch=C.c_void_p((1 << 20) + 4)) == -1
    for a in (0.0, 1.0):
        assert call(hip.SurpriseOpts(a, 2 ** 64 - 1, 2 ** 32 - 1, 0), n=0) == 0                      # n = 0 is a no-op
    assert lib.xq_surprise_count_host(1.0, 1, 4, 4, -0.5, 1, 0, 0, 0, 0) == -1
    assert lib.xq_surprise_count_host(1.0, 1, 4, 4, float("nan"), 1, 0, 0, 0, 0) == -1


def _train_config(**extra):
    return types.SimpleNamespace(min_buffer_size=4, num_epochs=1, batch_size=8, **extra)


def test_train_network_refuses_the_option_without_scored_records():
    """Before any kernel call, so a CPU buffer shows it: alpha > 0 on a buffer none of whose records carries policy statistics."""
    import torch
    from xiangqi_alphazero_amd import hip, training
    unmarked = surprise_records(12, 1, marked_share=0.0)
    buf = training.ReplayBuffer(200, device="cpu")
    assert buf.policy_stats_coverage() == 0.0                                         # empty
    buf.extend(unmarked)
    assert buf.policy_stats_coverage() == 0.0 and len(buf) == 24
    net = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10])
    with pytest.raises(hip.XqError, match="policy_surprise_weight") as e:
        training.train_network(net, opt, sch, buf, _train_config(), surprise_weight=0.5)
    assert "policy statistics" in str(e.value)
    with pytest.raises(hip.XqError, match="policy_surprise_weight"):                  # the config's alpha is the default
        training.train_network(net, opt, sch, buf, _train_config(policy_surprise_weight=0.25))
    for bad in (-0.5, 1.5):
        with pytest.raises(hip.XqError, match="policy_surprise_weight"):
            training.train_network(net, opt, sch, buf, _train_config(), surprise_weight=bad)
        with pytest.raises(hip.XqError, match="policy_surprise_weight"):
            training.train_network(net, opt, sch, buf, _train_config(policy_surprise_weight=bad))
    assert training.train_network(net, opt, sch, training.ReplayBuffer(200, device="cpu"), _train_config(), surprise_weight=0.5) == {}
    # coverage over the ring's live records only: 1 marked of the 4 held after the ring wrapped
    ring = training.ReplayBuffer(8, device="cpu")                                     # 4 records
    marked = surprise_records(3, 2, marked_share=1.0)
    ring.extend(marked)
    assert ring.policy_stats_coverage() == 1.0
    ring.extend(unmarked[:3])                                                         # wraps: holds marked[2], unmarked[0..2]
    assert ring.count == 4 and ring.policy_stats_coverage() == 0.25


def test_python_layer_reads_the_config_keys(monkeypatch, tmp_path):
    from xiangqi_alphazero_amd import hip, selfplay, train_loop, training
    assert "surprise_weight" in inspect.signature(training.train_network).parameters
    assert inspect.signature(training.train_network).parameters["surprise_weight"].default is None
    sig = inspect.signature(selfplay.score_samples).parameters
    assert [(k, sig[k].default) for k in ("late_temperature", "write_back", "chunk")] == [("late_temperature", 0.3), ("write_back", True),
                                                                                         ("chunk", 2048)]
    assert list(inspect.signature(training.ReplayBuffer.epoch_order).parameters)[1:5] == ["alpha", "seed", "epoch", "generator"]
    for cfg, want in ((types.SimpleNamespace(), 0.0), (types.SimpleNamespace(policy_surprise_weight=None), 0.0),
                      (types.SimpleNamespace(policy_surprise_weight=0), 0.0), (types.SimpleNamespace(policy_surprise_weight=0.5), 0.5)):
        assert selfplay.policy_surprise_weight(cfg) == want
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=4, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path))
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base), device="cpu", seed=1)
    assert loop.surprise_weight == 0.0 and loop.score_samples is False
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, score_samples=True), device="cpu", seed=1)
    assert loop.surprise_weight == 0.0 and loop.score_samples is True
    with pytest.raises(hip.XqError, match="policy_surprise_weight"):
        train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, policy_surprise_weight=1.5), device="cpu")
    # ... once: the train step is handed the loop's value, whatever the config says by then
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, policy_surprise_weight=0.25), device="cpu", seed=1)
    assert loop.surprise_weight == 0.25 and loop.score_samples is True
    loop.config.policy_surprise_weight = 0.75
    seen = {}
    monkeypatch.setattr(training, "train_network", lambda *a, **kw: seen.update(kw) or {})
    assert loop.train_network() == {} and seen["surprise_weight"] == 0.25
    # an evaluator without the legal-move protocol is refused by name, before anything runs
    with pytest.raises(hip.XqError, match="evaluate_legal"):
        selfplay.score_samples(object(), None)


def test_a_shard_without_games_still_takes_part_in_every_gather(monkeypatch, tmp_path):
    """num_games_per_iter < world gives some ranks no game; with scoring on such a rank must enter the same three all-gathers as
    the others, its score tensor [0, 16].  One process: the gather is replaced by a recorder."""
    import torch
    from xiangqi_alphazero_amd import train_loop
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=0, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path))
    seen = []
    monkeypatch.setattr(train_loop.xdist, "all_gather_records_device", lambda t, group=None: (seen.append(tuple(t.shape)), t)[1])
    for extra, want in ((dict(score_samples=True), [(0, 640), (0, 16), (0, 16)]), (dict(policy_surprise_weight=0.5), [(0, 640), (0, 16), (0, 16)]),
                        ({}, [(0, 640), (0, 16)])):
        loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, **extra), device="cpu", seed=1)
        loop.grouped = True                                                           # the collectives' branch, gather recorded
        del seen[:]
        out = loop.self_play()
        assert seen == want, (extra, seen)
        assert ("mean_policy_kl" in out) == bool(extra) and out["games"] == 0 and out["new_samples"] == 0
        if extra:
            assert out["scored_samples"] == 0 and out["mean_policy_kl"] == 0.0
    # a _play_shard that plays but does not score (a subclass) also gathers one row per sample
    class Loop(train_loop.AlphaZeroLoop):
        def _play_shard(self, n_games):
            return torch.zeros((3, 640), dtype=torch.uint8), torch.zeros((1, 16), dtype=torch.uint8)
    loop = Loop(types.SimpleNamespace(**base, score_samples=True), device="cpu", seed=1)
    loop.grouped = True
    del seen[:]
    assert loop.self_play()["scored_samples"] == 0 and seen == [(3, 640), (1, 16), (3, 16)]


def test_the_loop_scores_with_the_buffers_temperature_and_one_evaluator(monkeypatch, tmp_path):
    import torch
    from xiangqi_alphazero_amd import evaluator, selfplay, train_loop
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=2, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path), score_samples=True)
    built, updated, calls = [], [], []

    class Ev:
        def update(self, net):
            updated.append(net)

    monkeypatch.setattr(evaluator, "make_evaluator", lambda net, dev, kind: (built.append(net), (Ev(), "fake"))[1])
    monkeypatch.setattr(selfplay, "run_games", lambda *a, **kw: (torch.zeros((5, 640), dtype=torch.uint8),
                                                                 torch.zeros((2, 16), dtype=torch.uint8), {}, 0.0))
    monkeypatch.setattr(selfplay, "score_samples", lambda ev, smp, t, write_back: (calls.append((ev, t, write_back)),
                                                                                   torch.zeros((smp.shape[0], 16), dtype=torch.uint8))[1])
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base), device="cpu", seed=1)
    loop.buffer.late_temperature = 0.45                                               # whatever the buffer trains on
    for _ in range(3):
        assert loop.self_play()["scored_samples"] == 0
    assert len(built) == 1 and built[0] is loop.best_model and updated == [loop.best_model] * 2     # built once, refreshed after
    assert [c[1:] for c in calls] == [(0.45, True)] * 3 and len({id(c[0]) for c in calls}) == 1
