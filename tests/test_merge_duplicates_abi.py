"""CPU checks of merging duplicate positions (include/xq_hip.h: xq_position_keys, xq_position_key_host, xq_position_group_heads,
xq_groups_to_batch): header text, exports, the struct layouts earlier tests pin; every refusal returns XQ_ERR_ARG before any
launch, with no GPU present; train_network refuses the option together with policy-surprise weighting, naming both keys; the
config keys of AlphaZeroLoop and train_network."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

from policy_surprise_records import surprise_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_position_keys", "xq_position_key_host", "xq_position_group_heads", "xq_groups_to_batch")
FAKE = C.c_void_p(1 << 20)            # never dereferenced: the argument checks come first
ODD = C.c_void_p((1 << 20) + 4)


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for n in NEW:
        assert n + "(" in header and n in hip.EXPORTS and hasattr(lib, n)
    for text in ("#define XQ_POSITION_KEY_MIRROR 1", "mir(sq) = (sq / 9) * 9 + 8 - sq % 9",
                 "let sq* be the smallest square with board[sq*] != board[mir(sq*)]",
                 "mirrored = (board[mir(sq*)] < board[sq*]), compared as int8",
                 "x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31",
                 "term(i, b) = mix(0x9E3779B97F4A7C15 * (uint64)(i * 256 + (uint8)b + 1))",
                 "XOR over sq < 90 of term(sq, c[sq]), then ^ term(90, side)",
                 "starts a group iff j == 0, or its key, its side or its canonical board (90 bytes) differs",
                 "pi[a] = (float)((0.0 + t_0[a] + t_1[a] + ...) / (double)n_pi)",
                 "z     = (float)((0.0 + zt_0 + zt_1 + ...) / (double)n)", "VALID iff total_k > 0",
                 "o_k = member_mirrored_k XOR f"):
        assert text in header, text
    assert hip.POSITION_KEY_MIRROR == 1
    src = open(os.path.join(ROOT, "xiangqi-alphazero_amd", "csrc", "xq_merge.hip")).read()
    assert "__ballot" in src and "atomicAdd" not in src


def test_pinned_layouts_are_unchanged():
    hip, _ = _lib()
    from xiangqi_alphazero_amd import sample_format as F
    assert F.SAMPLE_DTYPE.itemsize == 640 and F.ROOT_STATS_DTYPE.itemsize == 20 and F.SAMPLE_DTYPE.fields["pad"][1] == 108
    assert F.SAMPLE_DTYPE.fields["board"][1] == 0 and F.SAMPLE_DTYPE.fields["side"][1] == 90
    assert F.POLICY_STATS_DTYPE.itemsize == 8 and F.SCORE_DTYPE.itemsize == 16 and F.GAME_RECORD_DTYPE.itemsize == 1024
    assert C.sizeof(hip.BatchOpts) == 16 and hip.BatchOpts.reserved.offset == 8
    assert C.sizeof(hip.ScoreOpts) == 16 and C.sizeof(hip.SampleScore) == 16 and C.sizeof(hip.SurpriseOpts) == 24
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    assert "typedef struct xq_batch_opts { double q_mix; int32_t reserved[2]; } xq_batch_opts;" in header


def test_position_keys_argument_errors():
    _, lib = _lib()

    def call(n=4, flags=1, samples=FAKE, index=None, keys=FAKE, mirrored=FAKE):
        return lib.xq_position_keys(samples, index, n, flags, keys, mirrored, None)

    assert call(n=-1) == -1
    for flags in (2, 3, -1, 256):
        assert call(flags=flags) == -1 and call(flags=flags, n=0) == -1, flags
    for k in ("samples", "keys", "mirrored"):
        assert call(**{k: None}) == -1, k
    assert call(keys=ODD) == -1
    for flags in (0, 1):
        assert call(n=0, flags=flags) == 0 and lib.xq_position_keys(None, None, 0, flags, None, None, None) == 0


def test_position_key_host_refuses_bad_arguments():
    hip, lib = _lib()
    m = C.c_uint8(7)
    board = np.zeros(90, dtype=np.int8)
    assert lib.xq_position_key_host(None, 1, 1, C.addressof(m)) == 0 and m.value == 0
    m = C.c_uint8(7)
    assert lib.xq_position_key_host(board.ctypes.data, 1, 2, C.addressof(m)) == 0 and m.value == 0
    assert lib.xq_position_key_host(board.ctypes.data, 1, 1, None) == hip.position_key_host(board, 1, True)[0] != 0


def test_position_group_heads_argument_errors():
    _, lib = _lib()

    def call(n=4, samples=FAKE, index=None, order=FAKE, keys=FAKE, mirrored=FAKE, head=FAKE):
        return lib.xq_position_group_heads(samples, index, order, keys, mirrored, n, head, None)

    assert call(n=-1) == -1
    for k in ("samples", "order", "keys", "mirrored", "head"):
        assert call(**{k: None}) == -1, k
    assert call(keys=ODD) == -1
    assert call(n=0) == 0 and lib.xq_position_group_heads(None, None, None, None, None, 0, None, None) == 0


def test_groups_to_batch_argument_errors():
    hip, lib = _lib()

    def call(opts=None, n=4, n_groups=3, t=0.3, samples=FAKE, offsets=FAKE, members=FAKE, mirrored=FAKE, group=FAKE, flip=FAKE,
             states=FAKE, pi=FAKE, z=FAKE):
        return lib.xq_groups_to_batch(samples, offsets, members, mirrored, n_groups, group, flip, n, t,
                                      None if opts is None else C.byref(opts), states, pi, z, None)

    assert call(n=-1) == -1 and call(n_groups=-1) == -1 and call(n=0, n_groups=-1) == -1
    for k in ("samples", "offsets", "members", "mirrored", "group", "flip", "states", "pi", "z"):
        assert call(**{k: None}) == -1, k
    for t in (0.0, -0.3, float("nan")):
        assert call(t=t) == -1 and call(t=t, n=0) == -1, t
    for q in (-0.1, 1.5, float("nan")):
        assert call(hip.BatchOpts(q)) == -1 and call(hip.BatchOpts(q), n=0) == -1, q
    for word in (0, 1):
        opts = hip.BatchOpts(0.25)
        opts.reserved[word] = 1
        assert call(opts) == -1, word
    assert call(pi=ODD) == -1
    assert call(n=0) == 0 and call(hip.BatchOpts(0.25), n=0) == 0 and call(hip.BatchOpts(1.0), n=0, n_groups=0) == 0
    assert lib.xq_groups_to_batch(None, None, None, None, 0, None, None, 0, 0.3, None, None, None, None, None) == 0


def _train_config(**extra):
    return types.SimpleNamespace(min_buffer_size=4, num_epochs=1, batch_size=8, **extra)


def test_train_network_refuses_merging_with_surprise_weighting():
    """Before any kernel call, so a CPU buffer shows it."""
    import torch
    from xiangqi_alphazero_amd import hip, training
    buf = training.ReplayBuffer(200, device="cpu")
    buf.extend(surprise_records(12, 1, marked_share=1.0))
    net = torch.nn.Linear(2, 2)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10])
    for kw, cfg in ((dict(merge_duplicates=True, surprise_weight=0.5), _train_config()),
                    (dict(), _train_config(merge_duplicate_positions=True, policy_surprise_weight=0.25)),
                    (dict(merge_duplicates=True), _train_config(policy_surprise_weight=0.25)),
                    (dict(surprise_weight=1.0), _train_config(merge_duplicate_positions=True))):
        with pytest.raises(hip.XqError, match="merge_duplicate_positions") as e:
            training.train_network(net, opt, sch, buf, cfg, **kw)
        assert "policy_surprise_weight" in str(e.value)
    # an empty buffer trains nothing, whatever the options
    assert training.train_network(net, opt, sch, training.ReplayBuffer(200, device="cpu"), _train_config(), merge_duplicates=True) == {}


def test_python_layer_reads_the_config_keys(monkeypatch, tmp_path):
    from xiangqi_alphazero_amd import hip, train_loop, training
    sig = inspect.signature(training.train_network).parameters
    assert sig["merge_duplicates"].default is None and sig["merge_mirror"].default is None
    assert list(inspect.signature(training.ReplayBuffer.position_groups).parameters) == ["self", "mirror"]
    assert inspect.signature(training.ReplayBuffer.position_groups).parameters["mirror"].default is True
    assert list(inspect.signature(training.ReplayBuffer.batch_groups).parameters) == ["self", "groups", "logical", "q_mix"]
    assert [f for f in training.PositionGroups.__dataclass_fields__] == ["offsets", "members", "member_mirrored", "n_groups", "sizes",
                                                                         "n_records"]
    for cfg, want in ((types.SimpleNamespace(), (False, True)), (types.SimpleNamespace(merge_duplicate_positions=None), (False, True)),
                      (types.SimpleNamespace(merge_duplicate_positions=True), (True, True)),
                      (types.SimpleNamespace(merge_duplicate_positions=1, merge_mirror_positions=False), (True, False)),
                      (types.SimpleNamespace(merge_mirror_positions=None), (False, True))):
        assert (training.merge_duplicate_positions(cfg), training.merge_mirror_positions(cfg)) == want
    base = dict(num_simulations=8, c_puct=1.5, temperature_threshold=10, max_game_length=30, random_opening_moves=2,
                enable_resign=False, resign_threshold=-0.9, resign_check_steps=5, num_channels=16, num_res_blocks=1,
                num_games_per_iter=4, learning_rate=0.01, weight_decay=1e-4, lr_milestones=[2], lr_gamma=0.1, max_buffer_size=40,
                min_buffer_size=4, num_epochs=1, batch_size=8, eval_games=4, eval_simulations=4, eval_win_rate=0.55,
                save_interval=2, num_iterations=1, checkpoint_dir=str(tmp_path))
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base), device="cpu", seed=1)
    assert loop.merge_duplicates is False and loop.merge_mirror is True
    with pytest.raises(hip.XqError, match="merge_duplicate_positions") as e:
        train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, merge_duplicate_positions=True, policy_surprise_weight=0.5), device="cpu")
    assert "policy_surprise_weight" in str(e.value)
    # read once: the train step is handed the loop's values, whatever the config says by then
    loop = train_loop.AlphaZeroLoop(types.SimpleNamespace(**base, merge_duplicate_positions=True, merge_mirror_positions=False),
                                    device="cpu", seed=1)
    assert loop.merge_duplicates is True and loop.merge_mirror is False
    loop.config.merge_duplicate_positions, loop.config.merge_mirror_positions = False, True
    seen = {}
    monkeypatch.setattr(training, "train_network", lambda *a, **kw: seen.update(kw) or {})
    assert loop.train_network() == {} and seen["merge_duplicates"] is True and seen["merge_mirror"] is False


def test_the_epoch_loop_is_unchanged_when_off(monkeypatch):
    """With the option off train_network never asks for groups, and the stats say so."""
    import torch
    from xiangqi_alphazero_amd import training
    buf = training.ReplayBuffer(200, device="cpu")
    buf.extend(surprise_records(12, 1))
    monkeypatch.setattr(buf, "position_groups", lambda *a, **kw: pytest.fail("groups built with the option off"))
    monkeypatch.setattr(buf, "batch", lambda idx, q_mix=0.0: (torch.zeros((len(idx), 2)), torch.full((len(idx), 2), 0.5),
                                                               torch.zeros((len(idx), 1))))

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 3)

        def forward(self, x):
            y = self.lin(x)
            return y[:, :2], y[:, 2:]

    net = Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10])
    for cfg in (_train_config(), _train_config(merge_duplicate_positions=False), _train_config(merge_duplicate_positions=None)):
        st = training.train_network(net, opt, sch, buf, cfg, generator=torch.Generator().manual_seed(1))
        assert st["merge_duplicate_positions"] is False and st["epoch_samples"] == [24]
        assert st["distinct_positions"] is None and st["merged_records"] is None and st["largest_group"] is None
