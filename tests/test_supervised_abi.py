"""CPU checks of game records as training samples (include/xq_hip.h: xq_supervise_opts, xq_records_sample_counts,
xq_records_to_samples): the two names in the header, the exports and the library; the options' size in C and ctypes; every refusal
coming back as XQ_ERR_ARG before any launch, so without a GPU (host addresses stand in for device buffers and are never
written); n = 0 being a no-op; the keywords of the Python layer."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xq_records_sample_counts", "xq_records_to_samples")


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip, hip.lib()


def test_new_exports_declared_and_present():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "xq_hip.h")).read()
    for name in NEW:
        assert name in hip.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header), name
    body = re.search(r"typedef struct xq_supervise_opts \{(.*?)\} xq_supervise_opts;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["movers", "skip_opening", "skip_draws", "reserved"]


def test_options_layout():
    hip, _ = _lib()
    assert C.sizeof(hip.SuperviseOpts) == 16            # the C side: four int32_t, no padding possible
    assert [n for n, _ in hip.SuperviseOpts._fields_] == ["movers", "skip_opening", "skip_draws", "reserved"]
    for i, (name, _) in enumerate(hip.SuperviseOpts._fields_):
        assert getattr(hip.SuperviseOpts, name).offset == 4 * i and getattr(hip.SuperviseOpts, name).size == 4


class _Buffers:
    """Host memory in the place of every device buffer of one record; a refused call must leave all of it alone."""

    def __init__(self, hip):
        self.records = np.zeros(1, dtype=hip.GAME_RECORD_DTYPE)
        self.movers = np.zeros(1, dtype=np.uint8)
        self.counts = np.full(1, -7, dtype=np.int32)
        self.offsets = np.zeros(2, dtype=np.int32)
        self.samples = np.full(640 + 16, 0xA5, dtype=np.uint8)
        self.status = np.full(1, -7, dtype=np.int32)
        self.rows = (self.samples.ctypes.data + 15) & ~15        # a 16-byte aligned row inside `samples`

    def untouched(self) -> bool:
        return (self.counts[0] == -7 and self.status[0] == -7 and bool((self.samples == 0xA5).all())
                and not self.records.view(np.uint8).any())


BAD_OPTS = [dict(movers=-1), dict(movers=4), dict(skip_opening=2), dict(skip_opening=-1), dict(skip_draws=2), dict(skip_draws=-1),
            dict(reserved=1), dict(reserved=-1)]


def _opts(hip, **kw):
    o = hip.SuperviseOpts(0, 1, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_counts_refusals_without_a_gpu():
    hip, lib = _lib()
    b = _Buffers(hip)
    good = _opts(hip)
    rec, mov, cnt = b.records.ctypes.data, b.movers.ctypes.data, b.counts.ctypes.data
    f = lib.xq_records_sample_counts
    assert f(rec, None, -1, C.byref(good), cnt, None) == -1                 # n < 0
    assert f(None, None, 1, C.byref(good), cnt, None) == -1                 # no records
    assert f(rec, None, 1, C.byref(good), None, None) == -1                 # no counts
    assert f(rec, mov, 1, None, cnt, None) == -1                            # no options
    assert f(None, None, 0, None, None, None) == -1                         # ... even for an empty batch
    for kw in BAD_OPTS:
        assert f(rec, mov, 1, C.byref(_opts(hip, **kw)), cnt, None) == -1, kw
        assert f(None, None, 0, C.byref(_opts(hip, **kw)), None, None) == -1, kw
    assert b.untouched()
    for movers in range(4):
        for so in (0, 1):
            for sd in (0, 1):
                assert f(None, None, 0, C.byref(hip.SuperviseOpts(movers, so, sd, 0)), None, None) == 0      # n = 0: a no-op


def test_conversion_refusals_without_a_gpu():
    hip, lib = _lib()
    b = _Buffers(hip)
    good = _opts(hip)
    rec, mov, off, st = b.records.ctypes.data, b.movers.ctypes.data, b.offsets.ctypes.data, b.status.ctypes.data
    f = lib.xq_records_to_samples
    assert f(rec, None, off, -1, C.byref(good), b.rows, st, None) == -1     # n < 0
    assert f(None, None, off, 1, C.byref(good), b.rows, st, None) == -1     # no records
    assert f(rec, None, None, 1, C.byref(good), b.rows, st, None) == -1     # no offsets
    assert f(rec, None, off, 1, C.byref(good), None, st, None) == -1        # no samples
    assert f(rec, None, off, 1, C.byref(good), b.rows, None, None) == -1    # no status
    assert f(rec, mov, off, 1, None, b.rows, st, None) == -1                # no options
    assert f(rec, mov, off, 1, C.byref(good), b.rows + 8, st, None) == -1   # rows are written with 16-byte stores
    assert f(None, None, None, 0, None, None, None, None) == -1
    for kw in BAD_OPTS:
        assert f(rec, mov, off, 1, C.byref(_opts(hip, **kw)), b.rows, st, None) == -1, kw
        assert f(None, None, None, 0, C.byref(_opts(hip, **kw)), None, None, None) == -1, kw
    assert b.untouched()
    assert f(None, None, None, 0, C.byref(good), None, None, None) == 0     # n = 0: a no-op


def test_python_layer_keywords():
    hip, _ = _lib()
    from xiangqi_alphazero_amd import train_loop, training
    p = inspect.signature(hip.records_to_samples).parameters
    assert list(p)[:5] == ["records", "movers", "per_record_movers", "skip_opening", "skip_draws"]
    assert (p["movers"].default, p["per_record_movers"].default, p["skip_opening"].default, p["skip_draws"].default) == \
        (0, None, True, False)
    assert inspect.signature(training.ReplayBuffer.extend_from_records).parameters["invalid"].default == "raise"
    assert list(inspect.signature(training.pretrain_from_records).parameters)[:5] == ["model", "optimizer", "records", "config",
                                                                                       "epochs"]
    assert callable(train_loop.AlphaZeroLoop.pretrain_from_records)
    for bad in (4, -1, 1.5, True):
        with pytest.raises(hip.XqError, match="movers"):
            hip.records_to_samples(np.zeros(1, dtype=hip.GAME_RECORD_DTYPE), movers=bad, device="cpu")
    with pytest.raises(hip.XqError, match="GAME_RECORD_DTYPE"):
        hip.records_to_samples(np.zeros(2, dtype=np.uint8), device="cpu")
