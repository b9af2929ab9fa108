"""CPU-side checks of the synchronised-BatchNorm C ABI (include/xq_hip.h: xq_bn_sync_*): the size of the sums buffer and the argument
conventions.  Every call below returns XQ_ERR_ARG before any launch, so none of them needs (or touches) a GPU."""

SYNC = ["xq_bn_sync_sums_count", "xq_bn_sync_forward_stats", "xq_bn_sync_forward_apply", "xq_bn_sync_backward_stats",
        "xq_bn_sync_backward_apply"]
A = 1 << 20                                    # a 16-byte-aligned stand-in address (never dereferenced)


def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


def _fwd_stats(lib, p=A, rows=900, c=64, sums=A):
    return lib.xq_bn_sync_forward_stats(p, rows, c, sums, p, None)


def _fwd_apply(lib, p=A, rows=900, c=64, sums=A, run=A):
    return lib.xq_bn_sync_forward_apply(p, None, p, p, run, run, 0.1, 1e-5, rows, c, 1, sums, p, p, p, None, None)


def _bwd_stats(lib, p=A, rows=900, c=64, sums=A):
    return lib.xq_bn_sync_backward_stats(p, p, p, p, p, rows, c, 1, sums, p, p, p, None)


def _bwd_apply(lib, p=A, rows=900, c=64, sums=A):
    return lib.xq_bn_sync_backward_apply(p, p, p, p, p, p, rows, c, 1, sums, p, None, None)


CALLS = (_fwd_stats, _fwd_apply, _bwd_stats, _bwd_apply)


def test_sums_count_is_two_per_channel_plus_the_row_count():
    lib = _lib()
    for c in (64, 128, 256, 512, 1024, 4, 1):
        assert lib.xq_bn_sync_sums_count(c) == 2 * c + 1
    assert lib.xq_bn_sync_sums_count(0) == 0 and lib.xq_bn_sync_sums_count(-64) == 0


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    for call in CALLS:
        name = call.__name__
        assert call(lib, p=None) == -1, name                                  # null data pointers
        assert call(lib, sums=None) == -1, name                               # null sums
        for c in (0, 32, 96, 100, 2048, -64):                                 # channels the kernels do not take (bn_args_ok)
            assert call(lib, c=c) == -1, (name, c)
        for rows in (0, -90):
            assert call(lib, rows=rows) == -1, (name, rows)
        for off in (1, 4):                                                    # sums must be 8-byte aligned
            assert call(lib, sums=A + off) == -1, (name, off)
        assert call(lib, p=A + 8) == -1, name                                 # tensors 16-byte aligned, as the fused entry points
    # running statistics come as a pair
    assert lib.xq_bn_sync_forward_apply(A, None, A, A, A, None, 0.1, 1e-5, 900, 64, 1, A, A, A, A, None, None) == -1
    # the ReLU mask needs y
    assert lib.xq_bn_sync_backward_stats(A, A, None, A, A, 900, 64, 1, A, A, A, A, None) == -1
    assert lib.xq_bn_sync_backward_apply(A, A, None, A, A, A, 900, 64, 1, A, A, None, None) == -1
    # a null scratch buffer is refused by the two stats calls
    assert lib.xq_bn_sync_forward_stats(A, 900, 64, A, None, None) == -1
    assert lib.xq_bn_sync_backward_stats(A, A, A, A, A, 900, 64, 1, A, A, A, None, None) == -1


def test_header_and_exports_list_the_sync_entry_points():
    import os
    from xiangqi_alphazero_amd import hip
    lib = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xq_hip.h")).read()
    for n in SYNC:
        assert n in hip.EXPORTS and hasattr(lib, n) and (n + "(") in header, n
