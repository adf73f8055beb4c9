"""The bf16 entries of the C-ABI: exported, declared to ctypes, and rejecting bad arguments
before anything reaches a device (no GPU needed)."""
import pytest

NEW = ("gnn_spmm_csr_bf16", "gnn_spmm_csr_hub_bf16", "gnn_spmm_csr_tasks_bf16",
       "gnn_gather_rows_bf16", "gnn_gcn_transform_bf16out", "gnn_gcn_transform_rows_bf16out")
E_ARG, E_UNSUPPORTED = -1, -3
P = 4096  # a non-null pointer value; never dereferenced: every call below fails its checks


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


def test_symbols_load(lib):
    from graphneuralnetwork_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.error_string(E_UNSUPPORTED)


def _plan_tail(flags=0, small=True):
    # seg_len, seg_row, seg_begin, n_seg, long_row, long_seg_ptr, n_long,
    # [small_row, small_col, small_val, n_small,] mid_row, n_mid
    t = (8, None, None, 0, None, None, 0)
    if small:
        t += (None, None, None, 0)
    return t + (None, 0)


def _plain(lib, rowptr=P, n_rows=10, x=P, ldx=8, feat=8, y=P, ldy=8, flags=0):
    return lib.gnn_spmm_csr_bf16(rowptr, P, P, n_rows, x, ldx, feat, None, y, ldy, *_plan_tail(),
                                 None, flags, None)


def _hub(lib, xh=P, ldh=8, xh_f32=0, n_rows=10, ldx=8, flags=0):
    return lib.gnn_spmm_csr_hub_bf16(P, P, P, n_rows, P, ldx, xh, ldh, xh_f32, 8, None, P, 8,
                                     *_plan_tail(), None, flags, None)


def _tasks(lib, n_task=1, task_row=P, mid_row=P, xh=None, xh_f32=0, n_rows=10, ldx=8, flags=0,
           rowptr=P):
    return lib.gnn_spmm_csr_tasks_bf16(rowptr, P, P, n_rows, P, ldx, xh, 8, xh_f32, 8, None, P, 8,
                                       8, None, None, 0, None, None, 0, mid_row, 0, task_row,
                                       n_task, None, flags, None)


def test_spmm_argument_rejection(lib):
    assert _plain(lib, rowptr=None) == E_ARG
    assert _plain(lib, x=None) == E_ARG
    assert _plain(lib, y=None) == E_ARG
    assert _plain(lib, n_rows=-1) == E_ARG
    assert _plain(lib, feat=-2) == E_ARG
    assert _plain(lib, ldx=7) == E_ARG          # ldx < feat
    assert _plain(lib, ldy=4) == E_ARG
    assert _plain(lib, flags=0x100) == E_ARG    # unknown epilogue flag
    assert _hub(lib, xh=None) == E_ARG
    assert _hub(lib, ldh=4) == E_ARG            # ldh < feat
    assert _hub(lib, xh_f32=2) == E_ARG
    assert _hub(lib, n_rows=-1) == E_ARG
    assert _hub(lib, ldx=7) == E_ARG
    assert _hub(lib, flags=0x100) == E_ARG
    assert _tasks(lib, n_task=-1) == E_ARG
    assert _tasks(lib, task_row=None) == E_ARG
    assert _tasks(lib, mid_row=None) == E_ARG
    assert _tasks(lib, xh_f32=7) == E_ARG
    assert _tasks(lib, rowptr=None) == E_ARG
    assert _tasks(lib, n_rows=-3) == E_ARG
    assert _tasks(lib, ldx=7) == E_ARG
    assert _tasks(lib, flags=0x100) == E_ARG


def test_gather_and_transform_argument_rejection(lib):
    g = lib.gnn_gather_rows_bf16
    assert g(P, 8, 10, P, -1, 8, P, 8, P, None) == E_ARG
    assert g(P, 8, -1, P, 4, 8, P, 8, P, None) == E_ARG
    assert g(None, 8, 10, P, 4, 8, P, 8, P, None) == E_ARG
    assert g(P, 8, 10, None, 4, 8, P, 8, P, None) == E_ARG
    assert g(P, 8, 10, P, 4, 8, P, 8, None, None) == E_ARG   # no error flag
    assert g(P, 4, 10, P, 4, 8, P, 8, P, None) == E_ARG      # ldx < feat
    assert g(P, 8, 10, P, 0, 8, P, 8, P, None) == 0          # nothing to copy
    t = lib.gnn_gcn_transform_bf16out
    assert t(P, 100, 10, 100, P, 72, P, 72, None) == E_UNSUPPORTED   # k = 100 is not covered
    assert t(P, 128, 10, 128, P, 7, P, 8, None) == E_UNSUPPORTED     # a 7-class layer
    assert t(P, 64, 10, 128, P, 128, P, 128, None) == E_ARG          # ldx < k
    assert t(P, 128, -1, 128, P, 128, P, 128, None) == E_ARG
    assert t(None, 128, 10, 128, P, 128, P, 128, None) == E_ARG
    r = lib.gnn_gcn_transform_rows_bf16out
    assert r(P, 128, 10, 128, P, 128, P, 128, None, 10, P, None) == E_ARG   # no row ids
    assert r(P, 128, 10, 128, P, 128, P, 128, P, 0, P, None) == E_ARG       # no output rows
    assert r(P, 128, 10, 128, P, 128, P, 128, P, 10, None, None) == E_ARG   # no error flag
    assert r(P, 100, 10, 100, P, 72, P, 72, P, 10, P, None) == E_UNSUPPORTED


def test_python_layer_without_gpu():
    import torch
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.graph import CsrGraph
    g = CsrGraph(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                 torch.zeros(0), 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spmm_forward(g, torch.zeros(2, 4, dtype=torch.bfloat16))
    # the support-dtype knob: set, nested, restored; other dtypes refused
    assert ops.SUPPORT_DTYPE == torch.float32
    with ops.support_dtype(torch.bfloat16):
        assert ops.SUPPORT_DTYPE == torch.bfloat16
        with ops.support_dtype(torch.float32):
            assert ops.SUPPORT_DTYPE == torch.float32
        assert ops.SUPPORT_DTYPE == torch.bfloat16
    assert ops.SUPPORT_DTYPE == torch.float32
    with pytest.raises(TypeError):
        with ops.support_dtype(torch.float16):
            pass
    # the hub thresholds on the table's real bytes, the row caps shared between the dtypes
    n, F = 1_000_000, 64
    assert n * 4 * F >= ops.HUB_MIN_X_BYTES > n * 2 * F
    assert ops.hub_rows_for(n, F) == ops.hub_rows_for(n, F, 4) > 0
    assert ops.hub_rows_for(n, F, 2) == 0 and ops.xcd_hub_rows_for(n, F, 2) == 0
    assert ops.hub_rows_for(4 * n, F, 2) == ops.hub_rows_for(4 * n, F)
    assert ops.xcd_hub_rows_for(4 * n, F, 2) == ops.xcd_hub_rows_for(4 * n, F)
