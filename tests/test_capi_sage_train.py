"""The training-SageLayer entries of the C-ABI (sage_bwd.hip): exported, declared to ctypes, and
rejecting bad arguments before anything reaches a device (no GPU needed)."""
import pytest

NEW = ("gnn_sage_maps_transpose_workspace_bytes", "gnn_sage_maps_transpose",
       "gnn_sage_scatter_concat_supported", "gnn_sage_scatter_concat_workspace_bytes",
       "gnn_sage_scatter_concat_f32")
OK, E_ARG, E_ALIGN, E_UNSUPPORTED = 0, -1, -2, -3
P = 4096  # a non-null, 16-B aligned pointer value; never dereferenced: every call returns first
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


def test_symbols_load(lib):
    from graphneuralnetwork_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), f"{name} not exported"


def _tr(lib, cidx=P, idx=P, ldi=10, M=4, k=10, n_prev=100, ptr=P, slot=P, err=P, ws=P,
        ws_bytes=BIG):
    return lib.gnn_sage_maps_transpose(cidx, idx, ldi, M, k, n_prev, ptr, slot, err, ws, ws_bytes,
                                       None)


def _sc(lib, dbuf=P, ldd=16, ptr=P, slot=P, M=4, k=10, feat=8, n_prev=100, dx=P, ldx=8, ws=P,
        ws_bytes=BIG):
    return lib.gnn_sage_scatter_concat_f32(dbuf, ldd, ptr, slot, M, k, feat, n_prev, dx, ldx, ws,
                                           ws_bytes, None)


def test_transpose_argument_rejection(lib):
    assert _tr(lib, cidx=None) == E_ARG
    assert _tr(lib, idx=None) == E_ARG
    assert _tr(lib, ptr=None) == E_ARG
    assert _tr(lib, slot=None) == E_ARG
    assert _tr(lib, err=None) == E_ARG
    assert _tr(lib, ws=None) == E_ARG
    assert _tr(lib, M=-1) == E_ARG
    assert _tr(lib, k=-1) == E_ARG
    assert _tr(lib, n_prev=-1) == E_ARG
    assert _tr(lib, ldi=9) == E_ARG                   # ldi < k
    assert _tr(lib, ws_bytes=16) == E_ARG             # below the workspace query
    assert _tr(lib, M=1 << 28, k=7) == E_UNSUPPORTED  # M (k + 1) = 2^31 slots
    assert _tr(lib, n_prev=2 ** 31 - 1) == E_UNSUPPORTED


def test_scatter_argument_rejection(lib):
    assert _sc(lib, dbuf=None) == E_ARG
    assert _sc(lib, ptr=None) == E_ARG
    assert _sc(lib, slot=None) == E_ARG
    assert _sc(lib, dx=None) == E_ARG
    assert _sc(lib, ws=None) == E_ARG
    assert _sc(lib, M=-1) == E_ARG
    assert _sc(lib, k=-1) == E_ARG
    assert _sc(lib, feat=-1) == E_ARG
    assert _sc(lib, n_prev=-1) == E_ARG
    assert _sc(lib, ldd=15) == E_ARG                  # ldd < 2 F
    assert _sc(lib, ldx=7) == E_ARG                   # ldx < F
    assert _sc(lib, ws_bytes=16) == E_ARG
    assert _sc(lib, feat=36, ldd=72, ldx=36) == E_UNSUPPORTED   # F / 4 not a power of two
    assert _sc(lib, feat=512, ldd=1024, ldx=512) == E_UNSUPPORTED
    assert _sc(lib, feat=2, ldd=4, ldx=4) == E_UNSUPPORTED
    assert _sc(lib, M=1 << 28, k=7) == E_UNSUPPORTED
    assert _sc(lib, dbuf=P + 4) == E_ALIGN
    assert _sc(lib, dx=P + 8) == E_ALIGN
    assert _sc(lib, ldd=18) == E_ALIGN
    assert _sc(lib, n_prev=0) == OK                   # no row to write: nothing launched


def test_supported_widths(lib):
    ok = [f for f in range(0, 600) if lib.gnn_sage_scatter_concat_supported(f)]
    assert ok == [4, 8, 16, 32, 64, 128, 256]


def test_workspace_queries(lib):
    tq, sq = lib.gnn_sage_maps_transpose_workspace_bytes, lib.gnn_sage_scatter_concat_workspace_bytes
    sizes = [0, 1, 7, 1000, 8192, 245760, 4_200_000]
    t = [tq(M, 25) for M in sizes]
    s = [sq(M, 25, 128) for M in sizes]
    for q in (t, s):
        assert all(v > 0 for v in q)
        assert all(a <= b for a, b in zip(q, q[1:])) and q[0] < q[-1]  # monotone in M
    assert tq(-1, 3) == E_ARG and tq(3, -1) == E_ARG
    assert sq(-1, 3, 8) == E_ARG and sq(3, -1, 8) == E_ARG and sq(3, 3, -1) == E_ARG
    assert tq(1 << 28, 7) == E_UNSUPPORTED and sq(1 << 28, 7, 8) == E_UNSUPPORTED
    assert sq(100, 5, 36) == E_UNSUPPORTED


def test_python_layer_without_gpu():
    import torch
    from graphneuralnetwork_amd import ops
    cidx = torch.zeros(3, dtype=torch.int64)
    idx = torch.zeros(3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_maps_transpose(cidx, idx, 4)
    tr = ops.SageMapsT(torch.zeros(5, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_scatter_concat(torch.zeros(3, 16), tr, 4)
    assert not ops.sage_train_layer_supported(torch.zeros(4, 64), torch.zeros(128, 128), 5)
