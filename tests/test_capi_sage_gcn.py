"""The gcn-mode SageLayer entries of the C-ABI (sage_kernels.hpp's aggregate-only gathers: the live
form and the winner-recording form; sage_bwd.hip's transpose of the neighbour map alone and the
adjoint of the gcn gather): exported, declared to ctypes, and rejecting bad arguments before
anything reaches a device (no GPU needed)."""
import pytest

NEW = ("gnn_sage_gather_aggregate_live_f32", "gnn_sage_gather_aggregate_live_bf16",
       "gnn_sage_gather_aggregate_arg_supported", "gnn_sage_gather_aggregate_arg_f32",
       "gnn_sage_gather_aggregate_arg_bf16", "gnn_sage_maps_transpose_nbr_workspace_bytes",
       "gnn_sage_maps_transpose_nbr", "gnn_sage_scatter_agg_workspace_bytes",
       "gnn_sage_scatter_agg_f32", "gnn_sage_scatter_agg_maxpool_workspace_bytes",
       "gnn_sage_scatter_agg_maxpool_f32")
OK, E_ARG, E_ALIGN, E_UNSUPPORTED = 0, -1, -2, -3
P = 4096  # a non-null, 16-B aligned pointer value; never dereferenced: every call returns first
BIG = 1 << 40
MEAN, ARGMAX, SUM, MAXPOOL, ARGMAX_F32 = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


def test_symbols_load(lib):
    from graphneuralnetwork_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), f"{name} not exported"


def _ga(lib, bf16=False, table=P, ldt=8, n_table=100, idx=P, ldi=10, M=4, k=10, feat=8, out=P,
        ldo=8, arg=P, lda=8, err=P):
    fn = lib.gnn_sage_gather_aggregate_arg_bf16 if bf16 else lib.gnn_sage_gather_aggregate_arg_f32
    return fn(table, ldt, n_table, idx, ldi, M, k, feat, out, ldo, arg, lda, err, None)


def _gl(lib, bf16=False, table=P, ldt=8, n_table=100, idx=P, ldi=10, M=4, live=P, k=10, feat=8,
        mode=MEAN, out=P, ldo=8, err=P):
    fn = (lib.gnn_sage_gather_aggregate_live_bf16 if bf16 else
          lib.gnn_sage_gather_aggregate_live_f32)
    return fn(table, ldt, n_table, idx, ldi, M, live, k, feat, mode, out, ldo, err, None)


def _tr(lib, idx=P, ldi=10, M=4, k=10, n_prev=100, ptr=P, slot=P, err=P, ws=P, ws_bytes=BIG):
    return lib.gnn_sage_maps_transpose_nbr(idx, ldi, M, k, n_prev, ptr, slot, err, ws, ws_bytes,
                                           None)


def _sc(lib, dbuf=P, ldd=8, ptr=P, slot=P, M=4, k=10, feat=8, n_prev=100, dx=P, ldx=8, ws=P,
        ws_bytes=BIG):
    return lib.gnn_sage_scatter_agg_f32(dbuf, ldd, ptr, slot, M, k, feat, n_prev, dx, ldx, ws,
                                        ws_bytes, None)


def _sm(lib, dbuf=P, ldd=8, arg=P, lda=8, ptr=P, slot=P, M=4, k=10, feat=8, n_prev=100, dx=P,
        ldx=8, ws=P, ws_bytes=BIG):
    return lib.gnn_sage_scatter_agg_maxpool_f32(dbuf, ldd, arg, lda, ptr, slot, M, k, feat,
                                                n_prev, dx, ldx, ws, ws_bytes, None)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_arg_gather_argument_rejection(lib, bf16):
    g = lambda **kw: _ga(lib, bf16, **kw)  # noqa: E731
    for name in ("table", "idx", "out", "arg", "err"):
        assert g(**{name: None}) == E_ARG, name
    for name in ("M", "k", "feat", "n_table"):
        assert g(**{name: -1}) == E_ARG, name
    assert g(k=0) == E_UNSUPPORTED
    assert g(k=256, ldi=256) == E_UNSUPPORTED
    assert g(feat=2, ldt=8) == E_UNSUPPORTED
    assert g(feat=36, ldt=40, ldo=36, lda=36) == E_UNSUPPORTED
    assert g(feat=512, ldt=512, ldo=512, lda=512) == E_UNSUPPORTED
    # one 16-B lane is 4 fp32 but 8 bf16: F = 4 is the fp32 entry's alone
    assert g(feat=4, M=0) == (E_UNSUPPORTED if bf16 else OK)
    assert g(ldt=7) == E_ARG       # a pitch below its row
    assert g(ldo=7) == E_ARG
    assert g(lda=7) == E_ARG       # lda < F
    assert g(ldi=9) == E_ARG       # ldi < k
    assert g(table=P + 4) == E_ALIGN
    assert g(out=P + 4) == E_ALIGN
    assert g(arg=P + 2) == E_ALIGN
    assert g(lda=10) == E_ALIGN
    assert g(ldo=10) == E_ALIGN
    assert g(ldt=12 if bf16 else 10) == E_ALIGN  # whole 16-B lanes per table row
    assert g(M=0) == OK            # no row to write: nothing launched


def test_arg_gather_supported_shapes(lib):
    sup, cat = (lib.gnn_sage_gather_aggregate_arg_supported,
                lib.gnn_sage_gather_concat_arg_supported)
    widths = [4, 8, 16, 32, 64, 128, 256]
    for k in (1, 2, 11, 26, 254, 255):
        assert [f for f in range(0, 600) if sup(f, k)] == widths, k
    for k in (-1, 0, 256, 257, 300, 1 << 20):
        assert not any(sup(f, k) for f in range(0, 600)), k
    assert [k for k in range(-2, 300) if sup(128, k)] == list(range(1, 256))
    assert all(bool(sup(f, k)) == bool(cat(f, k)) for f in range(0, 300) for k in (0, 5, 256))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_live_gather_argument_rejection(lib, bf16):
    g = lambda **kw: _gl(lib, bf16, **kw)  # noqa: E731
    for name in ("table", "idx", "out", "err"):
        assert g(**{name: None}) == E_ARG, name
    for name in ("M", "k", "feat", "n_table"):
        assert g(**{name: -1}) == E_ARG, name
    for mode in (ARGMAX, SUM, ARGMAX_F32, -1, 5):  # MEAN and MAXPOOL only
        assert g(mode=mode) == E_ARG, mode
        assert g(mode=mode, M=0) == E_ARG, mode
    assert g(k=0) == E_UNSUPPORTED
    assert g(ldt=7) == E_ARG
    assert g(ldo=7) == E_ARG
    assert g(ldi=9) == E_ARG
    for mode in (MEAN, MAXPOOL):
        assert g(mode=mode, M=0) == OK           # no row: nothing launched, live never read
        assert g(mode=mode, M=0, live=None) == OK
        assert g(mode=mode, feat=0, ldt=0, ldo=0) == OK


def test_transpose_argument_rejection(lib):
    for name in ("idx", "ptr", "slot", "err", "ws"):
        assert _tr(lib, **{name: None}) == E_ARG, name
    for name in ("M", "k", "n_prev"):
        assert _tr(lib, **{name: -1}) == E_ARG, name
    assert _tr(lib, ldi=9) == E_ARG                       # ldi < k
    assert _tr(lib, ws_bytes=16) == E_ARG
    assert _tr(lib, M=1 << 28, k=8, ldi=8) == E_UNSUPPORTED   # 2^31 slots
    assert _tr(lib, n_prev=(1 << 31) - 1) == E_UNSUPPORTED


def test_transpose_workspace_query(lib):
    q, cat = (lib.gnn_sage_maps_transpose_nbr_workspace_bytes,
              lib.gnn_sage_maps_transpose_workspace_bytes)
    assert q(-1, 3) == E_ARG and q(3, -1) == E_ARG
    for M, k in ((0, 5), (1, 1), (7, 0), (1000, 26), (245760, 11)):
        assert q(M, k) > 0
        assert q(M, k) <= cat(M, k)                       # M k slots, not M (k + 1)
    assert q(1 << 28, 8) == E_UNSUPPORTED                 # 2^31 slots
    assert q((1 << 28) - 1, 8) > 0                        # 2^31 - 8 slots
    assert q((1 << 31) - 1, 1) > 0 and q(1 << 31, 1) == E_UNSUPPORTED
    # the concat transpose, whose M (k + 1) slots overflow where M k do not, is as it was
    assert cat(1 << 28, 7) == E_UNSUPPORTED and q(1 << 28, 7) > 0


def test_scatter_argument_rejection(lib):
    for name in ("dbuf", "ptr", "slot", "dx", "ws"):
        assert _sc(lib, **{name: None}) == E_ARG, name
        assert _sm(lib, **{name: None}) == E_ARG, name
    assert _sm(lib, arg=None) == E_ARG
    for name in ("M", "k", "feat", "n_prev"):
        assert _sc(lib, **{name: -1}) == E_ARG, name
        assert _sm(lib, **{name: -1}) == E_ARG, name
    assert _sm(lib, k=0) == E_UNSUPPORTED
    assert _sm(lib, k=256) == E_UNSUPPORTED
    for f in (_sc, _sm):
        extra = {"lda": 512} if f is _sm else {}
        assert f(lib, feat=2, ldd=4, ldx=4) == E_UNSUPPORTED
        assert f(lib, feat=36, ldd=36, ldx=36, **extra) == E_UNSUPPORTED  # F / 4 not a power of 2
        assert f(lib, feat=512, ldd=512, ldx=512, **extra) == E_UNSUPPORTED
        assert f(lib, M=1 << 28, k=8) == E_UNSUPPORTED                    # 2^31 slots
        assert f(lib, ldd=7) == E_ARG                     # ldd < F
        assert f(lib, ldd=4) == E_ARG
        assert f(lib, ldx=7) == E_ARG
        assert f(lib, ws_bytes=16) == E_ARG
        assert f(lib, dbuf=P + 4) == E_ALIGN
        assert f(lib, dx=P + 8) == E_ALIGN
        assert f(lib, ldd=10) == E_ALIGN
        assert f(lib, ldx=10) == E_ALIGN
        assert f(lib, ws=P + 4) == E_ALIGN
        assert f(lib, n_prev=0) == OK                     # no row to write: nothing launched
        assert f(lib, n_prev=0, dx=None) == OK
    assert _sm(lib, lda=7) == E_ARG                       # lda < F
    assert _sm(lib, lda=4) == E_ARG
    assert _sm(lib, arg=P + 1) == E_ALIGN
    assert _sm(lib, lda=10) == E_ALIGN


def test_scatter_workspace_query(lib):
    q, qm, cat = (lib.gnn_sage_scatter_agg_workspace_bytes,
                  lib.gnn_sage_scatter_agg_maxpool_workspace_bytes,
                  lib.gnn_sage_scatter_concat_workspace_bytes)
    for M in (0, 1, 7, 1000, 245760):
        assert q(M, 26, 128) == qm(M, 26, 128) > 0        # the MEAN scatter's layout
        assert q(M, 26, 128) <= cat(M, 26, 128)
    for f in (q, qm):
        assert f(-1, 3, 8) == E_ARG and f(3, -1, 8) == E_ARG and f(3, 3, -1) == E_ARG
        assert f(100, 5, 36) == E_UNSUPPORTED and f(1 << 28, 8, 8) == E_UNSUPPORTED
        assert f(1 << 28, 7, 8) > 0                       # 7 * 2^28 slots fit
    assert qm(100, 0, 8) == E_UNSUPPORTED and qm(100, 256, 8) == E_UNSUPPORTED
    assert q(100, 0, 8) > 0 and q(100, 256, 8) > 0


def test_python_layer_without_gpu():
    import torch
    from graphneuralnetwork_amd import ops
    idx = torch.zeros(3, 2, dtype=torch.int64)
    for t in (torch.zeros(4, 8), torch.zeros(4, 8).bfloat16()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.sage_gather_aggregate_arg(t, idx)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.sage_gather_aggregate(t, idx, "MEAN", live=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_maps_transpose_nbr(idx, 4)
    tr = ops.SageMapsT(torch.zeros(5, dtype=torch.int64), torch.zeros(6, dtype=torch.int32), 3, 2,
                       False)
    assert not tr.centre
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_scatter_agg(torch.zeros(3, 8), tr, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_scatter_agg_maxpool(torch.zeros(3, 8), torch.zeros(3, 8, dtype=torch.uint8), tr,
                                     4)
    # existing callers build the concat maps as before: four fields, the centre slots first
    assert ops.SageMapsT(tr.ptr, torch.zeros(9, dtype=torch.int32), 3, 2).centre
    t, w = torch.zeros(4, 64), torch.zeros(128, 64)
    assert not ops.sage_train_layer_supported(t, w, 5, agg='MAXPOOL', gcn=True)
    assert not ops.sage_train_layer_supported(t, w, 5, 'MEAN', gcn=True)
    assert not ops.sage_train_layer_supported(t, w, 5, 'MAX', gcn=True)
