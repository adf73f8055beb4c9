"""The MAXPOOL training-SageLayer entries of the C-ABI (sage_kernels.hpp's winner-recording concat
gather, sage_bwd.hip's masked scatter): exported, declared to ctypes, and rejecting bad arguments
before anything reaches a device (no GPU needed)."""
import pytest

NEW = ("gnn_sage_gather_concat_arg_supported", "gnn_sage_gather_concat_arg_f32",
       "gnn_sage_gather_concat_arg_bf16", "gnn_sage_scatter_concat_maxpool_workspace_bytes",
       "gnn_sage_scatter_concat_maxpool_f32")
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


def _ga(lib, bf16=False, table=P, ldt=8, n_table=100, cidx=P, idx=P, ldi=10, M=4, k=10, feat=8,
        self_out=P, ld_self=16, out=P + 32, ldo=16, arg=P, lda=8, err=P):
    fn = lib.gnn_sage_gather_concat_arg_bf16 if bf16 else lib.gnn_sage_gather_concat_arg_f32
    return fn(table, ldt, n_table, cidx, idx, ldi, M, k, feat, self_out, ld_self, out, ldo, arg,
              lda, err, None)


def _sc(lib, dbuf=P, ldd=16, arg=P, lda=8, ptr=P, slot=P, M=4, k=10, feat=8, n_prev=100, dx=P,
        ldx=8, ws=P, ws_bytes=BIG):
    return lib.gnn_sage_scatter_concat_maxpool_f32(dbuf, ldd, arg, lda, ptr, slot, M, k, feat,
                                                   n_prev, dx, ldx, ws, ws_bytes, None)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_gather_argument_rejection(lib, bf16):
    g = lambda **kw: _ga(lib, bf16, **kw)  # noqa: E731
    for name in ("table", "cidx", "idx", "self_out", "out", "arg", "err"):
        assert g(**{name: None}) == E_ARG, name
    for name in ("M", "k", "feat", "n_table"):
        assert g(**{name: -1}) == E_ARG, name
    assert g(k=0) == E_UNSUPPORTED
    assert g(k=256, ldi=256) == E_UNSUPPORTED
    assert g(feat=2, ldt=8) == E_UNSUPPORTED
    assert g(feat=36, ldt=40, ld_self=72, ldo=72, lda=36) == E_UNSUPPORTED
    assert g(feat=512, ldt=512, ld_self=1024, ldo=1024, lda=512) == E_UNSUPPORTED
    # one 16-B lane is 4 fp32 but 8 bf16: F = 4 is the fp32 entry's alone
    assert g(feat=4, M=0) == (E_UNSUPPORTED if bf16 else OK)
    assert g(ldt=7) == E_ARG       # a pitch below its row
    assert g(ldo=7) == E_ARG
    assert g(ld_self=7) == E_ARG
    assert g(lda=7) == E_ARG       # lda < F
    assert g(ldi=9) == E_ARG       # ldi < k
    assert g(table=P + 4) == E_ALIGN
    assert g(out=P + 4) == E_ALIGN
    assert g(self_out=P + 8) == E_ALIGN
    assert g(arg=P + 2) == E_ALIGN
    assert g(lda=10) == E_ALIGN
    assert g(ldo=18) == E_ALIGN
    assert g(ldt=12 if bf16 else 10) == E_ALIGN  # whole 16-B lanes per table row
    assert g(M=0) == OK            # no row to write: nothing launched


def test_scatter_argument_rejection(lib):
    for name in ("dbuf", "arg", "ptr", "slot", "dx", "ws"):
        assert _sc(lib, **{name: None}) == E_ARG, name
    for name in ("M", "k", "feat", "n_prev"):
        assert _sc(lib, **{name: -1}) == E_ARG, name
    assert _sc(lib, k=0) == E_UNSUPPORTED
    assert _sc(lib, k=256) == E_UNSUPPORTED
    assert _sc(lib, feat=2, ldd=4, ldx=4, lda=4) == E_UNSUPPORTED
    assert _sc(lib, feat=36, ldd=72, ldx=36, lda=36) == E_UNSUPPORTED  # F / 4 not a power of two
    assert _sc(lib, feat=512, ldd=1024, ldx=512, lda=512) == E_UNSUPPORTED
    assert _sc(lib, M=1 << 28, k=7) == E_UNSUPPORTED                   # 2^31 slots
    assert _sc(lib, lda=7) == E_ARG                   # lda < F
    assert _sc(lib, lda=4) == E_ARG
    assert _sc(lib, ldd=15) == E_ARG                  # ldd < 2 F
    assert _sc(lib, ldx=7) == E_ARG
    assert _sc(lib, ws_bytes=16) == E_ARG
    assert _sc(lib, dbuf=P + 4) == E_ALIGN
    assert _sc(lib, dx=P + 8) == E_ALIGN
    assert _sc(lib, ldd=18) == E_ALIGN
    assert _sc(lib, arg=P + 1) == E_ALIGN
    assert _sc(lib, lda=10) == E_ALIGN
    assert _sc(lib, n_prev=0) == OK                   # no row to write: nothing launched


def test_supported_shapes(lib):
    sup = lib.gnn_sage_gather_concat_arg_supported
    widths = [4, 8, 16, 32, 64, 128, 256]
    for k in (1, 2, 10, 25, 254, 255):
        assert [f for f in range(0, 600) if sup(f, k)] == widths, k
    for k in (-1, 0, 256, 257, 300, 1 << 20):
        assert not any(sup(f, k) for f in range(0, 600)), k
    assert [k for k in range(-2, 300) if sup(128, k)] == list(range(1, 256))


def test_workspace_query(lib):
    q, mean = (lib.gnn_sage_scatter_concat_maxpool_workspace_bytes,
               lib.gnn_sage_scatter_concat_workspace_bytes)
    for M in (0, 1, 7, 1000, 245760):
        assert q(M, 25, 128) == mean(M, 25, 128) > 0   # the MEAN scatter's layout
    assert q(-1, 3, 8) == E_ARG and q(3, -1, 8) == E_ARG and q(3, 3, -1) == E_ARG
    assert q(100, 0, 8) == E_UNSUPPORTED and q(100, 256, 8) == E_UNSUPPORTED
    assert q(100, 5, 36) == E_UNSUPPORTED and q(1 << 28, 7, 8) == E_UNSUPPORTED


def test_python_layer_without_gpu():
    import torch
    from graphneuralnetwork_amd import ops
    cidx = torch.zeros(3, dtype=torch.int64)
    idx = torch.zeros(3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_gather_concat_arg(torch.zeros(4, 8), cidx, idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_gather_concat_arg(torch.zeros(4, 8).bfloat16(), cidx, idx)
    tr = ops.SageMapsT(torch.zeros(5, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_scatter_concat_maxpool(torch.zeros(3, 16), torch.zeros(3, 8, dtype=torch.uint8),
                                        tr, 4)
    t, w = torch.zeros(4, 64), torch.zeros(128, 128)
    assert not ops.sage_train_layer_supported(t, w, 5, agg='MAXPOOL')
    assert not ops.sage_train_layer_supported(t, w, 5, 'MEAN')
    assert not ops.sage_train_layer_supported(t, w, 5)
