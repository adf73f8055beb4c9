"""The GraphSAGE bf16 entries of the C-ABI: exported, declared to ctypes, and rejecting bad
arguments before anything reaches a device (no GPU needed)."""
import pytest

NEW = ("gnn_sage_aggregate_bf16", "gnn_sage_gather_aggregate_bf16", "gnn_sage_gather_concat_bf16",
       "gnn_sage_gather_concat_live_bf16", "gnn_gather_rows_bf16_f32")
OK, E_ARG, E_UNSUPPORTED = 0, -1, -3
MEAN, ARGMAX, SUM, MAXPOOL, ARGMAX_F32 = 0, 1, 2, 3, 4
P = 4096  # a non-null pointer value; never dereferenced: every call below returns at its checks


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


def test_symbols_load(lib):
    from graphneuralnetwork_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), f"{name} not exported"
        twin = name.replace("_bf16_f32", "_f32") if name.endswith("_bf16_f32") else \
            name.replace("_bf16", "_f32")
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]  # the _f32 twin's argument list


def _pre(lib, neigh=P, ld_k=8, ld_m=80, M=4, k=10, feat=8, mode=MEAN, out=P, ldo=8):
    return lib.gnn_sage_aggregate_bf16(neigh, ld_k, ld_m, M, k, feat, mode, out, ldo, None)


def _gather(lib, table=P, ldt=8, n_table=100, idx=P, ldi=10, M=4, k=10, feat=8, mode=MEAN, out=P,
            ldo=8, err=P):
    return lib.gnn_sage_gather_aggregate_bf16(table, ldt, n_table, idx, ldi, M, k, feat, mode, out,
                                              ldo, err, None)


def _concat(lib, live=False, table=P, ldt=8, n_table=100, self_idx=P, idx=P, ldi=10, M=4, k=10,
            feat=8, mode=MEAN, self_out=P, ld_self=16, out=P, ldo=16, err=P):
    if live:
        return lib.gnn_sage_gather_concat_live_bf16(table, ldt, n_table, self_idx, idx, ldi, M,
                                                    None, k, feat, mode, self_out, ld_self, out,
                                                    ldo, err, None)
    return lib.gnn_sage_gather_concat_bf16(table, ldt, n_table, self_idx, idx, ldi, M, k, feat,
                                           mode, self_out, ld_self, out, ldo, err, None)


def _rows(lib, x=P, ldx=8, n_x=100, idx=P, n=4, feat=8, out=P, ldo=8, err=P):
    return lib.gnn_gather_rows_bf16_f32(x, ldx, n_x, idx, n, feat, out, ldo, err, None)


def test_pregathered_argument_rejection(lib):
    assert _pre(lib, neigh=None) == E_ARG
    assert _pre(lib, out=None) == E_ARG
    assert _pre(lib, M=-1) == E_ARG
    assert _pre(lib, k=-1) == E_ARG
    assert _pre(lib, feat=-1) == E_ARG
    assert _pre(lib, ld_k=7) == E_ARG           # ld_k < feat
    assert _pre(lib, ldo=7) == E_ARG
    assert _pre(lib, mode=ARGMAX_F32) == E_ARG  # the concat entries only
    assert _pre(lib, mode=-1) == E_ARG
    assert _pre(lib, k=0) == E_UNSUPPORTED
    assert _pre(lib, M=0) == OK
    assert _pre(lib, feat=0) == OK


def test_gather_argument_rejection(lib):
    assert _gather(lib, table=None) == E_ARG
    assert _gather(lib, idx=None) == E_ARG
    assert _gather(lib, out=None) == E_ARG
    assert _gather(lib, err=None) == E_ARG
    assert _gather(lib, M=-1) == E_ARG
    assert _gather(lib, k=-1) == E_ARG
    assert _gather(lib, feat=-1) == E_ARG
    assert _gather(lib, n_table=-1) == E_ARG
    assert _gather(lib, ldt=7) == E_ARG         # ldt < feat
    assert _gather(lib, ldi=9) == E_ARG         # ldi < k
    assert _gather(lib, ldo=7) == E_ARG
    assert _gather(lib, mode=ARGMAX_F32) == E_ARG
    assert _gather(lib, mode=5) == E_ARG
    assert _gather(lib, k=0, ldi=0) == E_UNSUPPORTED
    assert _gather(lib, M=0) == OK
    assert _gather(lib, feat=0) == OK


@pytest.mark.parametrize("live", [False, True])
def test_concat_argument_rejection(lib, live):
    c = lambda **kw: _concat(lib, live, **kw)  # noqa: E731
    assert c(table=None) == E_ARG
    assert c(self_idx=None) == E_ARG
    assert c(idx=None) == E_ARG
    assert c(self_out=None) == E_ARG
    assert c(out=None) == E_ARG
    assert c(err=None) == E_ARG
    assert c(M=-1) == E_ARG
    assert c(k=-1) == E_ARG
    assert c(feat=-1) == E_ARG
    assert c(n_table=-1) == E_ARG
    assert c(ldt=7) == E_ARG
    assert c(ldi=9) == E_ARG
    assert c(ldo=7) == E_ARG
    assert c(ld_self=7) == E_ARG
    assert c(mode=ARGMAX) == E_ARG              # int64 argmax has no concat form
    assert c(mode=7) == E_ARG
    assert c(k=0, ldi=0) == E_UNSUPPORTED
    assert c(M=0) == OK
    assert c(feat=0) == OK


def test_widening_gather_argument_rejection(lib):
    assert _rows(lib, x=None) == E_ARG
    assert _rows(lib, idx=None) == E_ARG
    assert _rows(lib, out=None) == E_ARG
    assert _rows(lib, err=None) == E_ARG
    assert _rows(lib, n=-1) == E_ARG
    assert _rows(lib, feat=-1) == E_ARG
    assert _rows(lib, n_x=-1) == E_ARG
    assert _rows(lib, ldx=7) == E_ARG
    assert _rows(lib, ldo=7) == E_ARG
    assert _rows(lib, n=0) == OK
    assert _rows(lib, feat=0) == OK


def test_python_layer_without_gpu():
    import torch
    from graphneuralnetwork_amd import ops
    t = torch.zeros(6, 8, dtype=torch.bfloat16)
    idx = torch.zeros(3, 2, dtype=torch.int64)
    sid = torch.zeros(3, dtype=torch.int64)
    for call in (lambda x: ops.sage_gather_aggregate(x, idx),
                 lambda x: ops.sage_gather_concat(x, sid, idx),
                 lambda x: ops.gather_rows(x, sid),
                 lambda x: ops.sage_aggregate(x[idx])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t)
        with pytest.raises(TypeError):
            call(t.to(torch.float16))
    tg = t.clone().requires_grad_(True)
    with torch.enable_grad(), pytest.raises(TypeError, match="inference only"):
        from graphneuralnetwork_amd.graphsage import Gathered, reduce_neighbors
        reduce_neighbors(Gathered(tg, idx), "MEAN")
