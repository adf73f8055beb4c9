"""The supervised head's entries of the C-ABI (csrc/sup_head.hip: the selection's multiplicity,
the masked cross entropy with the count of correct predictions, the adjoint): exported, declared
to ctypes, and rejecting bad arguments before anything reaches a device; the ops refuse CPU
tensors and ``loss.supervised_loss`` / ``loss.accuracy`` on CPU tensors are torch's expressions
(no GPU needed)."""
import pytest
import torch
import torch.nn.functional as F

from graphneuralnetwork_amd import loss as L

NEW = ("gnn_sup_head_supported", "gnn_sup_head_workspace_bytes", "gnn_sup_head_count_index",
       "gnn_sup_head_count_mask", "gnn_sup_head_fwd_f32", "gnn_sup_head_bwd_f32")
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


def test_supported_widths(lib):
    sup = lib.gnn_sup_head_supported
    assert [c for c in range(-3, 200) if sup(c)] == list(range(2, 65))
    assert not sup(1 << 20) and not sup(-64)


def _cnt(lib, index=P, n=5, N=9, count=P, status=P):
    return lib.gnn_sup_head_count_index(index, n, N, count, status, None)


def _msk(lib, mask=P, N=9, count=P):
    return lib.gnn_sup_head_count_mask(mask, N, count, None)


def _fw(lib, z=P, ldz=7, labels=P, index=None, count=None, n=9, N=9, C=7, ignore=-100, loss=P,
        n_correct=P, inv_valid=P, status=P, ws=P, ws_bytes=BIG):
    return lib.gnn_sup_head_fwd_f32(z, ldz, labels, index, count, n, N, C, ignore, loss,
                                    n_correct, inv_valid, status, ws, ws_bytes, None)


def _bw(lib, z=P, ldz=7, labels=P, count=P, N=9, C=7, ignore=-100, upstream=P, inv_valid=P,
        status=P, dz=P, lddz=7):
    return lib.gnn_sup_head_bwd_f32(z, ldz, labels, count, N, C, ignore, upstream, inv_valid,
                                    status, dz, lddz, None)


def test_count_argument_rejection(lib):
    f = lambda **kw: _cnt(lib, **kw)  # noqa: E731
    for name in ("index", "count", "status"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("n", "N"):
        assert f(**{name: -1}) == E_ARG, name
    assert f(n=1 << 31) == E_UNSUPPORTED            # a multiplicity fits int32
    assert f(index=P + 4) == E_ALIGN and f(count=P + 2) == E_ALIGN and f(status=P + 2) == E_ALIGN
    assert f(N=0) == OK and f(N=0, n=0, index=None, count=None, status=None) == OK
    g = lambda **kw: _msk(lib, **kw)  # noqa: E731
    assert g(mask=None) == E_ARG and g(count=None) == E_ARG and g(N=-1) == E_ARG
    assert g(count=P + 2) == E_ALIGN
    assert g(N=0) == OK and g(N=0, mask=None, count=None) == OK


def test_forward_argument_rejection(lib):
    f = lambda **kw: _fw(lib, **kw)  # noqa: E731
    ws = lib.gnn_sup_head_workspace_bytes
    for name in ("z", "labels", "loss", "inv_valid", "status", "ws"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("n", "N", "C"):
        assert f(**{name: -1}) == E_ARG, name
    assert f(ldz=6) == E_ARG                        # a pitch below C
    assert f(n=5) == E_ARG                          # no index: the items are the N rows
    assert f(index=P, count=P, n=5) == E_ARG        # the selection is given once
    for C in (0, 1, 65, 128):
        assert f(C=C, ldz=128) == E_UNSUPPORTED, C
    assert f(z=P + 2) == E_ALIGN and f(loss=P + 2) == E_ALIGN and f(status=P + 2) == E_ALIGN
    assert f(labels=P + 4) == E_ALIGN and f(index=P + 4, n=5) == E_ALIGN
    assert f(count=P + 2) == E_ALIGN and f(n_correct=P + 4) == E_ALIGN
    assert f(inv_valid=P + 4) == E_ALIGN and f(ws=P + 4) == E_ALIGN
    assert ws(-1) == E_ARG
    sizes = [ws(n) for n in (0, 1, 150, 1024, 1025, 100_000, 1 << 20, 1 << 30, 1 << 40)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] > sizes[0]
    assert f(n=8192, N=8192, ws_bytes=ws(8192) - 1) == E_ARG and f(ws_bytes=0) == E_ARG
    # nothing selected: nothing launched, the mean of nothing is the caller's
    assert f(index=P, n=0) == OK and f(n=0, N=0) == OK
    assert f(n=0, N=0, z=None, labels=None, loss=None, n_correct=None, inv_valid=None,
             status=None, ws=None, ws_bytes=0) == OK


def test_backward_argument_rejection(lib):
    f = lambda **kw: _bw(lib, **kw)  # noqa: E731
    for name in ("z", "labels", "upstream", "inv_valid", "status", "dz"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("N", "C"):
        assert f(**{name: -1}) == E_ARG, name
    assert f(ldz=6) == E_ARG and f(lddz=6) == E_ARG  # a pitch below C
    for C in (0, 1, 65, 128):
        assert f(C=C, ldz=128, lddz=128) == E_UNSUPPORTED, C
    for name in ("z", "count", "upstream", "status", "dz"):
        assert f(**{name: P + 2}) == E_ALIGN, name
    assert f(labels=P + 4) == E_ALIGN and f(inv_valid=P + 4) == E_ALIGN
    assert f(N=0) == OK
    assert f(N=0, z=None, labels=None, count=None, upstream=None, inv_valid=None, status=None,
             dz=None) == OK


def test_ops_refuse_cpu_tensors():
    from graphneuralnetwork_amd import ops
    z, y, idx = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), torch.tensor([0, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sup_head_count(idx, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sup_head_forward(z, y, idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sup_head_backward(z, y, None, torch.ones(1), torch.ones(1, dtype=torch.float64),
                              torch.zeros(1, dtype=torch.int32))


def _ref_accuracy(y_hat, y):  # GCN/train_eval.py:9-17
    if len(y_hat.shape) > 1 and y_hat.shape[1] > 1:
        y_hat = torch.argmax(y_hat, axis=1)
    cmp = y_hat.to(dtype=y.dtype) == y
    cmp = cmp.to(dtype=y.dtype)
    return float(cmp.sum()) / len(cmp)


@pytest.mark.parametrize("kind", ["none", "index", "mask"])
def test_cpu_loss_and_accuracy_are_torchs(kind):
    """On CPU tensors nothing changes: the loops' expressions, bit for bit, and their
    gradients."""
    gen = torch.Generator().manual_seed(11)
    N, C = 37, 7
    out = torch.randn(N, C, generator=gen)
    labels = torch.randint(0, C, (N,), generator=gen)
    labels[3] = -100
    index = {"none": None, "index": torch.tensor([5, 3, 5, -1, 20, 5, 0]),
             "mask": torch.rand(N, generator=gen) < 0.4}[kind]
    assert L.SUPERVISED_HEAD_FUSED
    sel = (lambda t: t) if index is None else (lambda t: t[index])
    a = out.clone().requires_grad_()
    b = out.clone().requires_grad_()
    got, correct = L.supervised_loss(a, labels, index, count_correct=True)
    want = F.cross_entropy(sel(b), sel(labels))
    assert got.dim() == 0 and torch.equal(got, want)
    assert torch.equal(L.supervised_loss(a, labels, index), want)
    assert correct.dtype == torch.int64 and correct.dim() == 0
    assert torch.equal(correct, (torch.argmax(sel(out), 1) == sel(labels)).sum())
    (3 * got).backward()
    (3 * want).backward()
    assert torch.equal(a.grad, b.grad)
    assert L.accuracy(out, labels, index) == _ref_accuracy(sel(out), sel(labels))


def test_cpu_exceptions_are_torchs():
    out, labels = torch.randn(5, 3), torch.tensor([0, 1, 2, 0, 7])
    with pytest.raises(IndexError):
        L.supervised_loss(out, labels, torch.tensor([0, 9]))
    with pytest.raises(IndexError):  # torch's own check of the target
        L.supervised_loss(out, labels)
    empty = L.supervised_loss(out, labels, torch.zeros(0, dtype=torch.int64))
    assert empty.dim() == 0 and torch.isnan(empty)
