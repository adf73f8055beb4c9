"""The unsupervised head's entries of the C-ABI (csrc/sage_score.hip: the scores, their adjoint,
the binary cross entropy with logits): exported, declared to ctypes, and rejecting bad arguments
before anything reaches a device; the ops refuse CPU tensors and the model's CPU path is torch's
(no GPU needed)."""
import pytest
import torch
import torch.nn.functional as F

NEW = ("gnn_sage_score_supported", "gnn_sage_score_f32", "gnn_sage_score_bwd_f32",
       "gnn_bce_logits_workspace_bytes", "gnn_bce_logits_f32")
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
    sup = lib.gnn_sage_score_supported
    assert [h for h in range(0, 600) if sup(h)] == [4, 8, 16, 32, 64, 128, 256]
    assert not sup(-4) and not sup(1 << 20)


def _fw(lib, c=P, ldc=8, x=P, ldx=8, B=4, S=5, H=8, z=P, ldz=5):
    return lib.gnn_sage_score_f32(c, ldc, x, ldx, B, S, H, z, ldz, None)


def _bw(lib, g=P, ldg=5, c=P, ldc=8, x=P, ldx=8, B=4, S=5, H=8, dc=P, lddc=8, dx=P, lddx=8):
    return lib.gnn_sage_score_bwd_f32(g, ldg, c, ldc, x, ldx, B, S, H, dc, lddc, dx, lddx, None)


def _bce(lib, z=P, ldz=5, y=P, ldy=5, i64=0, rows=4, cols=5, loss=P, g=P, ldg=5, ws=P,
         ws_bytes=BIG):
    return lib.gnn_bce_logits_f32(z, ldz, y, ldy, i64, rows, cols, loss, g, ldg, ws, ws_bytes,
                                  None)


def test_score_argument_rejection(lib):
    f = lambda **kw: _fw(lib, **kw)  # noqa: E731
    for name in ("c", "x", "z"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("B", "S", "H"):
        assert f(**{name: -1}) == E_ARG, name
    assert f(ldc=4) == E_ARG and f(ldx=4) == E_ARG  # a pitch below H
    assert f(ldz=4) == E_ARG                        # ldz < S
    assert f(ldc=10) == E_ALIGN and f(ldx=10) == E_ALIGN
    assert f(c=P + 4) == E_ALIGN and f(x=P + 4) == E_ALIGN
    for H in (0, 2, 12, 36, 512):
        assert f(H=H, ldc=512, ldx=512) == E_UNSUPPORTED, H
    assert f(B=0) == OK and f(S=0, ldz=0) == OK     # nothing to write: nothing launched
    assert f(B=0, c=None, x=None, z=None) == OK


def test_score_bwd_argument_rejection(lib):
    f = lambda **kw: _bw(lib, **kw)  # noqa: E731
    for name in ("g", "c", "x"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("B", "S", "H"):
        assert f(**{name: -1}) == E_ARG, name
    for name in ("ldc", "ldx", "lddc", "lddx"):
        assert f(**{name: 4}) == E_ARG, name        # a pitch below H
        assert f(**{name: 10}) == E_ALIGN, name     # not a multiple of 4
    assert f(ldg=4) == E_ARG                        # ldg < S
    for name in ("c", "x", "dc", "dx"):
        assert f(**{name: P + 4}) == E_ALIGN, name
    for H in (0, 2, 12, 36, 512):
        assert f(H=H, ldc=512, ldx=512, lddc=512, lddx=512) == E_UNSUPPORTED, H
    assert f(B=0) == OK and f(S=0, ldg=0) == OK
    assert f(dc=None, dx=None) == OK                # neither half asked for
    # a half that is skipped takes its operand with it: x serves dc alone, c serves dx alone
    assert f(dc=None, x=None, B=0) == OK and f(dx=None, c=None, B=0) == OK
    assert f(dc=None, x=P + 4, ldx=3, B=0) == OK and f(dx=None, c=P + 4, ldc=3, B=0) == OK


def test_bce_argument_rejection(lib):
    f = lambda **kw: _bce(lib, **kw)  # noqa: E731
    ws = lib.gnn_bce_logits_workspace_bytes
    for name in ("z", "y", "loss", "ws"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("rows", "cols"):
        assert f(**{name: -1}) == E_ARG, name
        assert f(**{name: 0}) == E_ARG, name        # there is no mean of nothing
    for name in ("ldz", "ldy", "ldg"):
        assert f(**{name: 4}) == E_ARG, name        # a pitch below cols
    assert f(z=P + 2) == E_ALIGN and f(g=P + 2) == E_ALIGN and f(loss=P + 2) == E_ALIGN
    assert f(y=P + 4, i64=1) == E_ALIGN and f(ws=P + 4) == E_ALIGN
    assert ws(-1) == E_ARG
    sizes = [ws(n) for n in (0, 1, 150, 1024, 1025, 245_760, 1 << 20, 1 << 30, 1 << 40)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] > sizes[0]
    assert f(rows=8192, cols=30, ldz=30, ldy=30, ldg=30, ws_bytes=ws(245_760) - 1) == E_ARG
    assert f(ws_bytes=0) == E_ARG


def test_ops_refuse_cpu_tensors():
    from graphneuralnetwork_amd import ops
    c, x, g = torch.zeros(2, 8), torch.zeros(6, 8), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_score(c, x, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sage_score_backward(g, c, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bce_logits(g, torch.zeros(2, 3))


def test_cpu_model_and_loss_are_torchs():
    """On CPU tensors nothing changes: the unsupervised forward ends in torch.bmm and
    unsupervised_loss is torch's function, bit for bit. (The towers' layers have no CPU path,
    so a tower here hands its first argument on as the embeddings; the head is the model's.)"""
    from graphneuralnetwork_amd import graphsage as G

    class Head(G.GraphSAGE):
        def forward(self, a, b, c, d, e, *rest):
            if e is None:
                return a, None
            return super().forward(a, b, c, d, e, *rest)

    gen = torch.Generator().manual_seed(3)
    shape = (6, 5)
    net = Head(2, 8, 16, False, agg_func="MEAN", Unsupervised=True)
    emb0 = torch.randn(6, 16, generator=gen, requires_grad=True)
    second = torch.randn(30, 16, generator=gen, requires_grad=True)
    assert G.SAGE_SCORE_FUSED
    emb, scores = net(emb0, None, None, None, second, None, None, None, shape)
    ref = torch.bmm(emb0.unsqueeze(1), second.reshape(*shape, -1).permute(0, 2, 1))
    assert emb is emb0 and scores.shape == (6, 1, 5) and torch.equal(scores, ref)
    scores = scores.detach()
    for labels in (torch.randint(0, 2, shape, generator=gen),
                   torch.rand(shape, generator=gen)):
        want = F.binary_cross_entropy_with_logits(scores.reshape(labels.shape).float(),
                                                  labels.float())
        for s in (scores, scores.squeeze(1)):
            got = G.unsupervised_loss(s, labels)
            assert got.dim() == 0 and torch.equal(got, want)
    z = scores.detach().clone().requires_grad_()
    (3 * G.unsupervised_loss(z, labels)).backward()
    z2 = scores.detach().clone().requires_grad_()
    (3 * F.binary_cross_entropy_with_logits(z2.reshape(shape), labels)).backward()
    assert torch.equal(z.grad, z2.grad)
    empty = G.unsupervised_loss(torch.zeros(0, 1, 5), torch.zeros(0, 5))
    assert empty.dim() == 0 and torch.isnan(empty)
