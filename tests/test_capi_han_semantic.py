"""The semantic attention's entries of the C-ABI (csrc/han_semantic.hip: the scores, softmax and
weighted sum of HAN/models/SemanticAttention.py:15-20 and their adjoint): exported, declared to
ctypes, and rejecting bad arguments before anything reaches a device; the ops refuse CPU tensors
and ``han.SemanticAttention`` on CPU tensors is the torch expression bit for bit, gradients
included (no GPU needed)."""
import pytest
import torch

from graphneuralnetwork_amd import han

NEW = ("gnn_han_semantic_supported", "gnn_han_semantic_workspace_bytes",
       "gnn_han_semantic_fwd_f32", "gnn_han_semantic_bwd_f32", "gnn_han_tanh_f32")
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


def test_supported_table(lib):
    from graphneuralnetwork_amd import ops
    sup = lib.gnn_han_semantic_supported
    got = {(D, S, M) for D in range(-8, 300) for S in (0, 64, 127, 128, 129, 256)
           for M in range(-2, 12) if sup(D, S, M)}
    assert got == {(D, 128, M) for D in (16, 32, 64, 128) for M in range(1, 9)}
    assert not sup(1 << 40, 128, 3) and not sup(64, 128, 1 << 40)
    assert ops.han_semantic_supported(64, 128, 3) and not ops.han_semantic_supported(48, 128, 3)


def test_workspace_bytes(lib):
    ws = lib.gnn_han_semantic_workspace_bytes
    for D in (16, 32, 64, 128):
        for M in (1, 3, 8):
            sizes = [ws(n, M, D, 128) for n in (0, 1, 21, 22, 300, 5000, 100_000, 1 << 20,
                                                1 << 30, 1 << 40)]
            assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes)
            assert sizes[-1] == sizes[-2] == sizes[-3], "capped: no growth with N past the grid"
            assert sizes[-1] > sizes[0]
            assert sizes[-1] <= 32 << 20
    assert ws(-1, 3, 64, 128) == E_ARG and ws(5, -1, 64, 128) == E_ARG
    assert ws(5, 3, 48, 128) == E_UNSUPPORTED and ws(5, 9, 64, 128) == E_UNSUPPORTED
    assert ws(1 << 62, 8, 64, 128) == E_UNSUPPORTED


def _fw(lib, z=P, ld_n=192, ld_m=64, N=9, M=3, D=64, S=128, w1=P, b1=P, w2=P, w=P, beta=P, out=P,
        ldo=64, ws=P, ws_bytes=BIG):
    return lib.gnn_han_semantic_fwd_f32(z, ld_n, ld_m, N, M, D, S, w1, b1, w2, w, beta, out, ldo,
                                        ws, ws_bytes, None)


def _bw(lib, g=P, ldg=64, z=P, ld_n=192, ld_m=64, N=9, M=3, D=64, S=128, w1=P, b1=P, w2=P,
        beta=P, dz=P, lddz_n=192, lddz_m=64, dw1=P, db1=P, dw2=P, ws=P, ws_bytes=BIG):
    return lib.gnn_han_semantic_bwd_f32(g, ldg, z, ld_n, ld_m, N, M, D, S, w1, b1, w2, beta, dz,
                                        lddz_n, lddz_m, dw1, db1, dw2, ws, ws_bytes, None)


def test_forward_argument_rejection(lib):
    f = lambda **kw: _fw(lib, **kw)  # noqa: E731
    ws = lib.gnn_han_semantic_workspace_bytes
    for name in ("z", "w1", "b1", "w2", "beta", "out", "ws"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("N", "M", "D", "S"):
        assert f(**{name: -1}) == E_ARG, name
    assert f(ld_m=60) == E_ARG and f(ld_n=188) == E_ARG and f(ldo=60) == E_ARG  # pitches
    assert f(ld_m=68, ld_n=192) == E_ARG            # rows of one node overlap the next node's
    for D, S, M in ((48, 128, 3), (256, 128, 3), (64, 64, 3), (64, 128, 0), (64, 128, 9),
                    (0, 128, 3)):
        assert f(D=D, S=S, M=M, ld_m=256, ld_n=4096, ldo=256) == E_UNSUPPORTED, (D, S, M)
    for name in ("z", "w1", "out"):
        assert f(**{name: P + 8}) == E_ALIGN, name  # 16-B rows
    for name in ("b1", "w2", "w", "beta"):
        assert f(**{name: P + 2}) == E_ALIGN, name
    assert f(ws=P + 4) == E_ALIGN
    assert f(ld_m=66, ld_n=198) == E_ALIGN and f(ld_n=194) == E_ALIGN and f(ldo=66) == E_ALIGN
    assert f(ws_bytes=ws(9, 3, 64, 128) - 1) == E_ARG and f(ws_bytes=0) == E_ARG
    assert f(N=0) == OK
    assert f(N=0, z=None, w1=None, b1=None, w2=None, w=None, beta=None, out=None, ws=None,
             ws_bytes=0) == OK


def test_backward_argument_rejection(lib):
    f = lambda **kw: _bw(lib, **kw)  # noqa: E731
    ws = lib.gnn_han_semantic_workspace_bytes
    for name in ("g", "z", "w1", "b1", "w2", "beta", "ws"):
        assert f(**{name: None}) == E_ARG, name
    for name in ("N", "M", "D", "S"):
        assert f(**{name: -1}) == E_ARG, name
    assert f(ld_m=60) == E_ARG and f(ld_n=188) == E_ARG and f(ldg=60) == E_ARG
    assert f(lddz_m=60) == E_ARG and f(lddz_n=188) == E_ARG
    for D, S, M in ((48, 128, 3), (256, 128, 3), (64, 64, 3), (64, 128, 0), (64, 128, 9)):
        assert f(D=D, S=S, M=M, ld_m=256, ld_n=4096, ldg=256, lddz_m=256,
                 lddz_n=4096) == E_UNSUPPORTED, (D, S, M)
    for name in ("g", "z", "w1", "dz"):
        assert f(**{name: P + 8}) == E_ALIGN, name
    for name in ("b1", "w2", "beta", "dw1", "db1", "dw2"):
        assert f(**{name: P + 2}) == E_ALIGN, name
    assert f(ws=P + 4) == E_ALIGN and f(ldg=66) == E_ALIGN and f(lddz_n=194) == E_ALIGN
    assert f(ws_bytes=ws(9, 3, 64, 128) - 1) == E_ARG
    assert f(N=0) == OK
    assert f(N=0, g=None, z=None, w1=None, b1=None, w2=None, beta=None, dz=None, dw1=None,
             db1=None, dw2=None, ws=None, ws_bytes=0) == OK
    # nothing asked for: nothing launched (the pointers are never dereferenced)
    assert f(dz=None, dw1=None, db1=None, dw2=None) == OK
    t = lambda **kw: lib.gnn_han_tanh_f32(kw.get("x", P), kw.get("y", P), kw.get("n", 4), None)  # noqa: E731
    assert t(x=None) == E_ARG and t(y=None) == E_ARG and t(n=-1) == E_ARG
    assert t(x=P + 2) == E_ALIGN and t(n=0) == OK


def test_ops_refuse_cpu_tensors():
    from graphneuralnetwork_amd import ops
    z, w1, b1, w2 = torch.zeros(4, 3, 32), torch.zeros(128, 32), torch.zeros(128), torch.zeros(1, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.han_semantic_forward(z, w1, b1, w2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.han_semantic_backward(torch.zeros(4, 32), z, w1, b1, w2, torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.han_tanh(torch.zeros(4))


@pytest.mark.parametrize("shape", [(37, 3, 32), (5, 1, 64), (0, 2, 16), (9, 4, 24)])
def test_cpu_module_is_the_torch_expression(shape):
    """On CPU tensors nothing changes: the reference's two lines, bit for bit, and their
    gradients; state_dict keys as the reference's."""
    assert han.SEMANTIC_FUSED
    N, M, D = shape
    att = han.SemanticAttention(D)
    assert sorted(att.state_dict()) == ["project.0.bias", "project.0.weight", "project.2.weight"]
    z = torch.randn(N, M, D)
    a = z.clone().requires_grad_()
    b = z.clone().requires_grad_()
    got = att(a)
    beta = torch.softmax(att.project(b).mean(0), dim=0)
    want = (beta.unsqueeze(0) * b).sum(1)
    assert torch.equal(got, want) or (N == 0 and got.shape == want.shape)
    gy = torch.randn(N, D)
    ga = torch.autograd.grad((got * gy).sum(), [a, *att.parameters()], allow_unused=True)
    gb = torch.autograd.grad((want * gy).sum(), [b, *att.parameters()], allow_unused=True)
    for x, y in zip(ga, gb):
        assert (x is None and y is None) or torch.equal(x, y) or (N == 0 and x.shape == y.shape)
