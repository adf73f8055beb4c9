"""HAN's semantic attention in the kernels of csrc/han_semantic.hip (ops.han_semantic_forward /
_backward, han._SemanticFn, han.SemanticAttention) against float64: the forward against
oracle.gnn_oracle.han_semantic_attention, the gradients against torch's float64 autograd of the
reference expression on the CPU.

Bounds. ``out`` and ``dz`` element-wise: the project's fp32 bound, rtol 1e-4 and
atol 2e-5 max|ref|. ``beta``: 1e-5 absolute. dW1, db1, dw2 (sums over the node axis): 1e-4 of
the largest entry of each. The kernels' tanh, 1 - 2 / (1 + exp(2x)) on the hardware exponential
and reciprocal: with u = 2^-24, exp(2x) carries at most (2 + 2|x|) u relative error (the
argument's rounding and v_exp_f32's 1 ulp), which reaches the result through 2e / (1 + e)^2
(at most 1 u over all x); the rounding of 1 + e (u) and the reciprocal's 1 ulp (2u) reach it
through 2 / (1 + e) <= 2 (6u), the final fma adds u: 8u = 4.8e-7 absolute.

Shapes: a tile is 64 rows of the [N M, D] view, the persistent grid 512 workgroups, so
30,011 x 3 rows = 1,407 tiles give every workgroup two or three tiles."""
import functools

import numpy as np
import pytest
import torch

from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
S = 128
TANH_BOUND = 8 * 2.0 ** -24


@pytest.fixture(autouse=True)
def fused_on(monkeypatch):
    from graphneuralnetwork_amd import han
    monkeypatch.setattr(han, "SEMANTIC_FUSED", True)
    monkeypatch.setattr(han, "SEMANTIC_MIN_ROWS", None)


def close(a, b, rtol=1e-4):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-5 * scale)


def close_sum(a, b):
    """Sums over the node axis: within 1e-4 of the largest entry."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (np.abs(a - b).max(), np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _case(N, M, D):
    """Inputs (CPU float32) of one shape, drawn from the shape alone; never modified."""
    gen = torch.Generator().manual_seed(1000003 * N + 1009 * M + D)
    z = torch.randn(N, M, D, generator=gen) + 0.4 * torch.arange(M).view(1, M, 1)
    w1 = torch.randn(S, D, generator=gen) / D ** 0.5
    b1 = 0.1 * torch.randn(S, generator=gen)
    w2 = torch.randn(1, S, generator=gen) / S ** 0.5
    gy = torch.randn(N, D, generator=gen)
    return z, w1, b1, w2, gy


@functools.lru_cache(maxsize=None)
def _forward_ref(N, M, D):
    z, w1, b1, w2, _ = (t.numpy() for t in _case(N, M, D))
    out = O.han_semantic_attention(z, w1, b1, w2)
    w = (np.tanh(z.astype(np.float64) @ w1.astype(np.float64).T + b1) @ w2.astype(np.float64).T
         ).mean(0)[:, 0]
    e = np.exp(w - w.max())
    return out, e / e.sum()


def _ref_expr(z, w1, b1, w2):
    beta = torch.softmax((torch.tanh(z @ w1.T + b1) @ w2.T).mean(0), dim=0)
    return (beta.unsqueeze(0) * z).sum(1)


@functools.lru_cache(maxsize=None)
def _backward_ref(N, M, D):
    z, w1, b1, w2, gy = (t.double().requires_grad_(i < 4) for i, t in enumerate(_case(N, M, D)))
    (_ref_expr(z, w1, b1, w2) * gy).sum().backward()
    return tuple(t.grad.numpy() for t in (z, w1, b1, w2))


FWD_SHAPES = [(N, M, D) for N in (1, 5, 301, 30011) for M in (1, 2, 3, 8)
              for D in (16, 32, 64, 128)]
# N M one short of, on and one past a tile of 64 rows; with M = 3 a tile holds rows of
# different metapaths and a node's rows straddle two tiles
EDGE_SHAPES = [(63, 1, 32), (64, 1, 32), (65, 1, 32), (21, 3, 64), (64, 3, 16), (43, 3, 128)]


@pytest.mark.parametrize("N,M,D", FWD_SHAPES + EDGE_SHAPES)
def test_forward_matches_oracle(N, M, D, dev):
    from graphneuralnetwork_amd import ops
    z, w1, b1, w2, _ = (t.to(dev) for t in _case(N, M, D))
    out, beta = ops.han_semantic_forward(z, w1, b1, w2)
    ref_out, ref_beta = _forward_ref(N, M, D)
    assert out.shape == (N, D) and beta.shape == (M,)
    err = np.abs(beta.cpu().numpy().astype(np.float64) - ref_beta).max()
    print(f"beta max abs err {err:.3e}")
    assert err <= 1e-5
    close(out.cpu().numpy(), ref_out)


@pytest.mark.parametrize("N,M,D", [(301, 3, 32), (5, 2, 128), (30011, 3, 64)])
def test_forward_pitched_view(N, M, D, dev):
    from graphneuralnetwork_amd import ops
    z, w1, b1, w2, _ = (t.to(dev) for t in _case(N, M, D))
    ld_m = D + 4
    ld_n = M * ld_m + 8
    buf = torch.full((N * ld_n + 16,), float("nan"), device=dev)
    zv = buf.as_strided((N, M, D), (ld_n, ld_m, 1))
    zv.copy_(z)
    assert ops._han_rows(zv, "z") is zv, "the pitched view must be read in place"
    out, beta = ops.han_semantic_forward(zv, w1, b1, w2)
    out0, beta0 = ops.han_semantic_forward(z, w1, b1, w2)
    assert torch.equal(out, out0) and torch.equal(beta, beta0)
    close(out.cpu().numpy(), _forward_ref(N, M, D)[0])
    # and the adjoint writes a pitched dz / reads a pitched z
    g = _case(N, M, D)[4].to(dev)
    dbuf = torch.full_like(buf, float("nan"))
    dzv = dbuf.as_strided((N, M, D), (ld_n, ld_m, 1))
    got = ops.han_semantic_backward(g, zv, w1, b1, w2, beta, dz_out=dzv)
    want = ops.han_semantic_backward(g, z, w1, b1, w2, beta0)
    assert got[0] is dzv
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    touched = torch.zeros_like(buf, dtype=torch.bool)
    touched.as_strided((N, M, D), (ld_n, ld_m, 1)).fill_(True)
    assert torch.isnan(dbuf[~touched]).all(), "a store outside the view"


def test_tanh_bound(dev):
    from graphneuralnetwork_amd import ops
    x = np.concatenate([
        np.linspace(-60, 60, 240001), np.linspace(-12, 12, 200001),
        np.linspace(-1e-3, 1e-3, 20001), np.logspace(-30, -3, 2000), -np.logspace(-30, -3, 2000),
        np.array([0.0, -0.0, 40.5, -40.5, 44.0, -44.0, 50.0, -50.0, 88.0, -88.0, 89.0, -89.0,
                  100.0, -100.0, 1e4, -1e4, 1e30, -1e30, 3e38, -3e38])]).astype(np.float32)
    assert (np.abs(x) < 1e-3).sum() > 1000 and (np.abs(x) > 40).sum() > 1000
    y = ops.han_tanh(torch.from_numpy(x).to(dev)).cpu().numpy()
    err = np.abs(y.astype(np.float64) - np.tanh(x.astype(np.float64)))
    worst = int(err.argmax())
    print(f"tanh max abs err {err.max():.3e} at x = {x[worst]!r}; "
          f"|x| < 1e-3: {err[np.abs(x) < 1e-3].max():.3e}; |x| > 40: {err[np.abs(x) > 40].max():.3e}")
    assert err.max() <= TANH_BOUND
    assert (y[np.abs(x) > 40] == np.sign(x[np.abs(x) > 40])).all()
    sp = ops.han_tanh(torch.tensor([float("inf"), float("-inf"), float("nan")], device=dev)).cpu()
    assert sp[0] == 1 and sp[1] == -1 and torch.isnan(sp[2])


def test_saturation_matches_oracle(dev):
    from graphneuralnetwork_amd import ops
    N, M, D = 301, 3, 64
    z, w1, b1, w2, _ = _case(N, M, D)
    pre = (z.double() @ w1.double().T + b1.double()).abs().max().item()
    w1 = (w1 * (50.0 / pre * 1.05)).contiguous()
    pre = (z.double() @ w1.double().T + b1.double()).abs()
    assert pre.max() >= 50 and (pre > 20).float().mean() > 0.05
    out, beta = ops.han_semantic_forward(z.to(dev), w1.to(dev), b1.to(dev), w2.to(dev))
    assert torch.isfinite(out).all() and torch.isfinite(beta).all()
    close(out.cpu().numpy(), O.han_semantic_attention(z.numpy(), w1.numpy(), b1.numpy(), w2.numpy()))
    g = torch.randn(N, D, device=dev)
    for t in ops.han_semantic_backward(g, z.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), beta):
        assert torch.isfinite(t).all()


def test_nan_in_z_poisons_both_paths(dev, monkeypatch):
    from graphneuralnetwork_amd import han
    N, M, D = 301, 3, 32
    z = _case(N, M, D)[0].clone()
    z[77, 1, 5] = float("nan")
    att = han.SemanticAttention(D).to(dev)
    calls = []
    real = han.han_semantic_forward
    monkeypatch.setattr(han, "han_semantic_forward", lambda *a: calls.append(1) or real(*a))
    with torch.no_grad():
        fused = att(z.to(dev))
        assert calls == [1]
        monkeypatch.setattr(han, "SEMANTIC_FUSED", False)
        plain = att(z.to(dev))
        assert calls == [1]
    assert torch.isnan(fused).all() and torch.isnan(plain).all()
    from graphneuralnetwork_amd import ops
    l1, _, l2 = att.project
    _, beta = ops.han_semantic_forward(z.to(dev), l1.weight.detach(), l1.bias.detach(),
                                       l2.weight.detach())
    assert torch.isnan(beta).all()


@pytest.mark.parametrize("N,D", [(1, 16), (301, 64), (30011, 32)])
def test_one_metapath_is_the_identity(N, D, dev):
    from graphneuralnetwork_amd import ops
    z, w1, b1, w2, gy = (t.to(dev) for t in _case(N, 1, D))
    out, beta = ops.han_semantic_forward(z, w1, b1, w2)
    assert beta.item() == 1.0 and torch.equal(out, z[:, 0, :])
    dz, dw1, db1, dw2 = ops.han_semantic_backward(gy, z, w1, b1, w2, beta)
    assert torch.equal(dz[:, 0, :], gy)
    for t in (dw1, db1, dw2):
        assert (t == 0).all()


GRAD_SHAPES = [(30011, 3, 32), (30011, 3, 64), (1, 2, 16), (5, 8, 128), (301, 3, 128),
               (301, 8, 16), (301, 2, 64), (21, 3, 32), (64, 3, 64), (43, 3, 16), (65, 1, 128)]


@pytest.mark.parametrize("N,M,D", GRAD_SHAPES)
def test_gradients_match_float64_autograd(N, M, D, dev):
    from graphneuralnetwork_amd import han
    z, w1, b1, w2, gy = (t.to(dev) for t in _case(N, M, D))
    leaves = [t.clone().requires_grad_() for t in (z, w1, b1, w2)]
    (han._SemanticFn.apply(*leaves) * gy).sum().backward()
    ref = _backward_ref(N, M, D)
    got = [t.grad.cpu().numpy() for t in leaves]
    assert got[3].shape == (1, S)
    for name, a, b in zip(("dW1", "db1", "dw2"), got[1:], ref[1:]):
        print(f"{name}: max abs diff {np.abs(a - b).max():.3e}, largest entry {np.abs(b).max():.3e}")
    close(got[0], ref[0])
    for a, b in zip(got[1:], ref[1:]):
        if M == 1:
            assert (a == 0).all()   # the reference's are rounding noise around zero
        else:
            close_sum(a, b)


@pytest.mark.parametrize("frozen", ["params", "z"])
def test_needs_input_grad_variants(frozen, dev):
    from graphneuralnetwork_amd import han
    N, M, D = 301, 3, 64
    z, w1, b1, w2, gy = (t.to(dev) for t in _case(N, M, D))
    att = han.SemanticAttention(D).to(dev)
    with torch.no_grad():
        att.project[0].weight.copy_(w1)
        att.project[0].bias.copy_(b1)
        att.project[2].weight.copy_(w2)
    ref = _backward_ref(N, M, D)
    zz = z.clone()
    if frozen == "params":
        att.requires_grad_(False)
        zz.requires_grad_()
    (att(zz) * gy).sum().backward()
    if frozen == "params":
        close(zz.grad.cpu().numpy(), ref[0])
        assert all(p.grad is None for p in att.parameters())
    else:
        assert zz.grad is None
        for p, b in zip(att.parameters(), ref[1:]):
            close_sum(p.grad.cpu().numpy(), b.reshape(p.shape))


@pytest.mark.parametrize("N,M,D", [(30011, 3, 64), (301, 8, 128), (5, 2, 16)])
def test_determinism(N, M, D, dev):
    from graphneuralnetwork_amd import ops
    z, w1, b1, w2, gy = (t.to(dev) for t in _case(N, M, D))
    runs = []
    for _ in range(2):
        out, beta = ops.han_semantic_forward(z, w1, b1, w2)
        runs.append((out, beta, *ops.han_semantic_backward(gy, z, w1, b1, w2, beta)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ drop-in (golden han.npz)
def _sd(d, prefix="sd_"):
    return {k[len(prefix):]: torch.from_numpy(np.asarray(d[k])) for k in d if k.startswith(prefix)}


def _han(golden, dev, dropout):
    from graphneuralnetwork_amd.han import HANModel
    d = golden("han")
    N, M, Fin, hid, C = (int(v) for v in d["dims"])
    net = HANModel(M, Fin, hid, C, [int(h) for h in d["heads"]], dropout=dropout)
    net.load_state_dict(_sd(d), strict=True)
    gs = []
    for m in range(M):
        A = torch.zeros(N, N)
        A[torch.from_numpy(d[f"g{m}_row"]).long(), torch.from_numpy(d[f"g{m}_col"]).long()] = 1
        gs.append(A.to(dev))
    return d, net.to(dev), gs, torch.from_numpy(d["h"]).to(dev)


def close1(a, b, rtol=1e-4):  # test_han_sagepy_gpu.close
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-5 * scale)


def _count_fused(monkeypatch):
    from graphneuralnetwork_amd import han
    calls = []
    real = han.han_semantic_forward
    monkeypatch.setattr(han, "han_semantic_forward", lambda *a: calls.append(1) or real(*a))
    return calls


def test_golden_han_matches_reference_fused(golden, dev, monkeypatch):
    calls = _count_fused(monkeypatch)
    d, net, gs, h = _han(golden, dev, 0.6)
    net.eval()
    with torch.no_grad():
        close1(net.layers[0](gs, h).cpu().numpy(), d["layer0"])
        close1(net(gs, h).cpu().numpy(), d["logits"])
    assert len(calls) == 1 + len(net.layers), "the semantic attention ran in torch"


def test_golden_han_training_agrees_with_torch_path(golden, dev, monkeypatch):
    from graphneuralnetwork_amd import han
    calls = _count_fused(monkeypatch)
    d, net, gs, h = _han(golden, dev, 0.0)
    net.train()
    y = torch.from_numpy(np.arange(h.shape[0]) % int(d["dims"][4])).to(dev)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(han, "SEMANTIC_FUSED", fused)
        net.zero_grad()
        out = net(gs, h)
        torch.nn.functional.cross_entropy(out, y).backward()
        res[fused] = (out.detach().cpu().numpy(),
                      {k: p.grad.cpu().numpy().copy() for k, p in net.named_parameters()})
    assert len(calls) == len(net.layers)
    close1(res[True][0], res[False][0])
    assert any("semantic_attention" in k for k in res[True][1])
    for k, gref in res[False][1].items():
        close1(res[True][1][k], gref)


def test_min_rows_threshold(dev, monkeypatch):
    """N M below han.SEMANTIC_MIN_ROWS keeps torch's lines; the default is a row count."""
    import importlib.util
    from graphneuralnetwork_amd import han
    src = importlib.util.find_spec(han.__name__).origin
    assert "\nSEMANTIC_MIN_ROWS = 300_000\n" in open(src).read(), "the measured default"
    calls = _count_fused(monkeypatch)
    N, M, D = 301, 3, 32
    z = _case(N, M, D)[0].to(dev)
    att = han.SemanticAttention(D).to(dev)
    with torch.no_grad():
        monkeypatch.setattr(han, "SEMANTIC_MIN_ROWS", N * M + 1)
        plain = att(z)
        assert calls == []
        monkeypatch.setattr(han, "SEMANTIC_MIN_ROWS", N * M)
        fused = att(z)
        assert calls == [1]
    close(fused.cpu().numpy(), plain.cpu().numpy())


def test_forward_hook_sends_the_call_down_the_torch_path(dev, monkeypatch):
    from graphneuralnetwork_amd import han
    calls = _count_fused(monkeypatch)
    N, M, D = 301, 3, 32
    z = _case(N, M, D)[0].to(dev)
    att = han.SemanticAttention(D).to(dev)
    fired = []
    with torch.no_grad():
        want = att(z)
        assert calls == [1]
        handle = att.project[1].register_forward_hook(lambda m, i, o: fired.append(tuple(o.shape)))
        got = att(z)
        assert calls == [1] and fired == [(N, M, S)]
        handle.remove()
        att(z)
        assert calls == [1, 1]
        pre = att.project.register_forward_pre_hook(lambda m, i: fired.append("pre"))
        att(z)
        assert calls == [1, 1] and fired[-1] == "pre"
        pre.remove()
    close(got.cpu().numpy(), want.cpu().numpy())
