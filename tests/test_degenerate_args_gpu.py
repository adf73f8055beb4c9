"""Arguments the reference accepts and the drop-ins used to crash on or mishandle: dropout
p = 1.0 in training, a fused ReLU + dropout layer on a shape the transform declines, and
gemm_tn operands whose rows overlap (expanded rows, as_strided windows). Float64 references.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def close(a, b, rtol=RTOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale)


def _sym_graph(n, e, seed, dev):
    """The GCN adjacency D^-1/2 (A_sym + I) D^-1/2 of e random edges (device CSR), and its
    float64 dense form."""
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, e), rng.integers(0, n, e)
    g = gcn_adjacency(torch.from_numpy(s), torch.from_numpy(d), n, device=dev)
    rowptr = g.rowptr.cpu()
    rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    A = torch.zeros(n, n, dtype=torch.float64)
    A[rows, g.col.cpu().long()] = g.val.cpu().double()
    return g, A


# ------------------------------------------------------------------ 1: dropout p = 1.0
def test_gcn_model_dropout_one_trains(dev, monkeypatch):
    """GCN_Model(128, 128, 7, 2, 1.0).train(): nn.Dropout(1.0) zeroes the hidden layer, so the
    output is b2 in every row, dW1 = db1 = dW2 = 0 exactly and db2 = the column sums of the
    upstream gradient (to the rounding of an fp32 sum in another order). The fused epilogue
    takes p < 1 only: _fuse_train leaves that Dropout to torch (span 2). It used to raise
    ValueError from gcn_transform."""
    from graphneuralnetwork_amd import gcn as gcn_mod
    from graphneuralnetwork_amd.gcn import GCN_Model
    n = 400
    g, _ = _sym_graph(n, 2000, 1, dev)
    net = GCN_Model(128, 128, 7, 2, 1.0).to(dev).train()
    with torch.no_grad():
        for m in (net.gcn_blocks.gcn0, net.gcn_blocks.gcn1):
            m.bias.normal_()
    spans = []
    real = gcn_mod._fuse_train
    monkeypatch.setattr(gcn_mod, "_fuse_train", lambda *a: spans.append(real(*a)) or spans[-1])
    X = torch.randn(n, 128, device=dev)
    gy = torch.randn(n, 7, device=dev)
    out = net(X, g)
    out.backward(gy)
    assert spans == [2, 0]
    b2 = net.gcn_blocks.gcn1.bias
    assert torch.equal(out, b2.detach().expand(n, 7))
    for t in (net.gcn_blocks.gcn0.dense.weight, net.gcn_blocks.gcn0.bias,
              net.gcn_blocks.gcn1.dense.weight):
        assert t.grad is not None and bool((t.grad == 0).all())
    close(b2.grad.cpu().numpy(), gy.double().sum(0).cpu().numpy())


def _gat_model_ref(model, x, mask, slope, sparse):
    """Float64 restatement of GAT / SpGAT (GAT/models/GAT.py:14-18, layers.py:22-37 and
    :94-131) in training with dropout 1.0: F.dropout(t, 1.0) is t * 0."""
    drop = lambda t: t * 0.0
    f64 = lambda t: t.detach().cpu().double()

    def layer(h, m, elu):
        W, a = f64(m.W), f64(m.a).reshape(-1)
        fh = W.shape[1]
        Wh = h @ W
        e = torch.nn.functional.leaky_relu((Wh @ a[:fh])[:, None] + (Wh @ a[fh:])[None, :], slope)
        if sparse:
            ee = torch.exp(-e) * mask
            hp = (drop(ee) @ Wh) / ee.sum(1, keepdim=True)
        else:
            att = torch.softmax(torch.where(mask, e, torch.full_like(e, -9e15)), dim=1)
            hp = drop(att) @ Wh
        return torch.nn.functional.elu(hp) if elu else hp

    h = drop(x.cpu().double())
    h = torch.cat([layer(h, m, True) for m in model.attentions], dim=1)
    return torch.nn.functional.elu(layer(drop(h), model.out_att, False))


@pytest.mark.parametrize("kind", ["GAT", "SpGAT"])
def test_gat_model_dropout_one_trains(dev, kind):
    """GAT / SpGAT(64, 8, 7, 1.0, 0.2, 8).train() on 400 nodes: the output is the float64
    restatement's with F.dropout(., 1.0) giving zeros, and the backward runs (zero
    gradients); one attention layer alone, over features that are not zero, gives zeros as
    well. The layers used to hand p = 1 to the kernels, which refuse it (GNN_E_ARG)."""
    from graphneuralnetwork_amd import gat as gat_mod
    n = 400
    rng = np.random.default_rng(2)
    adj = np.zeros((n, n), np.float32)
    adj[rng.integers(0, n, 3000), rng.integers(0, n, 3000)] = 1.0
    adj[np.arange(n), np.arange(n)] = 1.0  # no edgeless row (the sparse layer's 0 / 0)
    A = torch.from_numpy(adj).to(dev)
    x = torch.randn(n, 64, device=dev)
    model = getattr(gat_mod, kind)(64, 8, 7, 1.0, 0.2, 8).to(dev).train()
    out = model(x, A)
    ref = _gat_model_ref(model, x, torch.from_numpy(adj > 0), 0.2, kind == "SpGAT")
    assert out.shape == ref.shape and not bool(ref.any())
    assert torch.equal(out.cpu().double(), ref)
    out.backward(torch.randn_like(out))
    for p in model.parameters():
        assert p.grad is None or bool((p.grad == 0).all())
    layer = model.out_att.train()
    h = torch.randn(n, 64, device=dev, requires_grad=True)
    y = layer(h, A)
    assert y.shape == (n, 7) and bool((y == 0).all())
    y.backward(torch.randn_like(y))
    assert bool((h.grad == 0).all())
    with torch.no_grad():  # training mode without autograd: the same zeros
        assert bool((layer(h, A) == 0).all())


# ------------------------------------------- 2: the fused layer where the transform declines
def test_fused_relu_dropout_declines_with_the_transform(dev, monkeypatch):
    """ops.TRANSFORM_WIDE_MFMA = False: gcn_transform declines 128 -> 256, so
    fuses_relu_dropout must too. GCN_Model(128, 256, 7, 2, 0.5).train() then runs layer 1
    unfused (_fuse_train gives 0; the fused op used to save and return None), and its logits
    and gradients match the float64 statement of the chain under the mask its nn.Dropout drew
    (read off that module's output: an unfused Dropout draws from torch's generator, not from
    the hashed stream); gcn_layer(relu_dropout=) called on that shape raises ValueError."""
    from graphneuralnetwork_amd import gcn as gcn_mod
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.gcn import GCN_Model
    monkeypatch.setattr(ops, "TRANSFORM_WIDE_MFMA", False)
    n = 400
    g, A = _sym_graph(n, 2000, 3, dev)
    net = GCN_Model(128, 256, 7, 2, 0.5).to(dev).train()
    with torch.no_grad():
        for m in (net.gcn_blocks.gcn0, net.gcn_blocks.gcn1):
            m.bias.normal_()
    monkeypatch.setattr(gcn_mod, "dropout_seed", lambda: 1357)
    spans = []
    real = gcn_mod._fuse_train
    monkeypatch.setattr(gcn_mod, "_fuse_train", lambda *a: spans.append(real(*a)) or spans[-1])
    seen = {}
    net.gcn_blocks.dropout0.register_forward_hook(
        lambda mod, inp, out: seen.update(h=inp[0].detach(), d=out.detach()))
    X = torch.randn(n, 128, device=dev, requires_grad=True)
    gy = torch.randn(n, 7, device=dev)
    assert not ops.fuses_relu_dropout(X, net.gcn_blocks.gcn0.dense.weight, g)
    out = net(X, g)
    out.backward(gy)
    assert spans == [0, 0]
    keep = (seen["d"] != 0).cpu()
    pos = (seen["h"] > 0).cpu()
    assert not bool((keep & ~pos).any()) and abs(float(keep[pos].double().mean()) - 0.5) < 0.02
    params = [net.gcn_blocks.gcn0.dense.weight, net.gcn_blocks.gcn0.bias,
              net.gcn_blocks.gcn1.dense.weight, net.gcn_blocks.gcn1.bias]
    Xr, W1, b1, W2, b2 = (t.detach().cpu().double().requires_grad_() for t in [X] + params)
    y1 = A @ (Xr @ W1.t()) + b1
    # the ReLU mask is the model's own (H > 0), so no element near the kink can flip
    h = y1 * pos * keep * 2.0
    ref = A @ (h @ W2.t()) + b2
    ref.backward(gy.cpu().double())
    close(seen["h"].cpu().numpy(), (y1 * pos).detach().numpy())
    close(out.detach().cpu().numpy(), ref.detach().numpy())
    for got, want in zip([X] + params, (Xr, W1, b1, W2, b2)):
        close(got.grad.cpu().numpy(), want.grad.numpy())
    with pytest.raises(ValueError):
        ops.gcn_layer(g, X.detach(), net.gcn_blocks.gcn0.dense.weight, net.gcn_blocks.gcn0.bias,
                      relu_dropout=(0.5, 1357))


# ------------------------------------------------------------------ 3: gemm_tn row strides
def _tn_check(a, b, d, h):
    """gemm_tn (plain and transposed output, with the column sums of d) and gemm_tn_masked over
    the given operands against float64."""
    from graphneuralnetwork_amd.ops import gemm_tn, gemm_tn_masked
    ref = a.double().t() @ b.double()
    c, ds = gemm_tn(a, b, d)
    close(c.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)
    close(ds.cpu().numpy(), d.double().sum(0).cpu().numpy(), rtol=1e-5)
    ct, none = gemm_tn(a, b, trans=True)
    assert none is None and ct.shape == ref.t().shape
    close(ct.cpu().numpy(), ref.t().cpu().numpy(), rtol=1e-5)
    bm = torch.where(h > 0, b.double() * 2.0, torch.zeros((), dtype=torch.float64,
                                                          device=b.device))
    cm, dm = gemm_tn_masked(a, b, h, 2.0, True, trans=True)
    close(cm.cpu().numpy(), (bm.t() @ a.double()).cpu().numpy(), rtol=1e-5)
    close(dm.cpu().numpy(), bm.sum(0).cpu().numpy(), rtol=1e-5)


def test_transforms_take_expanded_rows(dev):
    """gcn_transform (the MFMA transform) and linear_small (the narrow kernels) over a row
    expanded to n rows (row stride 0, e.g. the gradient of a column sum) copy it out: the
    C entry points refuse a row stride below the row length (GNN_E_ARG), which the GAT
    projection's backward used to run into."""
    from graphneuralnetwork_amd.ops import gcn_transform, linear_small
    n = 37
    x = torch.randn(128, device=dev).expand(n, 128)
    for fout, fn in ((128, gcn_transform), (7, linear_small)):
        w = torch.randn(fout, 128, device=dev)
        y = fn(x, w)
        assert y is not None
        close(y.cpu().numpy(), (x.double() @ w.double().t()).cpu().numpy())


@pytest.mark.parametrize("m,k", [(128, 128), (64, 8), (33, 5)])
def test_gemm_tn_overlapping_rows(dev, m, k):
    """gemm_tn / gemm_tn_masked with operands whose row stride is below the row length -- a
    row expanded to n rows (stride 0) as a, as b and as d, and an as_strided window of
    overlapping rows (stride 1) -- in the wide (128, 128) and the narrow kinds: such operands
    are copied out and the kernel gets their real stride (the call used to pass
    max(stride, row length) over the uncopied view: n * m floats read from one row). A single
    row (n = 1) of any stride is passed as it is."""
    n = 37
    gen = torch.Generator(device=dev).manual_seed(m + k)
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen)
    a, b, d, h = rand(n, m), rand(n, k), rand(n, k), torch.relu(rand(n, k))
    _tn_check(rand(m).expand(n, m), b, d, h)
    eb = rand(k).expand(n, k)
    _tn_check(a, eb, eb, h)
    _tn_check(a, b, rand(k).expand(n, k), h)
    _tn_check(torch.as_strided(rand(n + m), (n, m), (1, 1)), b, d, h)
    _tn_check(a, torch.as_strided(rand(n + k), (n, k), (1, 1)), d, h)
    # n = 1: views with stride(0) < row length
    a1, b1 = rand(m, 1).t(), rand(k, 1).t()
    assert a1.shape == (1, m) and a1.stride(0) < m and b1.stride(0) < k
    h1 = torch.relu(rand(1, k))
    _tn_check(a1, b1, b1, h1)
    _tn_check(rand(m).expand(1, m), rand(k).expand(1, k), rand(1, k), h1)
