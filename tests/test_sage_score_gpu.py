"""The unsupervised GraphSAGE head on the device (csrc/sage_score.hip, ops.sage_score /
sage_score_backward / bce_logits, graphsage._SageScoreFn / unsupervised_loss): the scores of
GraphSAGE/GraphSAGE.py:61, their adjoint and the loss of GraphSAGE/train_eval.py:113-114.

Every comparison against a float64 restatement is under the project's fp32 rule
(test_unsup_sampler_gpu._close: rtol 1e-4, atol 2e-5 max|ref|); what is stated as exact is
compared with torch.equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4), (3, 7, 8), (64, 30, 16), (7, 3, 64), (5, 30, 128), (2, 65, 256)]
NAN, INF = float("nan"), float("inf")
# the spacing of fp32 subnormals: no fp32 result lies closer than half of it to a reference below
# 2^-126 (log1p(exp(-100)) = 3.7e-44 is 26.5 of them)
F32_QUANTUM = 2.0 ** -149


def _close(got, ref, what, extra_atol=0.0):  # test_unsup_sampler_gpu._close: the fp32 rule
    a, b = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=2e-5 * scale + extra_atol, err_msg=what)


def _operands(dev, B, S, H, pitched):
    """center [B, H] and second [B S, H]; pitched: column slices [:, 4:4 + H] of wider tensors."""
    if pitched:
        c = torch.randn(B, H + 8, device=dev)[:, 4:4 + H]
        x = torch.randn(B * S, H + 12, device=dev)[:, 4:4 + H]
        assert not c.is_contiguous() or B == 1
    else:
        c, x = torch.randn(B, H, device=dev), torch.randn(B * S, H, device=dev)
    return c, x


def _bmm64(c, x, S):
    c64, x64 = c.cpu().double(), x.cpu().double()
    return torch.bmm(c64.unsqueeze(1), x64.reshape(c.shape[0], S, -1).permute(0, 2, 1)).squeeze(1)


# ------------------------------------------------------------------ the score kernels
@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
@pytest.mark.parametrize("B,S,H", SHAPES)
def test_forward_parity(dev, B, S, H, pitched):
    from graphneuralnetwork_amd import ops
    c, x = _operands(dev, B, S, H, pitched)
    z = ops.sage_score(c, x, S)
    assert z is not None and z.shape == (B, S) and z.dtype == torch.float32
    _close(z, _bmm64(c, x, S), f"scores {B, S, H}")
    out = torch.full((B, S), NAN, device=dev)
    assert ops.sage_score(c, x, S, out=out) is out and torch.equal(out, z)


@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
@pytest.mark.parametrize("B,S,H", SHAPES)
def test_backward_parity(dev, B, S, H, pitched):
    from graphneuralnetwork_amd import ops
    c, x = _operands(dev, B, S, H, pitched)
    g = torch.randn(B, S, device=dev)
    c64 = c.cpu().double().requires_grad_()
    x64 = x.cpu().double().requires_grad_()
    z64 = torch.bmm(c64.unsqueeze(1), x64.reshape(B, S, H).permute(0, 2, 1)).squeeze(1)
    z64.backward(g.cpu().double())
    dc, dx = ops.sage_score_backward(g, c, x)
    assert dc.shape == (B, H) and dx.shape == (B * S, H) and dx.is_contiguous()
    _close(dc, c64.grad, f"d_center {B, S, H}")
    _close(dx, x64.grad, f"d_second {B, S, H}")
    exact = (g.unsqueeze(2) * c.unsqueeze(1)).reshape(B * S, H)  # one fp32 product per element
    assert torch.equal(dx, exact)
    # a half nobody asks for is not allocated
    dc1, none = ops.sage_score_backward(g, c, x, need_second=False)
    assert none is None and torch.equal(dc1, dc)
    none, dx1 = ops.sage_score_backward(g, c, x, need_center=False)
    assert none is None and torch.equal(dx1, dx)
    assert ops.sage_score_backward(g, c, x, False, False) == (None, None)


@pytest.mark.parametrize("needs", [(True, False), (False, True), (True, True)],
                         ids=["center", "second", "both"])
def test_score_function_needs_input_grad(dev, needs):
    from graphneuralnetwork_amd.graphsage import _SageScoreFn
    B, S, H = 5, 30, 128
    c = torch.randn(B, H, device=dev, requires_grad=needs[0])
    x = torch.randn(B, S, H, device=dev, requires_grad=needs[1])
    g = torch.randn(B, 1, S, device=dev)
    z = _SageScoreFn.apply(c, x)
    assert z.shape == (B, 1, S)
    z.backward(g)
    c64 = c.detach().cpu().double().requires_grad_()
    x64 = x.detach().cpu().double().requires_grad_()
    torch.bmm(c64.unsqueeze(1), x64.permute(0, 2, 1)).backward(g.cpu().double())
    assert (c.grad is not None) == needs[0] and (x.grad is not None) == needs[1]
    if needs[0]:
        _close(c.grad, c64.grad, "d_center")
    if needs[1]:
        _close(x.grad, x64.grad, "d_second")
        assert x.grad.is_contiguous() and torch.equal(x.grad, g.reshape(B, S, 1) * c.detach()
                                                      .unsqueeze(1))


def test_determinism(dev):
    from graphneuralnetwork_amd import ops
    B, S, H = 64, 30, 128
    c, x = _operands(dev, B, S, H, False)
    g = torch.randn(B, S, device=dev)
    y = torch.randint(0, 2, (B, S), device=dev)
    first = (ops.sage_score(c, x, S), *ops.sage_score_backward(g, c, x), *ops.bce_logits(g, y))
    again = (ops.sage_score(c, x, S), *ops.sage_score_backward(g, c, x), *ops.bce_logits(g, y))
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_nan_rows_reach_the_scores_bmm_gives_them(dev):
    from graphneuralnetwork_amd import ops
    B, S, H = 7, 30, 128
    c, x = _operands(dev, B, S, H, False)
    x[::5] = 0.0  # NaN times zero is NaN as well
    c[2, 17] = NAN
    x[4 * S + 9, 100] = NAN
    z = ops.sage_score(c, x, S)
    ref = torch.bmm(c.unsqueeze(1), x.reshape(B, S, H).permute(0, 2, 1)).squeeze(1)
    want = torch.isnan(ref)
    assert int(want.sum()) == S + 1
    assert torch.equal(torch.isnan(z), want)
    _close(z[~want], ref[~want].double(), "the finite scores")


def test_offsets_past_32_bits(dev):
    """x is 8,200 x 1,024 rows of 128 floats = 4.3 GB: the last rows lie past 2^32 bytes."""
    from graphneuralnetwork_amd import ops
    B, S, H = 8200, 1024, 128
    assert B * S * H * 4 > 2 ** 32
    c = torch.randn(B, H, device=dev)
    x = torch.randn(B * S, H, device=dev)
    g = torch.randn(B, S, device=dev)
    z = ops.sage_score(c, x, S)
    for rows in (slice(0, 8), slice(B - 8, B)):
        xs = x[rows.start * S:rows.stop * S]
        _close(z[rows], _bmm64(c[rows], xs, S), f"scores of rows {rows.start}..")
    del z
    dc, dx = ops.sage_score_backward(g, c, x)
    t = slice(B - 8, B)
    assert torch.equal(dx[t.start * S:], (g[t].unsqueeze(2) * c[t].unsqueeze(1)).reshape(-1, H))
    ref = (g[t].cpu().double().unsqueeze(2) * x[t.start * S:].cpu().double().reshape(8, S, H)).sum(1)
    _close(dc[t], ref, "d_center of the last rows")
    assert torch.equal(dx[:S], g[0].unsqueeze(1) * c[0].unsqueeze(0))


def test_wrappers_check_and_decline(dev):
    from graphneuralnetwork_amd import ops
    c, x = torch.randn(4, 12, device=dev), torch.randn(20, 12, device=dev)
    g = torch.randn(4, 5, device=dev)
    assert ops.sage_score(c, x, 5) is None and ops.sage_score_backward(g, c, x) is None  # H = 12
    c, x = _operands(dev, 4, 5, 16, False)
    with pytest.raises(TypeError):
        ops.sage_score(c.double(), x, 5)
    with pytest.raises(ValueError):
        ops.sage_score(c, x, 4)
    with pytest.raises(ValueError):
        ops.sage_score_backward(g[:, :4], c, x)
    with pytest.raises(TypeError):
        ops.bce_logits(g.double(), g)
    with pytest.raises(TypeError):
        ops.bce_logits(g, g.to(torch.int32))
    with pytest.raises(ValueError):
        ops.bce_logits(g, g[:, :4])
    wide = torch.randn(20, 32, device=dev)
    assert ops.sage_score(c, wide[:, ::2], 5) is None          # stride 2 along H
    assert ops.sage_score(c, wide[:, 1:17], 5) is None         # rows 4 B off a 16-B boundary
    assert ops.sage_score(c, torch.randn(20, 18, device=dev)[:, :16], 5) is None  # pitch 18
    assert ops.bce_logits(wide[:, ::2], wide[:, ::2]) is None
    assert ops.bce_logits(g[:0], g[:0]) is None
    empty = ops.sage_score(c[:0], x[:0], 5)
    assert empty.shape == (0, 5)
    dc, dx = ops.sage_score_backward(torch.zeros(4, 0, device=dev), c, x[:0])
    assert dx.shape == (0, 16) and torch.equal(dc, torch.zeros_like(c))


# ------------------------------------------------------------------ the loss
def _labels(kind, shape, dev):
    if kind == "float":
        return torch.randint(0, 2, shape, device=dev).float()
    if kind == "int64":
        return torch.randint(0, 2, shape, device=dev)
    return torch.rand(shape, device=dev)


@pytest.mark.parametrize("kind", ["float", "int64", "soft"])
@pytest.mark.parametrize("B,S", [(1, 1), (5, 30), (8192, 30)], ids=["n1", "n150", "n245760"])
def test_bce_parity(dev, B, S, kind):
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.graphsage import unsupervised_loss
    z = 3 * torch.randn(B, S, device=dev)
    y = _labels(kind, (B, S), dev)
    z64 = z.cpu().double().requires_grad_()
    ref = F.binary_cross_entropy_with_logits(z64, y.cpu().double())
    (3 * ref).backward()
    loss, g = ops.bce_logits(z, y)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and g.shape == (B, S)
    _close(loss, ref, f"loss {kind} n={B * S}")
    _close(3 * g, z64.grad, f"g {kind} n={B * S}")
    only, none = ops.bce_logits(z, y, want_grad=False)
    assert none is None and torch.equal(only, loss)
    got = {}
    for name, zz in (("[B,S]", z), ("[B,1,S]", z.reshape(B, 1, S))):
        zz = zz.clone().requires_grad_()
        l = unsupervised_loss(zz, y)
        assert l.dim() == 0
        (3 * l).backward()
        assert zz.grad.shape == zz.shape
        _close(l, ref, f"unsupervised_loss {name}")
        _close(zz.grad.reshape(B, S), z64.grad, f"unsupervised_loss grad {name}")
        got[name] = (l.detach(), zz.grad.reshape(B, S))
    assert torch.equal(got["[B,S]"][0], got["[B,1,S]"][0]) and torch.equal(got["[B,S]"][0], loss)
    assert torch.equal(got["[B,S]"][1], got["[B,1,S]"][1])


def _cls(t):
    v = float(t.detach())
    return "nan" if v != v else "+inf" if v == INF else "-inf" if v == -INF else "finite"


@pytest.mark.parametrize("y", [0.0, 1.0])
@pytest.mark.parametrize("z", [INF, -INF, NAN, 100.0, -100.0, 88.8, -88.8])
def test_bce_nonfinite(dev, z, y):
    """The class (NaN / inf / finite) of the loss and of g is torch's on the same device; what is
    finite agrees with torch in float64 under the rule, plus one fp32 subnormal spacing (the loss
    at (100, 1) is log1p(exp(-100)) = 3.7e-44)."""
    from graphneuralnetwork_amd import ops
    zt = torch.tensor([[z]], device=dev)
    yt = torch.tensor([[y]], device=dev)
    loss, g = ops.bce_logits(zt, yt)
    zd = zt.clone().requires_grad_()
    F.binary_cross_entropy_with_logits(zd, yt).backward()
    tl = F.binary_cross_entropy_with_logits(zt, yt)
    z64 = zt.cpu().double().requires_grad_()
    l64 = F.binary_cross_entropy_with_logits(z64, yt.cpu().double())
    l64.backward()
    print(f"z {z} y {y}: loss {float(loss)!r} torch {float(tl)!r} float64 {float(l64.detach())!r}; "
          f"g {float(g)!r} torch {float(zd.grad)!r} float64 {float(z64.grad)!r}")
    assert _cls(loss) == _cls(tl) == _cls(l64)
    assert _cls(g) == _cls(zd.grad) == _cls(z64.grad)
    if _cls(loss) == "finite":
        _close(loss, l64, "loss", extra_atol=F32_QUANTUM)
    if _cls(g) == "finite":
        _close(g, z64.grad, "g", extra_atol=F32_QUANTUM)
    li, gi = ops.bce_logits(zt, yt.long())
    assert torch.equal(li, loss) or _cls(loss) == "nan"
    assert torch.equal(gi, g) or _cls(g) == "nan"


# ------------------------------------------------------------------ the model
def _ring_graph(dev, n, chords, seed=0):  # test_unsup_sampler_gpu._ring_graph
    from graphneuralnetwork_amd.sampler import symmetric_adjacency
    rs = np.random.default_rng(seed)
    ring = np.arange(n)
    src = np.concatenate([ring, rs.integers(0, n, chords)])
    dst = np.concatenate([(ring + 1) % n, rs.integers(0, n, chords)])
    return symmetric_adjacency(src, dst, n, device=dev)


def _tower64(T, b, W, gcn):  # test_unsup_sampler_gpu._tower64
    h = None
    src = T
    steps = [(b.frontier, b.frontier_nbrs), (b.center_maps[0], b.neigh_maps[0])]
    for (cm, nm), w in zip(steps, W):
        cm, nm = cm.cpu(), nm.cpu()
        agg = src[nm].mean(dim=1)
        x = agg if gcn else torch.cat([src[cm], agg], dim=1)
        h = torch.relu(x @ w.t())
        src = h
    return h


KINK = 1e-4  # test_sage_maxpool_train_gpu.KINK: a pre-activation of at least KINK max|pre|


def _pre64(T, b, W, gcn):
    """The float64 pre-activations of one tower's two layers (the products of ``_tower64``)."""
    out, src = [], T
    steps = [(b.frontier, b.frontier_nbrs), (b.center_maps[0], b.neigh_maps[0])]
    for (cm, nm), w in zip(steps, W):
        cm, nm = cm.cpu(), nm.cpu()
        agg = src[nm].mean(dim=1)
        out.append((agg if gcn else torch.cat([src[cm], agg], dim=1)) @ w.t())
        src = torch.relu(out[-1])
    return out


def _kinks(T, ub, W, gcn, layer):
    """The output units of ``layer`` with a float64 pre-activation nearer to zero than
    KINK max|pre| in either tower."""
    pre = torch.cat([_pre64(T, t, W, gcn)[layer] for t in (ub.center, ub.context)]).abs()
    return (pre.min(dim=0).values < KINK * float(pre.max())).nonzero().flatten()


def _settled_weights(net, T, ub, gcn):
    """The model's weights with the rows of the units above redrawn (nn.Linear's own uniform
    init, fp32 values) until the float64 forward is away from every ReLU kink: at a kink the
    gradient is a matter of which side fp32's rounding falls on (with H = 128 some of the 250,000
    pre-activations of a random draw lie within 1e-8 of zero), not of the code under test. The
    clearance is asserted here, on the CPU, from the float64 restatement alone. Float64 copies
    that require grad; the net holds the same values."""
    gen = torch.Generator().manual_seed(11)
    W = [b.weight.weight.detach().cpu().double() for b in net.sage_blocks]
    for layer in range(2):  # layer 1 reads layer 0's output: settle in order
        for _ in range(400):
            bad = _kinks(T, ub, W, gcn, layer)
            if not len(bad):
                break
            fan = W[layer].shape[1]
            W[layer][bad] = ((torch.rand(len(bad), fan, generator=gen) * 2 - 1)
                             * fan ** -0.5).double()
    assert all(len(_kinks(T, ub, W, gcn, layer)) == 0 for layer in range(2)), \
        "the fixture does not clear its kinks"
    with torch.no_grad():
        for b, w in zip(net.sage_blocks, W):
            b.weight.weight.copy_(w.float())
    return [w.requires_grad_() for w in W]


def _ref64(T, ub, W, gcn):  # test_unsup_sampler_gpu._ref64
    hc = _tower64(T, ub.center, W, gcn)
    hx = _tower64(T, ub.context, W, gcn)
    B, S = ub.labels.shape
    scores = torch.bmm(hc.unsqueeze(1), hx.reshape(B, S, -1).permute(0, 2, 1))
    loss = F.binary_cross_entropy_with_logits(scores.squeeze(1), ub.labels.cpu().double())
    return hc, scores, loss


@pytest.fixture(scope="module")
def batch_graph(dev):  # the graph and sizes of test_unsup_sampler_gpu.test_unsupervised_batch
    adj = _ring_graph(dev, 2000, 6000, seed=3)
    seeds = torch.from_numpy(np.random.default_rng(1).choice(2000, 64, replace=False)).to(dev)
    table = torch.randn(2000, 32, generator=torch.Generator().manual_seed(77)).to(dev)
    return adj, seeds, table


class _NoBmm:
    """torch.bmm replaced by a function that raises (or counts), restored on exit."""

    def __init__(self, monkeypatch, forbid):
        self.calls = 0
        real = torch.bmm

        def bmm(*a, **kw):
            self.calls += 1
            if forbid:
                raise AssertionError("torch.bmm reached with the fused head on")
            return real(*a, **kw)

        monkeypatch.setattr(torch, "bmm", bmm)


def _step(net, args, labels):
    """One reference-shaped training step; (embeddings, scores, loss, weight gradients)."""
    from graphneuralnetwork_amd.graphsage import unsupervised_loss
    net.zero_grad(set_to_none=True)
    e, s = net(*args)
    l = unsupervised_loss(s, labels)
    l.backward()
    return (e.detach(), s.detach(), l.detach(),
            [b.weight.weight.grad.clone() for b in net.sage_blocks])


@pytest.mark.parametrize("H", [16, 128])
@pytest.mark.parametrize("gcn,dtype", [(False, torch.float32), (False, torch.bfloat16),
                                       (True, torch.float32)],
                         ids=["mean-fp32", "mean-bf16", "gcn-fp32"])
def test_model_training_step(dev, batch_graph, monkeypatch, gcn, dtype, H):
    from graphneuralnetwork_amd import graphsage as G
    from graphneuralnetwork_amd import sampler as S
    adj, seeds, table32 = batch_graph
    ub = S.sample_unsupervised_batch(adj, seeds, (5, 3), 5, 5, seed=21, gcn=gcn)
    table = table32.to(dtype)
    T64 = table.cpu().double()  # for bf16 the float64 side reads the rounded values
    torch.manual_seed(5)
    net = G.GraphSAGE(2, 32, H, gcn, agg_func="MEAN", Unsupervised=True).to(dev).train()
    W = _settled_weights(net, T64, ub, gcn)
    hc, scores, loss = _ref64(T64, ub, W, gcn)
    loss.backward()
    args = ub.forward_args(table)
    assert G.SAGE_SCORE_FUSED
    with monkeypatch.context() as m:
        _NoBmm(m, forbid=True)
        on = _step(net, args, ub.labels)
    with monkeypatch.context() as m:
        m.setattr(G, "SAGE_SCORE_FUSED", False)
        spy = _NoBmm(m, forbid=False)
        off = _step(net, args, ub.labels)
        assert spy.calls >= 1
    tag = f"gcn={gcn} {dtype} H={H}"
    for name, got in (("on", on), ("off", off)):
        _close(got[0], hc, f"{tag} {name} embeddings vs float64")
        _close(got[1], scores, f"{tag} {name} scores vs float64")
        _close(got[2], loss, f"{tag} {name} loss vs float64")
        for i, gw in enumerate(got[3]):
            _close(gw, W[i].grad, f"{tag} {name} grad W{i} vs float64")
    _close(on[1], off[1], f"{tag} scores on vs off")
    _close(on[2], off[2], f"{tag} loss on vs off")
    for i, (a, b) in enumerate(zip(on[3], off[3])):
        _close(a, b, f"{tag} grad W{i} on vs off")


def test_model_falls_back_at_unsupported_width(dev, batch_graph, monkeypatch):
    """H = 12: the score kernel declines, the forward and the training step run torch.bmm and
    still match float64."""
    from graphneuralnetwork_amd import graphsage as G
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd import sampler as S
    adj, seeds, table = batch_graph
    assert ops.sage_score(torch.zeros(2, 12, device=dev), torch.zeros(6, 12, device=dev), 3) is None
    ub = S.sample_unsupervised_batch(adj, seeds, (5, 3), 5, 5, seed=21)
    torch.manual_seed(5)
    net = G.GraphSAGE(2, 32, 12, False, agg_func="MEAN", Unsupervised=True).to(dev).train()
    W = _settled_weights(net, table.cpu().double(), ub, False)
    hc, scores, loss = _ref64(table.cpu().double(), ub, W, False)
    loss.backward()
    spy = _NoBmm(monkeypatch, forbid=False)
    e, s, l, grads = _step(net, ub.forward_args(table), ub.labels)
    assert spy.calls >= 1
    with torch.no_grad():
        e2, s2 = net.eval()(*ub.forward_args(table))
    assert spy.calls >= 2
    _close(e, hc, "embeddings")
    _close(s, scores, "scores")
    _close(s2, scores, "eval scores")
    _close(l, loss, "loss")
    for i, gw in enumerate(grads):
        _close(gw, W[i].grad, f"grad W{i}")


def _golden_close(a, b, rtol=1e-4):  # test_sage_gpu.close
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale)


@pytest.mark.parametrize("fused", [True, False], ids=["on", "off"])
def test_model_golden(golden, dev, monkeypatch, fused):
    """The reference's own unsupervised forward (tests/golden/sage.npz, B = 6, S = 5, H = 16);
    with the switch on torch.bmm is not reached."""
    from graphneuralnetwork_amd import graphsage as G
    g = golden("sage")
    sd = {k[len("unsup_sd_"):]: torch.from_numpy(v) for k, v in g.items()
          if k.startswith("unsup_sd_")}
    net = G.GraphSAGE(2, g["feat"].shape[1], 16, False, agg_func="MEAN", Unsupervised=True)
    net.load_state_dict(sd, strict=True)
    net.to(dev).eval()
    X = [torch.from_numpy(g[f"unsup_X{i}"]).to(dev) for i in range(8)]
    monkeypatch.setattr(G, "SAGE_SCORE_FUSED", fused)
    spy = _NoBmm(monkeypatch, forbid=fused)
    with torch.no_grad():
        emb, scores = net(*X, tuple(int(v) for v in g["unsup_shape"]))
    assert scores.shape == g["unsup_scores"].shape and spy.calls == (0 if fused else 1)
    _golden_close(emb.cpu().numpy(), g["unsup_emb"])
    _golden_close(scores.cpu().numpy(), g["unsup_scores"])


def test_pending_batch_stays_pending(dev, monkeypatch):
    """sync=False: no host read between the context draw and the end of the inference forward
    through the fused head (torch's sync debug mode raises on one); embeddings and scores equal
    the synced batch's bit for bit. The graph of test_unsup_sampler_gpu's pending test."""
    from graphneuralnetwork_amd import graphsage as G
    from graphneuralnetwork_amd import sampler as S
    adj = _ring_graph(dev, 2000, 6000, seed=3)
    seeds = torch.arange(100, 164, device=dev)
    table = torch.randn(2000, 64, device=dev)
    net = G.GraphSAGE(2, 64, 128, False, agg_func="MEAN", Unsupervised=True).to(dev).eval()
    a = S.sample_unsupervised_batch(adj, seeds, (5, 3), seed=4)
    _NoBmm(monkeypatch, forbid=True)
    with torch.no_grad():
        e1, s1 = net(*a.forward_args(table))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            p = S.sample_unsupervised_batch(adj, seeds, (5, 3), seed=4, sync=False)
            e2, s2 = net(*p.forward_args(table))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert p.pending and p.center.pending and p.context.pending
    assert s1.shape == (64, 1, 30)
    assert torch.equal(e1, e2) and torch.equal(s1, s2)
