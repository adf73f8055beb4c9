"""NaN / Inf propagation of the fused epilogues and gathers against torch's own behaviour.

Every reference is a float64 CPU restatement, in torch operations, of the reference module's
formula -- torch.relu, dropout as a multiplication by keep * scale (the oracle's hashed keep
mask), sums over the edges of a row -- so that torch decides what a NaN or an Inf does. Inputs
stay at randn scale: fp32 cannot overflow where float64 does not.

The gathers are poisoned where kernels clamp to: masked tail lanes gather row 0 with weight 0,
so row 0 and the last row are the poisoned ones (a 0 * NaN leak from a clamped lane shows as a
NaN in a row that has no edge to the poisoned one). Containment: every output row with no edge
to the poisoned row is bit-identical to the clean run's row.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-4  # the kernels' usual tolerance (tests/test_training_gpu.py close())
NAN, INF = float("nan"), float("inf")


def close(a, b, rtol=RTOL, scale=None):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if scale is None:
        scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale)


def same(got, ref, zero=None, rtol=RTOL):
    """The one comparison of this file: the isnan / isposinf / isneginf patterns of ``got``
    (fp32, device) and ``ref`` (float64) are equal, the finite entries are close at the
    kernel's usual tolerance (atol scaled by the largest finite |ref|), and the entries that
    are zero by construction (``zero``: a dropped element, ReLU of -Inf) are == 0 (either
    sign). A ReLU zero next to the kink is left to the tolerance: fp32 may round a 1e-9
    pre-activation to the other side of 0."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu()
    assert got.shape == ref.shape
    for name, f in (("nan", torch.isnan), ("+inf", torch.isposinf), ("-inf", torch.isneginf)):
        a, b = f(got), f(ref)
        assert torch.equal(a, b), f"{name} pattern differs at {(a != b).nonzero()[:8].tolist()}"
    fin = torch.isfinite(ref)
    scale = max(1.0, float(ref[fin].abs().max())) if fin.any() else 1.0
    close(got[fin].numpy(), ref[fin].numpy(), rtol, scale)
    if zero is not None:
        zero = zero & fin
        assert bool((ref[zero] == 0).all()) and bool((got[zero] == 0).all())


def bits_equal(a, b):
    """Bit for bit, NaNs included (the same code on the same finite inputs)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def cpu(*ts):
    return ts[0].cpu() if len(ts) == 1 else tuple(t.cpu() for t in ts)


@pytest.fixture(params=["split-bf16", "fp32-mfma"])
def precision(request, dev):
    from graphneuralnetwork_amd.ops import set_transform_precision
    prev = set_transform_precision(request.param)
    yield request.param
    set_transform_precision(prev)


def _xw(k, fout, n, dev):
    gen = torch.Generator().manual_seed(1000 * k + fout + n)
    x = torch.randn(n, k, generator=gen)
    w = torch.randn(fout, k, generator=gen) * 0.2
    return x, w


# ------------------------------------------------------------------ 1, 2: linear + ReLU
@pytest.mark.parametrize("n", [37, 333])
@pytest.mark.parametrize("k,fout", [(64, 64), (128, 128), (256, 256)])
def test_transform_relu_keeps_nan(dev, precision, k, fout, n):
    """gcn_transform(relu=True), plain and with live= (gnn_linear_relu_f32 / _live_f32): one
    NaN in x[0] and one in x[n - 1] make exactly those output rows NaN (torch.relu keeps NaN;
    fmaxf(NaN, 0) returned 0); every other row equals the clean run's bit for bit, and the
    clean run is relu of the plain transform."""
    from graphneuralnetwork_amd.ops import gcn_transform
    x, w = _xw(k, fout, n, dev)
    xp = x.clone()
    xp[0, 5] = NAN
    xp[n - 1, k - 1] = NAN
    ref = torch.relu(xp.double() @ w.double().t())
    assert torch.isnan(ref[0]).all() and torch.isnan(ref[n - 1]).all()
    wd = w.to(dev)
    clean = gcn_transform(x.to(dev), wd, relu=True)
    assert torch.equal(clean, torch.relu(gcn_transform(x.to(dev), wd)))
    clean = cpu(clean)
    got = cpu(gcn_transform(xp.to(dev), wd, relu=True))
    same(got, ref)
    assert bits_equal(got[1:n - 1], clean[1:n - 1])
    # live=: rows [0, live) computed, the rest left as they were
    live = n - 2
    xl = x.clone()
    xl[0, 5] = NAN
    xl[live - 1, 0] = NAN
    xl[live] = NAN  # not computed: must not show
    out = torch.full((n, fout), 7.0, device=dev)
    got = cpu(gcn_transform(xl.to(dev), wd, relu=True, out=out,
                            live=torch.tensor(live, dtype=torch.int64, device=dev)))
    same(got[:live], torch.relu(xl[:live].double() @ w.double().t()))
    assert bits_equal(got[1:live - 1], clean[1:live - 1])
    assert bool((got[live:] == 7.0).all())


@pytest.mark.parametrize("n", [37, 333])
@pytest.mark.parametrize("k,fout", [(64, 64), (128, 128), (256, 256)])
@pytest.mark.parametrize("operand", ["x", "w"])
def test_transform_relu_infinite_operand(dev, precision, k, fout, n, operand):
    """+Inf and -Inf in an operand of gcn_transform(relu=True). On the fp32 MFMA (every K = 64
    shape, and 'fp32-mfma' mode) the whole pattern is torch's: +Inf products stay +Inf, -Inf
    ones become 0 after the ReLU. The 'split-bf16' kernels (K >= 128) split an infinite
    operand into bf16 pieces inf, inf - inf = NaN, ...: every entry it touches comes out NaN,
    so there only 'no finite entry where torch has a non-finite one' is asserted. Rows (x) or
    columns (w) the infinite value does not touch equal the clean run bit for bit."""
    from graphneuralnetwork_amd.ops import gcn_transform
    x, w = _xw(k, fout, n, dev)
    xp, wp = x.clone(), w.clone()
    if operand == "x":
        xp[0, 3] = INF
        xp[n - 1, 4] = -INF
    else:
        wp[0, 3] = INF
        wp[fout - 1, 4] = -INF
    pre = xp.double() @ wp.double().t()
    ref = torch.relu(pre)
    assert torch.isposinf(ref).any() and torch.isneginf(pre).any() and not torch.isnan(ref).any()
    clean = cpu(gcn_transform(x.to(dev), w.to(dev), relu=True))
    got = cpu(gcn_transform(xp.to(dev), wp.to(dev), relu=True))
    if precision == "fp32-mfma" or k < 128:
        same(got, ref, zero=torch.isneginf(pre))
    else:
        assert not bool(torch.isfinite(got)[~torch.isfinite(ref)].any())
    if operand == "x":
        assert bits_equal(got[1:n - 1], clean[1:n - 1])
    else:
        assert bits_equal(got[:, 1:fout - 1], clean[:, 1:fout - 1])


# ------------------------------------------------------ 3: bias + ReLU + dropout epilogue
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("k,fout", [(128, 128), (64, 128)])
def test_transform_epilogue_follows_torch(dev, precision, k, fout, p):
    """gnn_gcn_transform_epi_f32, dropout_p(ReLU(x W^T + b)) with a NaN row of x and
    b[3] = +inf, b[5] = -inf, b[9] = nan, against relu(z) * keep * scale: a kept +Inf stays
    +Inf, a dropped one is Inf * 0 = NaN, NaN stays NaN kept or dropped, -Inf gives 0, and a
    dropped finite element is 0. (The kernel wrote literal 0 for a dropped element and took
    the ReLU with fmaxf: NaN -> 0.)"""
    from graphneuralnetwork_amd.ops import gcn_transform
    n, seed = 333, 2 ** 40 + 77
    x, w = _xw(k, fout, n, dev)
    b = torch.randn(fout, generator=torch.Generator().manual_seed(5))
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    before = gcn_transform(xd, wd, relu=True, bias=bd, dropout_p=p, seed=seed)
    keep = torch.from_numpy(c_oracle.dropout_keep(seed, np.arange(n)[:, None],
                                                  np.arange(fout)[None, :], p))
    scale = 1.0 / (1.0 - p)
    # finite inputs: what the epilogue gave before it followed torch on NaN (x * 0 and 0
    # differ in the sign of zero only, which == does not see)
    base = torch.relu(gcn_transform(xd, wd) + bd)
    assert torch.equal(before, torch.where(keep.to(dev), base * scale,
                                           torch.zeros((), device=dev)))
    before = cpu(before)
    for row in (0, n - 1, 100):
        xp, bp = x.clone(), b.clone()
        xp[row, 7] = NAN
        bp[3], bp[5], bp[9] = INF, -INF, NAN
        z = xp.double() @ w.double().t() + bp.double()
        ref = torch.relu(z) * keep * scale
        if p > 0:
            assert torch.isnan(ref[:, 3]).any() and torch.isposinf(ref[:, 3]).any()
        got = cpu(gcn_transform(xp.to(dev), wd, relu=True, bias=bp.to(dev), dropout_p=p,
                                seed=seed))
        same(got, ref, zero=~keep | torch.isneginf(z))
        ok = torch.ones(fout, dtype=torch.bool)
        ok[[3, 5, 9]] = False
        rows = torch.arange(n) != row
        assert bits_equal(got[rows][:, ok], before[rows][:, ok])


# ------------------------------------------------------------- 4: classifier epilogue
def test_linear_relu_classify_keeps_nan(dev, precision):
    """gnn_linear_relu_cls_f32 (y = relu(x W^T), logits = y Wd^T + bd in one launch): a NaN in
    x[r] makes row r of y and of the logits NaN and no other row (the classifier dot took the
    ReLU with fmaxf: finite logits from a NaN row)."""
    from graphneuralnetwork_amd.ops import linear_relu_classify
    n, k, fout, n_cls = 333, 128, 128, 3
    x, w = _xw(k, fout, n, dev)
    gen = torch.Generator().manual_seed(6)
    wc = torch.randn(n_cls, fout, generator=gen) * 0.2
    bc = torch.randn(n_cls, generator=gen)
    y0, l0 = cpu(*linear_relu_classify(x.to(dev), w.to(dev), wc.to(dev), bc.to(dev)))
    for row in (0, n - 1, 100):
        xp = x.clone()
        xp[row, 11] = NAN
        yr = torch.relu(xp.double() @ w.double().t())
        lr = yr @ wc.double().t() + bc.double()
        y, lg = cpu(*linear_relu_classify(xp.to(dev), w.to(dev), wc.to(dev), bc.to(dev)))
        same(y, yr)
        same(lg, lr)
        assert torch.isnan(lg[row]).all() and int(torch.isnan(lg).any(1).sum()) == 1
        rows = torch.arange(n) != row
        assert bits_equal(y[rows], y0[rows]) and bits_equal(lg[rows], l0[rows])


# ------------------------------------------------------------------ 5: fused SAGE layer
@pytest.mark.parametrize("bad", [0, 499, 250])
def test_fused_sage_layer_keeps_nan(dev, bad, monkeypatch):
    """gnn_sage_layer_f32 (F = H = 128, M = 100, k = 10, a 500-row table) with one NaN table
    row: the output rows that have it as self or as a neighbour are NaN (F.relu keeps NaN;
    the store epilogue took fmaxf), the others are bit-identical to the clean run."""
    from graphneuralnetwork_amd import ops
    monkeypatch.setattr(ops, "SAGE_FUSED_MIN_ROWS", 1)
    rng = np.random.default_rng(9)
    n, F, H, M, k = 500, 128, 128, 100, 10
    table = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, n, (M, k)))
    cidx = torch.from_numpy(rng.integers(0, n, M))
    idx[3, 2] = idx[98, 9] = bad  # a neighbour of rows 3 and 98 ...
    cidx[40] = cidx[99] = bad     # ... and the centre of rows 40 and 99
    W = torch.from_numpy((rng.standard_normal((H, 2 * F)) * 0.1).astype(np.float32))
    tp = table.clone()
    tp[bad, 17] = NAN
    hit = (idx == bad).any(1) | (cidx == bad)
    assert 4 <= int(hit.sum()) < M // 2

    def ref(t):
        t = t.double()
        return torch.relu(torch.cat([t[cidx], t[idx].mean(1)], 1) @ W.double().t())

    run = lambda t: ops.sage_layer(t.to(dev), idx.to(dev), W.to(dev), t.to(dev), cidx.to(dev))
    clean, got = run(table), run(tp)
    assert clean is not None and got is not None
    clean, got = cpu(clean, got)
    same(clean, ref(table))
    same(got, ref(tp))
    assert torch.equal(torch.isnan(got).all(1), hit)
    assert bits_equal(got[~hit], clean[~hit])


# ------------------------------------------------------------------------ 6-8: gathers
def _class_graph(seed=0, n=3000, unit=False):
    """A 3000-row graph with every row class of the plans: edgeless rows, one-edge rows, short
    rows (2..16 edges), mid rows, 24 rows longer than a wave (65..200 edges) and one hub row (row 7) of 2000 edges. Columns 0 and n - 1 are each a
    neighbour of about 4 % of the rows of every class; the hub holds column n - 1 and not
    column 0, so a poisoned row 0 must leave its 2000-edge sum (and every clamped tail lane)
    untouched and a poisoned last row must reach it. Distinct columns per row."""
    rng = np.random.default_rng(seed)
    deg = np.zeros(n, np.int64)
    cls = np.arange(n) % 4
    deg[cls == 1] = 1
    deg[cls == 2] = rng.integers(2, 17, int((cls == 2).sum()))
    deg[cls == 3] = rng.integers(17, 41, int((cls == 3).sum()))
    long_rows = rng.choice(np.arange(8, n - 8), 24, replace=False)
    deg[long_rows] = rng.integers(65, 201, 24)
    deg[7] = 2000
    src, dst = [], []
    for i in np.flatnonzero(deg):
        c = rng.choice(np.arange(1, n - 1), deg[i], replace=False)
        u = rng.random()
        if i == 7 or u < 0.04:
            c[-1] = n - 1
        elif u < 0.08:
            c[-1] = 0
        src.append(np.full(deg[i], i))
        dst.append(c)
    src, dst = np.concatenate(src), np.concatenate(dst)
    val = (np.ones(src.size) if unit else rng.standard_normal(src.size)).astype(np.float32)
    rowptr, col, val = O.coo_to_csr(src, dst, val, n)
    assert np.array_equal(np.diff(rowptr), deg)
    return rowptr, col, val


def _device_graph(rowptr, col, val, dev):
    from graphneuralnetwork_amd.graph import CsrGraph
    n = len(rowptr) - 1
    return CsrGraph(torch.as_tensor(rowptr, dtype=torch.int64, device=dev),
                    torch.as_tensor(col, dtype=torch.int32, device=dev),
                    torch.as_tensor(val, dtype=torch.float32, device=dev), n, n)


def _edges(rowptr, col):
    rows = torch.from_numpy(np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)))
    return rows, torch.from_numpy(col.astype(np.int64))


def _touch(rowptr, col, bad):
    """bool [n]: rows with an edge to column ``bad``."""
    rows, cols = _edges(rowptr, col)
    t = torch.zeros(len(rowptr) - 1, dtype=torch.bool)
    t[rows[cols == bad]] = True
    return t


@pytest.mark.parametrize("F", [8, 64, 128])
def test_spmm_relu_bias_nan_containment(dev, F):
    """spmm_forward(activation='relu', bias) over the row-class graph, clean and with X[0] /
    X[n - 1] poisoned: the rows with an edge to the poisoned row are NaN in the poisoned
    column and nowhere else, every other row is bit-identical to the clean run (no 0 * NaN
    from a clamped tail lane), the values match the float64 edge sum, and edgeless rows are
    relu(bias) exactly."""
    from graphneuralnetwork_amd.ops import spmm_forward
    rowptr, col, val = _class_graph(1)
    n = len(rowptr) - 1
    g = _device_graph(rowptr, col, val, dev)
    plan = g.plan(64)
    assert plan.n_small and plan.n_mid and plan.n_long  # every class exists (at seg_len 64)
    rows, cols = _edges(rowptr, col)
    gen = torch.Generator().manual_seed(F)
    X = torch.randn(n, F, generator=gen)
    b = torch.randn(F, generator=gen)
    v64 = torch.from_numpy(val).double()

    def ref(x):
        y = torch.zeros(n, F, dtype=torch.float64)
        y.index_add_(0, rows, v64[:, None] * x.double()[cols])
        return torch.relu(y + b.double())

    empty = torch.from_numpy(np.diff(rowptr) == 0)
    for seg in (None, 64):  # the default segment length, and one that splits the long rows
        run = lambda x: cpu(spmm_forward(g, x.to(dev), b.to(dev), activation="relu",
                                         seg_len=seg))
        clean = run(X)
        same(clean, ref(X))
        assert torch.equal(clean[empty], torch.relu(b).expand(int(empty.sum()), F))
        for bad in (0, n - 1):
            Xp = X.clone()
            Xp[bad, F - 3] = NAN
            got = run(Xp)
            same(got, ref(Xp))
            hit = _touch(rowptr, col, bad)
            assert hit[7] == (bad == n - 1) and 50 < int(hit.sum()) < 400
            nan = torch.isnan(got)
            assert torch.equal(nan[:, F - 3], hit) and int(nan.sum()) == int(hit.sum())
            assert bits_equal(got[~hit], clean[~hit])
            assert torch.equal(got[empty], torch.relu(b).expand(int(empty.sum()), F))


def _gat_ref(rowptr, col, wh, a_s, a_d, H, fh, slope, sparse, keep, scale):
    """Float64 statement of both GAT layers over the edges of a CSR graph: the formula of
    tests/test_gat_gpu.py's _torch_gat (softmax over a row's edges of +-leaky_relu(el_i +
    er_j), attention times keep * scale, weighted sum of the Wh rows) without its [n, n, H]
    tensors, which 3000 nodes would make 0.6 GB each. An edgeless row is the uniform average
    of every row in the dense layer (softmax over n equal -9e15 logits, layers.py:28-32) and
    0 / 0 = NaN in the sparse one (layers.py:122)."""
    n = wh.shape[0]
    rows, cols = _edges(rowptr, col)
    W3 = wh.double().view(n, H, fh)
    el = (W3 * a_s.double().view(H, fh)).sum(-1)
    er = (W3 * a_d.double().view(H, fh)).sum(-1)
    x = torch.nn.functional.leaky_relu(el[rows] + er[cols], slope)  # [E, H]
    z = -x if sparse else x
    ix = rows[:, None].expand(-1, H)
    m = torch.full((n, H), -INF, dtype=torch.float64).scatter_reduce(0, ix, z, "amax")
    e = torch.exp(z - m[rows])
    att = e / torch.zeros(n, H, dtype=torch.float64).index_add_(0, rows, e)[rows]
    att = att * keep * scale
    out = torch.zeros(n, H, fh, dtype=torch.float64).index_add_(0, rows, att[:, :, None] * W3[cols])
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    out[empty] = NAN if sparse else W3.mean(0)
    return out.reshape(n, H * fh)


def _gat_setup(H, fh, dev):
    rowptr, col, val = _class_graph(2, unit=True)
    n = len(rowptr) - 1
    gen = torch.Generator().manual_seed(10 * H + fh)
    wh = torch.randn(n, H * fh, generator=gen) * 0.5
    a_s = torch.randn(H * fh, generator=gen) * 0.3
    a_d = torch.randn(H * fh, generator=gen) * 0.3
    return rowptr, col, _device_graph(rowptr, col, val, dev), wh, a_s, a_d


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H,fh", [(8, 8), (1, 8)])
@pytest.mark.parametrize("sparse", [False, True])
def test_gat_aggregate_nan_containment(dev, sparse, H, fh, p):
    """gat_aggregate (dense and sparse layer, with and without attention dropout, er loaded
    and recomputed from the gathered rows) over the row-class graph, clean and with Wh[0] /
    Wh[n - 1] all NaN (el, er from the poisoned Wh): the poisoned node's own row (its el) and
    every row with an edge to it are NaN in every head -- in the dense layer also the
    edgeless rows, which average every row of Wh -- and all other rows are bit-identical to
    the clean run; values against the float64 restatement under the oracle's (edge, head)
    keep mask."""
    from graphneuralnetwork_amd.ops import GAT_DENSE, GAT_SPARSE, gat_aggregate, gat_logits
    rowptr, col, g, wh, a_s, a_d = _gat_setup(H, fh, dev)
    n = len(rowptr) - 1
    seed = 991
    keep = torch.from_numpy(c_oracle.dropout_keep(seed, np.arange(col.size)[:, None],
                                                  np.arange(H)[None, :], p))
    scale = 1.0 / (1.0 - p)
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    asd, add = a_s.to(dev), a_d.to(dev)

    def run(w, rec):
        wd = w.to(dev)
        el, er = gat_logits(wd, H, fh, asd, add)
        return cpu(gat_aggregate(g, wd, el, er, H, fh, 0.2,
                                 GAT_SPARSE if sparse else GAT_DENSE, None, dropout_p=p,
                                 seed=seed, a_dst=add if rec else None))

    for rec in (False, True):
        clean = run(wh, rec)
        same(clean, _gat_ref(rowptr, col, wh, a_s, a_d, H, fh, 0.2, sparse, keep, scale))
        for bad in (0, n - 1):
            wp = wh.clone()
            wp[bad] = NAN
            got = run(wp, rec)
            same(got, _gat_ref(rowptr, col, wp, a_s, a_d, H, fh, 0.2, sparse, keep, scale))
            hit = _touch(rowptr, col, bad)
            hit[bad] = True
            if not sparse:
                hit |= empty
            assert torch.equal(torch.isnan(got).all(1), hit | empty)
            assert not bool(torch.isnan(got[~(hit | empty)]).any())
            assert bits_equal(got[~hit], clean[~hit])


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H,fh", [(8, 8), (1, 8)])
@pytest.mark.parametrize("sparse", [False, True])
def test_gat_backward_nan_containment(dev, sparse, H, fh, p):
    """_GatLayerFn's backward under a finite upstream gradient, setup as above: containment
    only. The forward's NaN rows are S = {poisoned node} + {rows with an edge to it}; a row
    of S hands NaN to the Wh gradient of every column it holds (its softmax normaliser is
    NaN) and to its own (through el). The gradient rows of every other node -- no edge from
    a row of S -- equal the clean run's bit for bit. (No activation: the dense layer's
    edgeless rows are NaN in the forward, and an ELU backward would spread them to every
    row through the uniform average.)"""
    from graphneuralnetwork_amd.gat import _GatLayerFn
    rowptr, col, g, wh, a_s, a_d = _gat_setup(H, fh, dev)
    n = len(rowptr) - 1
    rows, cols = _edges(rowptr, col)
    R = torch.randn(n, H * fh, generator=torch.Generator().manual_seed(3)).to(dev)

    def grad(w):
        W = w.to(dev).requires_grad_()
        s, d = a_s.to(dev).requires_grad_(), a_d.to(dev).requires_grad_()
        out = _GatLayerFn.apply(W, s, d, g, H, fh, 0.2, 1 if sparse else 0, None, p, 4321)
        out.backward(R)
        return cpu(W.grad)

    clean = grad(wh)
    assert bool(torch.isfinite(clean).all())
    for bad in (0, n - 1):
        wp = wh.clone()
        wp[bad] = NAN
        got = grad(wp)
        S = _touch(rowptr, col, bad)
        S[bad] = True
        hit = S.clone()
        hit[cols[S[rows]]] = True
        assert 0 < int((~hit).sum())
        assert bool(torch.isnan(got[bad]).all())
        assert bits_equal(got[~hit], clean[~hit])


# ------------------------------------------------------------------------ 9: the model
@pytest.mark.parametrize("mode,r", [("train", 0), ("train", 2999), ("eval", 0)])
def test_gcn_model_nan_reaches_the_loss(dev, mode, r, monkeypatch):
    """GCN_Model(128, 128, 7, 2, 0.5) on a symmetric 3000-node graph (below XCD_MIN_NNZ: no
    training order) with one NaN in X[r]: the logits' non-finite pattern is the float64
    restatement's (the 2-hop neighbourhood of r), the finite rows are close, the NLL loss is
    NaN -- a diverged run must not report a finite loss -- and every parameter-gradient entry
    that is non-finite in the float64 autograd reference is non-finite here.

    Elementwise parity of the fused backward at a NaN position is not asserted: the backward
    keeps only H, and at a NaN it cannot tell a kept element from a dropped one (it passes the
    gradient where H > 0, so 0 at a NaN, where torch passes it through). This test is what
    pins the backward: the NaN reaches every gradient through the rows around the NaN ones."""
    from graphneuralnetwork_amd import gcn as gcn_mod
    from graphneuralnetwork_amd.gcn import GCN_Model
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    n, C, seed = 3000, 7, 24680
    rng = np.random.default_rng(4)
    s, d = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    g = gcn_adjacency(torch.from_numpy(s), torch.from_numpy(d), n, device=dev)
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    rows, cols = _edges(rowptr, col)
    v64 = g.val.cpu().double()
    torch.manual_seed(3)
    net = GCN_Model(128, 128, C, 2, 0.5).to(dev)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for m in (net.gcn_blocks.gcn0, net.gcn_blocks.gcn1):
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
    X = torch.randn(n, 128, generator=gen)
    X[r, 20] = NAN
    y = torch.randint(0, C, (n,), generator=gen)
    monkeypatch.setattr(gcn_mod, "dropout_seed", lambda: seed)
    spans = []
    real = gcn_mod._fuse_train
    monkeypatch.setattr(gcn_mod, "_fuse_train", lambda *a: spans.append(real(*a)) or spans[-1])
    params = [net.gcn_blocks.gcn0.dense.weight, net.gcn_blocks.gcn0.bias,
              net.gcn_blocks.gcn1.dense.weight, net.gcn_blocks.gcn1.bias]
    W1, b1, W2, b2 = (t.detach().cpu().double().requires_grad_() for t in params)
    A = lambda v: torch.zeros(n, v.shape[1], dtype=torch.float64).index_add(
        0, rows, v64[:, None] * v[cols])
    h = torch.relu(A(X.double()) @ W1.t() + b1)
    if mode == "train":
        keep = torch.from_numpy(c_oracle.dropout_keep(seed, np.arange(n)[:, None],
                                                      np.arange(128)[None, :], 0.5))
        h = h * keep * 2.0
    ref = A(h @ W2.t()) + b2
    hop1 = _touch(rowptr, col, r)
    hop2 = hop1.clone()
    hop2[rows[hop1[cols]]] = True
    assert hop1[r] and torch.equal(torch.isnan(ref).all(1), hop2) and 3 < int(hop2.sum()) < 300
    assert torch.equal(torch.isnan(ref).any(1), hop2)
    nll = lambda t, lab: torch.nn.functional.nll_loss(torch.log_softmax(t, 1), lab)
    if mode == "eval":
        net.eval()
        with torch.no_grad():
            logits = net(X.to(dev), g)
        same(logits, ref)
        assert bool(torch.isnan(nll(logits, y.to(dev))))
        return
    net.train()
    logits = net(X.to(dev), g)
    assert spans == [3, 0]  # layer 1 + ReLU + Dropout as one op
    same(logits, ref)
    loss = nll(logits, y.to(dev))
    assert bool(torch.isnan(loss)) and bool(torch.isnan(nll(ref, y)))
    loss.backward()
    nll(ref, y).backward()
    for got, want in zip(params, (W1, b1, W2, b2)):
        bad = ~torch.isfinite(want.grad)
        assert bool(bad.any())
        assert not bool(torch.isfinite(got.grad.cpu())[bad].any())
