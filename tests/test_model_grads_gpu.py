"""One training step of every drop-in model against float64 autograd of the reference math.

Each case draws fp32 weights, copies them to a plain-torch float64 restatement of the model
(dense N x N adjacency, masked_fill, softmax, torch.max, torch.cat -- the way the reference
writes it, not the way the kernels do), shows that restatement equal to the numpy oracle's
forward (oracle/gnn_oracle.py, itself pinned to the reference's golden outputs) at 1e-9, and
then compares one HIP training step with the float64 step: logits, loss, the gradient of every
named parameter (none may be None) and of the inputs that take one.

Kinks. ReLU, LeakyReLU and max / argmax are not differentiable at one point; an fp32 forward
may take the other branch there and move a gradient by a whole term. Every case therefore
asserts, on its float64 reference, that no such argument lies within KINK (1e-4) x the largest
magnitude of its tensor of the kink: |pre-activation| for ReLU and for LeakyReLU (the attention
logits of the graph's edges -- the masked pairs never reach an output), the gap between the two
largest candidates for max / argmax. This is a property of the fixture: ``_settle`` redraws, with
the test's seeded generator, the bias column / weight row / attention vector / table column that
owns an offending element until the reference is clear (earliest stage first: a later parameter
never moves an earlier pre-activation). One class of ties is structural and not a kink: a max over
post-ReLU candidates that are all exact zeros. With every pre-activation at least the bound below
zero the max is the constant 0 in a neighbourhood (gradient 0 through either candidate, argmax
the first index by the first-maximum rule on both sides); these are left out of the max gap and
nowhere else. No element is left out of any comparison.

Tolerances: the project's (tests/test_training_gpu.py ``close``: rtol 1e-4, atol 1e-5 x max|ref|;
rtol 2e-4 for GAT / HAN gradients as test_gat_backward_vs_torch has it). Where a case passes
``ref32`` -- the same restatement evaluated in fp32 by torch on the CPU -- the absolute part is the
larger of the project's and 4 x that evaluation's own largest deviation from float64.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import c_oracle
from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
KINK = 1e-4
F64 = torch.float64


# ------------------------------------------------------------------ comparison
def _np(t):
    return t.detach().cpu().double().numpy()


def close(got, ref, rtol=1e-4, ref32=None, what=""):
    a, b = _np(got), _np(ref)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    atol = 1e-5 * scale
    dev32 = None
    if ref32 is not None:
        dev32 = float(np.abs(_np(ref32) - b).max()) if b.size else 0.0
        atol = max(atol, 4.0 * dev32)
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {float(np.abs(b).max()) if b.size else 0:.3e} "
          f"atol {atol:.3e}" + (f" fp32-restatement dev {dev32:.3e}" if dev32 is not None else ""))
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def _compare(tag, got, ref, grad_rtol=1e-4, ref32=None):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k in ref:
        if ref[k] is None:  # an input the model does not differentiate through (the argmax of
            assert got[k] is None, k  # MAX, the centre rows in gcn mode): none on either side
            assert k.startswith(("grad:center", "grad:neigh")), k
            continue
        close(got[k], ref[k], rtol=1e-4 if k in ("logits", "loss") else grad_rtol,
              ref32=None if ref32 is None else ref32[k], what=f"{tag} {k}")


def _params(model, dtype=F64):
    return {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in model.named_parameters()}


def _param_grads(model):
    out = {}
    for k, v in model.named_parameters():
        assert v.grad is not None, f"no gradient for {k}"
        out["grad:" + k] = v.grad
    return out


def _ref_grads(P):
    out = {}
    for k, v in P.items():
        assert v.grad is not None, f"reference: no gradient for {k}"
        out["grad:" + k] = v.grad
    return out


# ------------------------------------------------------------------ kinks
def _settle(run, redraw, tries=400):
    """run() -> [(stage, name, per-column smallest distance, largest magnitude)];
    redraw(stage, name, columns) redraws what owns them. Earliest stage first."""
    for _ in range(tries):
        with torch.no_grad():
            rec = run()
        bad = None
        for stage, name, m, mx in rec:
            cols = torch.nonzero(m < KINK * mx).flatten().tolist()
            if cols and (bad is None or stage < bad[0]):
                bad = (stage, name, cols)
        if bad is None:
            return
        redraw(*bad)
    raise AssertionError("the fixture does not clear its kinks")


def _assert_kinks(rec, tag):
    assert rec
    worst = min(float(m.min()) / mx for _, _, m, mx in rec)
    print(f"{tag}: smallest kink distance {worst:.3e} x max|tensor| over {len(rec)} tensors")
    for stage, name, m, mx in rec:
        assert float(m.min()) >= KINK * mx, (tag, stage, name, float(m.min()), mx)


# ------------------------------------------------------------------ graph fixture
@functools.lru_cache(maxsize=None)
def _fixture_edges(n=320, seed=0, n_iso=8, n_one=16, long_deg=200):
    """Form (a): n_iso isolated nodes (edgeless rows), n_one one-edge rows, one row of long_deg
    edges, a hub column most rows point to, one node nothing points to, a bulk of degree 2-12;
    non-symmetric, no self-loop anywhere. Returns sorted unique (row, col)."""
    rng = np.random.default_rng(seed)
    long_row, hub, src_only = n_iso + n_one, n_iso + n_one + 1, n_iso + n_one + 2
    targets = np.setdiff1d(np.arange(n_iso, n), [src_only])
    s, d = [], []
    for i in range(n_iso, n_iso + n_one):
        s.append(i)
        d.append(int(rng.choice(targets[targets != i])))
    pick = rng.choice(targets[targets != long_row], long_deg, replace=False)
    s += [long_row] * long_deg
    d += pick.tolist()
    plain = targets[targets != hub]
    for i in range(hub, n):
        deg = int(rng.integers(2, 13))
        to_hub = i != hub and rng.random() < 0.75
        others = rng.choice(plain[plain != i], deg - int(to_hub), replace=False)
        s += [i] * deg
        d += others.tolist() + ([hub] if to_hub else [])
    key = np.unique(np.asarray(s, np.int64) * n + np.asarray(d, np.int64))
    r, c = key // n, key % n
    deg = np.bincount(r, minlength=n)
    indeg = np.bincount(c, minlength=n)
    assert (deg[:n_iso] == 0).all() and (indeg[:n_iso] == 0).all()
    assert (deg[n_iso:n_iso + n_one] == 1).all() and deg[long_row] == long_deg
    assert ((deg[hub:] >= 2) & (deg[hub:] <= 12)).all()
    assert indeg[hub] > n // 2 and indeg[src_only] == 0 and deg[src_only] >= 2
    assert (r != c).all()
    return r, c


def _with_loops(r, c, n, nodes):
    nodes = np.asarray(nodes, np.int64)
    key = np.unique(np.concatenate([r * n + c, nodes * (n + 1)]))
    return key // n, key % n


def _symmetrised(r, c, n, loops):
    """Form (b): A or A^T, self-loops on ``loops``."""
    key = np.unique(np.concatenate([r * n + c, c * n + r, np.asarray(loops, np.int64) * (n + 1)]))
    return key // n, key % n


def _csr(r, c, n):
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return rowptr, c.astype(np.int32)


def _graph(dev, r, c, n, symmetric=False, val=None):
    from graphneuralnetwork_amd.graph import CsrGraph
    rowptr, col = _csr(r, c, n)
    v = torch.ones(col.size) if val is None else torch.from_numpy(val)
    return CsrGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev),
                    v.float().to(dev), n, n, symmetric=symmetric)


def _mask(r, c, n):
    m = torch.zeros(n, n, dtype=torch.bool)
    m[torch.from_numpy(r), torch.from_numpy(c)] = True
    return m


# ------------------------------------------------------------------ GAT / HAN restatement
def _hash3(seed: int, edge: np.ndarray, head: int) -> np.ndarray:
    """csrc/gat.hip hash3 in numpy uint32 arithmetic (the attention dropout stream)."""
    M = np.uint64(0xFFFFFFFF)
    e = edge.astype(np.uint64)
    h = np.uint64(seed & 0xFFFFFFFF) ^ ((np.uint64(seed >> 32) * np.uint64(0x27d4eb2f)) & M)
    h = h ^ ((e & M) * np.uint64(0x9e3779b9) & M)
    h = h ^ (((e >> np.uint64(32)) * np.uint64(0x85ebca6b)) & M)
    h = h ^ ((np.uint64(head) * np.uint64(0xc2b2ae35)) & M)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & M
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & M
    h = h ^ (h >> np.uint64(16))
    return h


def _att_keep(seed, r, c, n, head, p):
    """[n, n] 0/1 keep matrix of the attention dropout: (seed, CSR edge index, head)."""
    keep = (_hash3(seed, np.arange(r.size), head) >> np.uint64(8)).astype(np.float64) \
        / 16777216.0 >= p
    m = torch.zeros(n, n, dtype=F64)
    m[torch.from_numpy(r), torch.from_numpy(c)] = torch.from_numpy(keep.astype(np.float64))
    return m


def _elem_keep(seed, rows, cols, p):
    return torch.from_numpy(c_oracle.dropout_keep(seed, np.arange(rows)[:, None],
                                                  np.arange(cols)[None, :], p).astype(np.float64))


def _ref_att_layer(h, mask, W, a, alpha, concat, sparse, keep=None, p=0.0, rec=None, name=""):
    """GraphAttentionLayer / SpGraphAttentionLayer.forward (GAT/models/layers.py:22-37, :94-131)
    over the dense pair matrix; ``keep`` where the reference applies F.dropout."""
    Wh = h @ W
    fo = W.shape[1]
    a = a.reshape(-1)
    t = (Wh @ a[:fo])[:, None] + (Wh @ a[fo:])[None, :]
    if rec is not None:
        te = t.detach()[mask].abs()
        rec.append((len(rec), name, te.min().reshape(1), float(te.max())))
    e = F.leaky_relu(t, alpha)
    if sparse:
        ee = torch.exp(torch.where(mask, -e, torch.full_like(e, float("-inf"))))
        rowsum = ee.sum(1, keepdim=True)
        if keep is not None:
            ee = ee * keep.to(ee.dtype) / (1.0 - p)
        out = (ee @ Wh) / rowsum
    else:
        att = torch.softmax(e.masked_fill(~mask, -9e15), dim=1)
        if keep is not None:
            att = att * keep.to(att.dtype) / (1.0 - p)
        out = att @ Wh
    return F.elu(out) if concat else out


def _ref_gat_model(P, x, mask, nheads, alpha, sparse, drop=None, rec=None, prefix="",
                   out_att=True):
    """GATBase.forward (GAT/models/GAT.py:14-18); without out_att, GATConv's second ELU
    (HAN/models/NodeAttention.py:59-62)."""
    p = drop["p"] if drop else 0.0
    if drop:
        x = x * drop["x"].to(x.dtype) / (1.0 - p)
    hs = [_ref_att_layer(x, mask, P[f"{prefix}attentions.AttentionHead{i}.W"],
                         P[f"{prefix}attentions.AttentionHead{i}.a"], alpha, True, sparse,
                         drop["att"][i] if drop else None, p, rec,
                         f"{prefix}attentions.AttentionHead{i}") for i in range(nheads)]
    h = torch.cat(hs, dim=1)
    if drop:
        h = h * drop["hid"].to(h.dtype) / (1.0 - p)
    if not out_att:
        return F.elu(h)
    return F.elu(_ref_att_layer(h, mask, P[f"{prefix}out_att.W"], P[f"{prefix}out_att.a"], alpha,
                                False, sparse, drop["out"] if drop else None, p, rec,
                                f"{prefix}out_att"))


def _redraw_attention(model):
    from graphneuralnetwork_amd.gat import SpGraphAttentionLayer
    mods = dict(model.named_modules())

    def redraw(stage, name, cols):
        m = mods[name]
        init = torch.nn.init.xavier_normal_ if isinstance(m, SpGraphAttentionLayer) \
            else torch.nn.init.xavier_uniform_
        init(m.a.data, gain=1.414)
    return redraw


def _ce_step(run, P, inputs, labels):
    """loss.backward() of cross-entropy on the restatement; gradients of P and ``inputs``."""
    logits = run(P)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    out = {"logits": logits, "loss": loss, **_ref_grads(P)}
    for k, v in inputs.items():
        assert v.grad is not None, k
        out["grad:" + k] = v.grad
    return out


def _gat_heads_np(model):
    return ([(_np(m.W), _np(m.a)) for m in model.attentions],
            (_np(model.out_att.W), _np(model.out_att.a)) if getattr(model, "out_att", None)
            is not None else None)


GAT_SHAPES = [(64, 8, 7, 8), (24, 5, 3, 3), (32, 16, 4, 1)]
GAT_CASES = [(s, v) for s in GAT_SHAPES for v in ("a", "b_ordered")] + [(GAT_SHAPES[0], "a_seg16")]


def _gat_edges(kind, variant, n=320):
    r, c = _fixture_edges(n)
    if variant.startswith("a"):
        if kind == "SpGAT":  # 0 / 0 on an edgeless row: the reference asserts on NaN
            r, c = _with_loops(r, c, n, np.arange(8))
        return r, c, False
    loops = np.arange(n) if kind == "SpGAT" else np.arange(8, n)
    r, c = _symmetrised(r, c, n, loops)
    return r, c, True


@pytest.mark.parametrize("shape,variant", GAT_CASES,
                         ids=[f"{'x'.join(map(str, s))}-{v}" for s, v in GAT_CASES])
@pytest.mark.parametrize("kind", ["GAT", "SpGAT"])
def test_gat_model_step_vs_float64(dev, kind, shape, variant, monkeypatch):
    """GAT / SpGAT, dropout 0: graph (a) (for GAT with its 8 edgeless rows: the column-mean fill
    and its backward term under ELU), graph (b) with the training order P A P^T forced at this
    size, and once with the long-row threshold at 16. out_att is zero-padded 7 -> 8 and 3 -> 4,
    unpadded at 4; head width 5 is one the two-pass backward refuses. SpGAT's absolute bound is
    max(project, 4 x the fp32 CPU restatement's own deviation from float64), measured per
    quantity and printed; on the CPU that deviation was at most 5.4e-7 x max(1, max|ref|) over
    these cases (logits, loss and gradients alike), so 4 x it stays below the project's
    1e-5 x max|ref|, which therefore governs."""
    from graphneuralnetwork_amd import gat as gat_mod
    from graphneuralnetwork_amd import graph as graph_mod
    from graphneuralnetwork_amd import ops
    nfeat, nhid, nclass, heads = shape
    n, alpha, sparse = 320, 0.2, kind == "SpGAT"
    torch.manual_seed(1000 + nfeat + (7 if sparse else 0))
    r, c, sym = _gat_edges(kind, variant)
    mask = _mask(r, c, n)
    model = getattr(gat_mod, kind)(nfeat, nhid, nclass, 0.0, alpha, heads).train()
    x = 0.5 * torch.randn(n, nfeat)
    labels = torch.randint(0, nclass, (n,))

    def run(P, xx, rec=None):
        return _ref_gat_model(P, xx, mask, heads, alpha, sparse, rec=rec)

    def kinks():
        rec = []
        run(_params(model), x.double(), rec)
        return rec
    _settle(kinks, _redraw_attention(model))
    _assert_kinks(kinks(), f"{kind} {shape} {variant}")

    P, x64 = _params(model), x.double().requires_grad_()
    ref = _ce_step(lambda q: run(q, x64), P, {"x": x64}, labels)
    hp, op = _gat_heads_np(model)
    np.testing.assert_allclose(_np(ref["logits"]),
                               O.gat_model(x.numpy(), mask.numpy().astype(np.float64), hp, op,
                                           alpha, sparse), rtol=1e-9, atol=1e-9)
    ref32 = None
    if sparse:
        P32, x32 = _params(model, torch.float32), x.clone().requires_grad_()
        ref32 = _ce_step(lambda q: run(q, x32), P32, {"x": x32}, labels)

    if variant == "b_ordered":
        monkeypatch.setattr(ops, "HUB_MIN_X_BYTES", 0)
    if variant == "a_seg16":
        monkeypatch.setattr(graph_mod, "seg_len_for", lambda f, *a: 16)
        monkeypatch.setattr(ops, "seg_len_for", graph_mod.seg_len_for)
    g = _graph(dev, r, c, n, symmetric=sym)
    model.to(dev)
    xg = x.to(dev).requires_grad_()
    y = model(xg, g)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    assert (("_nodeorder",) in g._plans) == (variant == "b_ordered")
    if kind == "GAT":
        assert g.has_empty_rows()
    got = {"logits": y, "loss": loss, "grad:x": xg.grad, **_param_grads(model)}
    _compare(f"{kind} {shape} {variant}", got, ref, grad_rtol=2e-4, ref32=ref32)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused_hidden", "separate_hidden"])
@pytest.mark.parametrize("kind", ["GAT", "SpGAT"])
def test_gat_model_dropout_step_vs_float64(dev, kind, fuse, monkeypatch):
    """Dropout 0.5 on graph (a) with self-loops on its 8 rows (the dense layer's column-mean fill
    ignores attention dropout, the reference does not), training order off. Four seeds are drawn
    -- input dropout (ops), heads' attention (gat), hidden dropout (ops), out_att's attention (gat)
    -- and the float64 step applies the same masks where the reference applies F.dropout, scale
    1 / (1 - p): the oracle's (seed, row, column) mask for the two element dropouts, the (seed,
    CSR edge, head) hash for the attention. With the hidden dropout inside the heads' op and as a
    pass of its own. SpGAT's bound as in test_gat_model_step_vs_float64 (fp32 restatement's
    deviation on the CPU: at most 4.1e-7 x max(1, max|ref|))."""
    from graphneuralnetwork_amd import gat as gat_mod
    from graphneuralnetwork_amd import ops
    nfeat, nhid, nclass, heads = 64, 8, 7, 8
    n, alpha, p, sparse = 320, 0.2, 0.5, kind == "SpGAT"
    torch.manual_seed(2000 + (7 if sparse else 0))
    r, c = _with_loops(*_fixture_edges(n), n, np.arange(8))
    mask = _mask(r, c, n)
    model = getattr(gat_mod, kind)(nfeat, nhid, nclass, p, alpha, heads).train()
    x = 0.5 * torch.randn(n, nfeat)
    labels = torch.randint(0, nclass, (n,))
    step_seed = 4321
    torch.manual_seed(step_seed)  # the model draws its seeds from torch's generator
    want = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(4)]
    drop = {"p": p, "x": _elem_keep(want[0], n, nfeat, p),
            "att": [_att_keep(want[1], r, c, n, h, p) for h in range(heads)],
            "hid": _elem_keep(want[2], n, nhid * heads, p),
            "out": _att_keep(want[3], r, c, n, 0, p)}

    def run(P, xx, rec=None, d=drop):
        return _ref_gat_model(P, xx, mask, heads, alpha, sparse, drop=d, rec=rec)

    def kinks():
        rec = []
        run(_params(model), x.double(), rec)
        return rec
    torch.manual_seed(2001)
    _settle(kinks, _redraw_attention(model))
    _assert_kinks(kinks(), f"{kind} dropout")

    P, x64 = _params(model), x.double().requires_grad_()
    ref = _ce_step(lambda q: run(q, x64), P, {"x": x64}, labels)
    hp, op = _gat_heads_np(model)
    with torch.no_grad():  # the restatement without masks is the oracle's eval forward
        np.testing.assert_allclose(
            _np(run(_params(model), x.double(), d=None)),
            O.gat_model(x.numpy(), mask.numpy().astype(np.float64), hp, op, alpha, sparse),
            rtol=1e-9, atol=1e-9)
    ref32 = None
    if sparse:
        P32, x32 = _params(model, torch.float32), x.clone().requires_grad_()
        ref32 = _ce_step(lambda q: run(q, x32), P32, {"x": x32}, labels)

    monkeypatch.setattr(gat_mod, "GAT_FUSE_OUT_DROPOUT", fuse)
    drawn = []
    real_ops, real_gat = ops.dropout_seed, gat_mod._dropout_seed
    monkeypatch.setattr(ops, "dropout_seed",
                        lambda: drawn.append(("ops", real_ops())) or drawn[-1][1])
    monkeypatch.setattr(gat_mod, "_dropout_seed",
                        lambda: drawn.append(("gat", real_gat())) or drawn[-1][1])
    g = _graph(dev, r, c, n)
    model.to(dev)
    xg = x.to(dev).requires_grad_()
    torch.manual_seed(step_seed)
    y = model(xg, g)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    assert drawn == [("ops", want[0]), ("gat", want[1]), ("ops", want[2]), ("gat", want[3])]
    assert ("_nodeorder",) not in g._plans
    got = {"logits": y, "loss": loss, "grad:x": xg.grad, **_param_grads(model)}
    _compare(f"{kind} dropout fuse={fuse}", got, ref, grad_rtol=2e-4, ref32=ref32)


# ------------------------------------------------------------------ HAN
def _han_graphs(n=150):
    """Three metapath graphs from the fixture's construction; metapath 0 keeps one edgeless row,
    every other row has a self-loop."""
    out = []
    for m in range(3):
        n_iso = 1 if m == 0 else 0
        r, c = _fixture_edges(n, 10 + m, n_iso, 8, 90)
        r, c = _with_loops(r, c, n, np.arange(n_iso, n))
        out.append(_mask(r, c, n))
    assert int((out[0].sum(1) == 0).sum()) == 1 and all(int((m.sum(1) == 0).sum()) == 0
                                                        for m in out[1:])
    return out


def _ref_han(P, h, masks, num_heads, alpha=0.2, rec=None):
    """HANModel.forward (HAN/models/HAN.py:17-23, :37-41; SemanticAttention.py:15-20)."""
    for l, nh in enumerate(num_heads):
        z = torch.stack([_ref_gat_model(P, h, masks[m], nh, alpha, False, rec=rec,
                                        prefix=f"layers.{l}.gat_layers.meta_path_model{m}.",
                                        out_att=False) for m in range(len(masks))], dim=1)
        pre = f"layers.{l}.semantic_attention.project."
        w = (torch.tanh(z @ P[pre + "0.weight"].t() + P[pre + "0.bias"])
             @ P[pre + "2.weight"].t()).mean(0)
        h = (torch.softmax(w, dim=0).unsqueeze(0) * z).sum(1)
    return h @ P["predict.weight"].t() + P["predict.bias"]


def test_han_model_step_vs_float64(dev):
    """HANModel(3, 32, 8, 4, [4, 2]) on 150 nodes: every head's W / a, both semantic attentions,
    ``predict`` and h against float64."""
    from graphneuralnetwork_amd.han import HANModel
    n, num_heads = 150, [4, 2]
    torch.manual_seed(3000)
    masks = _han_graphs(n)
    model = HANModel(3, 32, 8, 4, num_heads, dropout=0.0).train()
    h = 0.5 * torch.randn(n, 32)
    labels = torch.randint(0, 4, (n,))

    def kinks():
        rec = []
        _ref_han(_params(model), h.double(), masks, num_heads, rec=rec)
        return rec
    _settle(kinks, _redraw_attention(model))
    _assert_kinks(kinks(), "HAN")
    P, h64 = _params(model), h.double().requires_grad_()
    ref = _ce_step(lambda q: _ref_han(q, h64, masks, num_heads), P, {"h": h64}, labels)
    gs_np = [m.numpy().astype(np.float64) for m in masks]
    hn = h.numpy()
    for layer in model.layers:
        heads = [[(_np(a.W), _np(a.a)) for a in conv.attentions] for conv in layer.gat_layers]
        pr = layer.semantic_attention.project
        hn = O.han_layer(gs_np, hn, heads, (_np(pr[0].weight), _np(pr[0].bias), _np(pr[2].weight)))
    np.testing.assert_allclose(_np(ref["logits"]),
                               hn @ _np(model.predict.weight).T + _np(model.predict.bias),
                               rtol=1e-9, atol=1e-9)
    model.to(dev)
    hg = h.to(dev).requires_grad_()
    y = model([m.float().to(dev) for m in masks], hg)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    got = {"logits": y, "loss": loss, "grad:h": hg.grad, **_param_grads(model)}
    _compare("HAN", got, ref, grad_rtol=2e-4)


def test_han_gatconv_classes_step_vs_float64(dev):
    """GATConv(32, 8, 0, 4, num_class=5) alone on metapath 0 (one edgeless row; out_att 5 -> 8)."""
    from graphneuralnetwork_amd.han import GATConv
    n = 150
    torch.manual_seed(3100)
    mask = _han_graphs(n)[0]
    conv = GATConv(32, 8, 0.0, 4, num_class=5).train()
    h = 0.5 * torch.randn(n, 32)
    labels = torch.randint(0, 5, (n,))

    def run(P, hh, rec=None):
        return _ref_gat_model(P, hh, mask, 4, 0.2, False, rec=rec)

    def kinks():
        rec = []
        run(_params(conv), h.double(), rec)
        return rec
    _settle(kinks, _redraw_attention(conv))
    _assert_kinks(kinks(), "GATConv")
    P, h64 = _params(conv), h.double().requires_grad_()
    ref = _ce_step(lambda q: run(q, h64), P, {"h": h64}, labels)
    hp, op = _gat_heads_np(conv)
    np.testing.assert_allclose(_np(ref["logits"]),
                               O.han_gatconv(h.numpy(), mask.numpy().astype(np.float64), hp, 0.2,
                                             op),
                               rtol=1e-9, atol=1e-9)
    conv.to(dev)
    hg = h.to(dev).requires_grad_()
    y = conv(hg, mask.float().to(dev))
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    got = {"logits": y, "loss": loss, "grad:h": hg.grad, **_param_grads(conv)}
    _compare("GATConv", got, ref, grad_rtol=2e-4)


# ------------------------------------------------------------------ GCN
def _ref_gcn(P, X, A, layers, keeps=None, p=0.0, rec=None):
    """GCN_Model.forward (GCN/GCN.py:21-27, :41-47): spmm(A, X W^T) + b, ReLU, Dropout."""
    h = X
    for i in range(layers):
        h = A @ (h @ P[f"gcn_blocks.gcn{i}.dense.weight"].t()) + P[f"gcn_blocks.gcn{i}.bias"]
        if i != layers - 1:
            if rec is not None:
                d = h.detach().abs()
                rec.append((i, f"gcn{i}", d.min(0).values, float(d.max())))
            h = torch.relu(h)
            if keeps is not None:
                h = h * keeps[i].to(h.dtype) / (1.0 - p)
    return h


def _redraw_gcn_bias(model):
    def redraw(stage, name, cols):
        b = getattr(model.gcn_blocks, name).bias
        b.data[cols] = 0.1 * torch.randn(len(cols))
    return redraw


def _gcn_model(shape, p):
    from graphneuralnetwork_amd.gcn import GCN_Model
    model = GCN_Model(*shape, p).train()
    with torch.no_grad():
        for m in model.gcn_blocks:
            if hasattr(m, "bias"):
                m.bias.normal_(0.0, 0.1)
    return model


def _gcn_graph_a(n=320):
    """Graph (a) with a few duplicate entries and random signed fp32 values."""
    r, c = _fixture_edges(n)
    rng = np.random.default_rng(5)
    dup = rng.choice(r.size, 12, replace=False)
    r, c = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]])
    order = np.lexsort((c, r))
    return r[order], c[order], rng.standard_normal(r.size).astype(np.float32)


def _dense_a(r, c, val, n):
    A = torch.zeros(n, n, dtype=F64)
    A.index_put_((torch.from_numpy(np.asarray(r, np.int64)),
                  torch.from_numpy(np.asarray(c, np.int64))),
                 torch.from_numpy(np.asarray(val, np.float64)), accumulate=True)
    return A


def _gcn_oracle(model, r, c, val, n, X, layers):
    rowptr, col = _csr(np.asarray(r, np.int64), np.asarray(c, np.int64), n)
    ws = [_np(getattr(model.gcn_blocks, f"gcn{i}").dense.weight) for i in range(layers)]
    bs = [_np(getattr(model.gcn_blocks, f"gcn{i}").bias) for i in range(layers)]
    return O.gcn_model(rowptr, col, val, X.numpy(), ws, bs)


GCN_SHAPES = [(128, 128, 7, 2), (64, 128, 7, 3), (100, 16, 3, 2)]


@pytest.mark.parametrize("x_grad", [True, False], ids=["dX", "no_dX"])
@pytest.mark.parametrize("graph", ["a", "b_ordered"])
@pytest.mark.parametrize("shape", GCN_SHAPES, ids=["x".join(map(str, s)) for s in GCN_SHAPES])
def test_gcn_model_step_vs_float64(dev, shape, graph, x_grad, monkeypatch):
    """GCN_Model, dropout 0: graph (a) with signed values and duplicates (transposed CSR in the
    backward), graph (b) under the gcn_adjacency normalisation with training over P A P^T forced
    (X permuted on entry, or -- X without gradient -- read through P A, GCN_FIRST_ROWS; the logits
    permuted back on exit). 100 -> 16 -> 3 is covered by no MFMA transform."""
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    fin, hid, ncls, layers = shape
    n = 320
    torch.manual_seed(4000 + fin + layers)
    model = _gcn_model(shape, 0.0)
    X = torch.randn(n, fin)
    labels = torch.randint(0, ncls, (n,))
    if graph == "a":
        r, c, val = _gcn_graph_a(n)
        g = _graph(dev, r, c, n, val=val)
    else:
        monkeypatch.setattr(ops, "XCD_MIN_NNZ", 0)
        monkeypatch.setattr(ops, "HUB_MIN_X_BYTES", 0)
        s, d = _fixture_edges(n)
        g = gcn_adjacency(torch.from_numpy(s), torch.from_numpy(d), n, device=dev)
        assert g.symmetric
        rp = g.rowptr.cpu().numpy()
        r, c, val = np.repeat(np.arange(n), np.diff(rp)), g.col.cpu().numpy(), g.val.cpu().numpy()
    A = _dense_a(r, c, val, n)

    def kinks():
        rec = []
        _ref_gcn(_params(model), X.double(), A, layers, rec=rec)
        return rec
    _settle(kinks, _redraw_gcn_bias(model))
    _assert_kinks(kinks(), f"GCN {shape} {graph}")
    P, X64 = _params(model), X.double().requires_grad_(x_grad)
    ref = _ce_step(lambda q: _ref_gcn(q, X64, A, layers), P, {"X": X64} if x_grad else {}, labels)
    np.testing.assert_allclose(_np(ref["logits"]), _gcn_oracle(model, r, c, val, n, X, layers),
                               rtol=1e-9, atol=1e-9)
    model.to(dev)
    Xg = X.to(dev).requires_grad_(x_grad)
    y = model(Xg, g)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    assert (("_nodeorder",) in g._plans) == (graph == "b_ordered")
    if graph == "b_ordered":
        assert (("_nodeorder_rows",) in g._plans) == (not x_grad and fin <= hid)
    got = {"logits": y, "loss": loss, **_param_grads(model)}
    if x_grad:
        got["grad:X"] = Xg.grad
    _compare(f"GCN {shape} {graph}", got, ref)


@pytest.mark.parametrize("x_grad", [True, False], ids=["dX", "no_dX"])
@pytest.mark.parametrize("shape", GCN_SHAPES[:2],
                         ids=["x".join(map(str, s)) for s in GCN_SHAPES[:2]])
def test_gcn_model_dropout_step_vs_float64(dev, shape, x_grad, monkeypatch):
    """p = 0.5 on the shapes whose Graph_conv_layer -> ReLU -> Dropout triples run as one op
    (ops.fuses_relu_dropout): one seed per hidden layer, the float64 step under the oracle's
    (seed, row, column) keep mask of that layer's output times 1 / (1 - p)."""
    from graphneuralnetwork_amd import gcn as gcn_mod
    from graphneuralnetwork_amd import ops
    fin, hid, ncls, layers = shape
    n, p = 320, 0.5
    torch.manual_seed(4500 + fin)
    model = _gcn_model(shape, p)
    X = torch.randn(n, fin)
    labels = torch.randint(0, ncls, (n,))
    r, c, val = _gcn_graph_a(n)
    A = _dense_a(r, c, val, n)
    step_seed = 987
    torch.manual_seed(step_seed)
    want = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(layers - 1)]
    keeps = [_elem_keep(s, n, hid, p) for s in want]

    def kinks():
        rec = []
        _ref_gcn(_params(model), X.double(), A, layers, keeps, p, rec)
        return rec
    torch.manual_seed(4501)
    _settle(kinks, _redraw_gcn_bias(model))
    _assert_kinks(kinks(), f"GCN dropout {shape}")
    P, X64 = _params(model), X.double().requires_grad_(x_grad)
    ref = _ce_step(lambda q: _ref_gcn(q, X64, A, layers, keeps, p), P,
                   {"X": X64} if x_grad else {}, labels)
    with torch.no_grad():
        np.testing.assert_allclose(_np(_ref_gcn(_params(model), X.double(), A, layers)),
                                   _gcn_oracle(model, r, c, val, n, X, layers),
                                   rtol=1e-9, atol=1e-9)
    g = _graph(dev, r, c, n, val=val)
    model.to(dev)
    for i in range(layers - 1):
        w = getattr(model.gcn_blocks, f"gcn{i}").dense.weight
        assert ops.fuses_relu_dropout(torch.empty(n, w.shape[1], device=dev), w, g)
    drawn = []
    real = gcn_mod.dropout_seed
    monkeypatch.setattr(gcn_mod, "dropout_seed", lambda: drawn.append(real()) or drawn[-1])
    Xg = X.to(dev).requires_grad_(x_grad)
    torch.manual_seed(step_seed)
    y = model(Xg, g)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    assert drawn == want
    got = {"logits": y, "loss": loss, **_param_grads(model)}
    if x_grad:
        got["grad:X"] = Xg.grad
    _compare(f"GCN dropout {shape}", got, ref)


def test_spmm_layer_step_vs_float64(dev):
    """ops.spmm (_SpmmFn) under a hand-composed layer spmm(A, X W^T, b) on graph (a) with signed
    values: output, dX (A^T over the transposed CSR), dW through torch's mm, db."""
    from graphneuralnetwork_amd import ops
    n = 320
    torch.manual_seed(4900)
    r, c, val = _gcn_graph_a(n)
    A = _dense_a(r, c, val, n)
    X, W, b, R = torch.randn(n, 40), 0.2 * torch.randn(24, 40), torch.randn(24), torch.randn(n, 24)
    t64 = [t.double().requires_grad_() for t in (X, W, b)]
    y64 = A @ (t64[0] @ t64[1].t()) + t64[2]
    (y64 * R.double()).sum().backward()
    g = _graph(dev, r, c, n, val=val)
    tg = [t.to(dev).requires_grad_() for t in (X, W, b)]
    y = ops.spmm(g, tg[0] @ tg[1].t(), tg[2])
    assert type(y.grad_fn).__name__ == "_SpmmFnBackward"
    (y * R.to(dev)).sum().backward()
    close(y, y64, what="spmm y")
    for name, a, ref in zip(("dX", "dW", "db"), tg, t64):
        close(a.grad, ref.grad, what=f"spmm {name}")


# ------------------------------------------------------------------ GraphSAGE
def _first_argmax(x):
    """torch.argmax over dim 1 with the first-maximum rule spelled out."""
    k = x.shape[1]
    idx = torch.arange(k).view(1, k, 1).expand_as(x)
    first = torch.where(x == x.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, k))
    return first.min(dim=1).values


def _max_gap(nf, layer):
    """Per feature, the smallest gap between the two largest of the k candidates; a set of
    post-ReLU candidates that are all exact zeros is locally constant (module docstring)."""
    s = nf.detach().sort(dim=1, descending=True).values
    gap = s[:, 0] - s[:, 1]
    if layer > 0:
        gap = torch.where(s[:, 0] == 0, torch.full_like(gap, float("inf")), gap)
    return gap.min(0).values, float(nf.detach().abs().max())


def _ref_sage(P, cf, cmaps, nf, nmaps, nlayers, agg, gcn, rec=None, tag=""):
    """GraphSAGE.forward, one branch (GraphSAGE/GraphSAGE.py:42-57, graph_utils.py:4-11)."""
    feats = None
    for i in range(nlayers):
        if agg != "MEAN" and rec is not None:
            rec.append((2 * i, f"max{i}{tag}", *_max_gap(nf, i)))
        if agg == "MEAN":
            a = nf.mean(dim=1)
        elif agg == "MAX":
            a = _first_argmax(nf).to(cf.dtype)
        else:
            a = torch.max(nf, dim=1).values
        comb = a if gcn else torch.cat([cf, a], dim=1)
        pre = comb @ P[f"sage_blocks.sage_layer{i}.weight.weight"].t()
        if rec is not None:
            d = pre.detach().abs()
            rec.append((2 * i + 1, f"relu{i}{tag}", d.min(0).values, float(d.max())))
        feats = torch.relu(pre)
        if i != nlayers - 1:
            cm, nm = cmaps[i], nmaps[i]
            cf = feats[cm[cm != -1]]
            nf = feats[nm[nm[:, 0] != -1, :]]
    return feats


def _sage_batch(rng, seeds, table_n, k_outer, k_inner, gcn):
    """Two-layer index maps as get_layer_adj_nodes lays them out (GraphSAGE/data_utils.py:82-124):
    global ids for the outer layer, positions in the outer layer's node list for the seeds, -1
    padded to the outer layer's length; gcn mode appends the node itself to its sample.
    Neighbours are distinct within a row (a repeated neighbour is an exact tie for max)."""
    ids = np.arange(table_n)
    inner = np.stack([rng.choice(ids[ids != s], k_inner, replace=False) for s in seeds])
    if gcn:
        inner = np.concatenate([inner, seeds[:, None]], axis=1)
    nodes = rng.permutation(np.unique(np.concatenate([seeds, inner.ravel()])))
    pos = np.full(table_n, -1)
    pos[nodes] = np.arange(nodes.size)
    outer = np.stack([rng.choice(ids[ids != v], k_outer, replace=False) for v in nodes])
    if gcn:
        outer = np.concatenate([outer, nodes[:, None]], axis=1)
    cm = np.full(nodes.size, -1, np.int64)
    cm[:seeds.size] = pos[seeds]
    nm = np.full((nodes.size, inner.shape[1]), -1, np.int64)
    nm[:seeds.size] = pos[inner]
    assert (cm == -1).any() and (nm[:, 0] == -1).any()
    return tuple(torch.from_numpy(a.astype(np.int64)) for a in (nodes, outer, cm, nm))


SAGE_CASES = [(64, 128, False, "MEAN", False), (64, 128, False, "MAX", False),
              (64, 128, False, "MAXPOOL", False), (64, 128, True, "MEAN", False),
              (64, 128, True, "MAXPOOL", False), (64, 128, False, "MEAN", True),
              (36, 24, False, "MEAN", False)]


@pytest.mark.parametrize("feed", ["pregathered", "gathered"])
@pytest.mark.parametrize("case", SAGE_CASES,
                         ids=[f"{a}-{b}-{'gcn' if g else 'cat'}-{f}-{'unsup' if u else 'sup'}"
                              for a, b, g, f, u in SAGE_CASES])
def test_graphsage_step_vs_float64(dev, case, feed):
    """GraphSAGE.forward, two layers, 40 seeds with fan-outs (5, 3) over a 300-row table, -1
    padded hop maps: fed as pre-gathered tensors that take gradients (_MeanAgg / _MaxPoolAgg in
    layer 0) and as Gathered(table, index) with the table taking one (_GatherRows,
    _GatherMeanAgg / _GatherMaxPoolAgg); layer 1 always gathers from layer 0's output. Supervised:
    cross-entropy on the classifier's logits; unsupervised: the bmm scores of the context /
    negative branch times a fixed random tensor. 36 -> 24 is outside the vector path."""
    from graphneuralnetwork_amd.graphsage import Gathered, GraphSAGE
    fin, fout, gcn, agg, unsup = case
    nt, B, S = 300, 40, 3
    torch.manual_seed(5000 + fin + len(agg) + 2 * gcn + unsup)
    rng = np.random.default_rng(50 + fin + len(agg) + 2 * gcn + unsup)
    model = GraphSAGE(2, fin, fout, gcn, agg, Unsupervised=unsup,
                      class_size=None if unsup else 5).train()
    table = torch.randn(nt, fin)
    branches = [_sage_batch(rng, rng.choice(nt, B, replace=False), nt, 5, 3, gcn)]
    if unsup:
        branches.append(_sage_batch(rng, rng.integers(0, nt, B * S), nt, 5, 3, gcn))
    labels = torch.randint(0, 5, (B,))
    R = torch.randn(B, 1, S)

    def run(P, tb, rec=None, leaves=None):
        outs = []
        for j, (nodes, outer, cm, nm) in enumerate(branches):
            cf, nf = tb[nodes], tb[outer]
            if leaves is not None:
                cf.retain_grad()
                nf.retain_grad()
                leaves += [cf, nf]
            outs.append(_ref_sage(P, cf, [cm], nf, [nm], 2, agg, gcn, rec, f"/{j}"))
        if not unsup:
            return outs[0], outs[0] @ P["dense.weight"].t() + P["dense.bias"]
        ctx = outs[1].reshape(B, S, -1)
        return outs[0], torch.bmm(outs[0].unsqueeze(1), ctx.permute(0, 2, 1))

    def kinks():
        rec = []
        run(_params(model), table.double(), rec)
        return rec

    def redraw(stage, name, cols):
        if stage == 0:   # layer 0's max over the table's rows
            table[:, cols] = torch.randn(nt, len(cols))
            return
        # stage 1 / 2: layer 0's ReLU / layer 1's max over its output; stage 3: layer 1's ReLU
        w = model.sage_blocks[0 if stage < 3 else 1].weight.weight
        bound = 1.0 / w.shape[1] ** 0.5
        w.data[cols] = (2 * torch.rand(len(cols), w.shape[1]) - 1) * bound
    _settle(kinks, redraw)
    _assert_kinks(kinks(), f"GraphSAGE {case}")

    def loss_of(feats, second, lab, rr):
        return F.cross_entropy(second, lab) if not unsup else (second * rr).sum()

    P, t64, leaves = _params(model), table.double().requires_grad_(), []
    f64_, s64 = run(P, t64, leaves=leaves)
    l64 = loss_of(f64_, s64, labels, R.double())
    l64.backward()
    ref = {"feats": f64_, "logits": s64, "loss": l64, **_ref_grads(P)}
    # the numpy oracle's forward, branch by branch
    ws = [_np(b.weight.weight) for b in model.sage_blocks]
    dense = None if unsup else (_np(model.dense.weight), _np(model.dense.bias))
    of = []
    for nodes, outer, cm, nm in branches:
        fo, cl = O.graphsage_forward(table.numpy()[nodes.numpy()], [cm.numpy()],
                                     table.numpy()[outer.numpy()], [nm.numpy()], ws, agg, gcn,
                                     dense)
        of.append((fo, cl))
    np.testing.assert_allclose(_np(f64_), of[0][0], rtol=1e-9, atol=1e-9)
    if unsup:
        want = np.einsum("bf,bsf->bs", of[0][0], of[1][0].reshape(B, S, -1))[:, None, :]
        np.testing.assert_allclose(_np(s64), want, rtol=1e-9, atol=1e-9)
    else:
        np.testing.assert_allclose(_np(s64), of[0][1], rtol=1e-9, atol=1e-9)

    model.to(dev)
    tg = table.to(dev)
    args, leaf_g = [], []
    if feed == "gathered":
        tg.requires_grad_()
        for nodes, outer, cm, nm in branches:
            args.append((Gathered(tg, nodes.to(dev)), [cm.to(dev)], Gathered(tg, outer.to(dev)),
                         [nm.to(dev)]))
        ref["grad:table"] = t64.grad
    else:
        for j, (nodes, outer, cm, nm) in enumerate(branches):
            cf = tg[nodes.to(dev)].clone().requires_grad_()
            nf = tg[outer.to(dev)].clone().requires_grad_()
            leaf_g += [cf, nf]
            args.append((cf, [cm.to(dev)], nf, [nm.to(dev)]))
            ref[f"grad:center{j}"] = leaves[2 * j].grad
            ref[f"grad:neigh{j}"] = leaves[2 * j + 1].grad
    if unsup:
        feats, second = model(*args[0], *args[1], (B, S))
    else:
        feats, second = model(*args[0], None, None, None, None, None)
    loss = loss_of(feats, second, labels.to(dev), R.to(dev))
    loss.backward()
    got = {"feats": feats, "logits": second, "loss": loss, **_param_grads(model)}
    if feed == "gathered":
        got["grad:table"] = tg.grad
    else:
        for j in range(len(branches)):
            got[f"grad:center{j}"] = leaf_g[2 * j].grad
            got[f"grad:neigh{j}"] = leaf_g[2 * j + 1].grad
    _compare(f"GraphSAGE {case} {feed}", got, ref)


# ------------------------------------------------------------------ GraphSAGE_Pytorch
def _ref_sage_gcn(src, nb, weight, agg_weight, neigh, hidden):
    a = nb.mean(dim=1) if neigh == "mean" else nb.sum(dim=1)
    sh, nh = src @ weight, a @ agg_weight
    return sh + nh if hidden == "sum" else torch.cat([sh, nh], dim=1)


def _ref_sagepy(P, feats, nbrs, rec=None):
    """GraphSage.forward (GraphSAGE_Pytorch/models/GraphSage.py:20-31, SageGCN.py:24-37)."""
    hidden, L = feats, len(nbrs)
    for l in range(L):
        nxt = []
        for hop in range(L - l):
            src = hidden[hop]
            nb = hidden[hop + 1].view(len(src), nbrs[hop], -1)
            pre = _ref_sage_gcn(src, nb, P[f"gcn.{l}.weight"], P[f"gcn.{l}.aggregator.weight"],
                                "mean", "sum")
            if l < L - 1:
                if rec is not None:
                    d = pre.detach().abs()
                    rec.append((l, f"gcn.{l}/hop{hop}", d.min(0).values, float(d.max())))
                pre = torch.relu(pre)
            nxt.append(pre)
        hidden = nxt
    return hidden[0]


def _redraw_cols(*weights):
    def go(cols):
        for w in weights:
            bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
            w.data[:, cols] = (2 * torch.rand(w.shape[0], len(cols)) - 1) * bound
    return go


@pytest.mark.parametrize("feed", ["pregathered", "gathered"])
def test_graphsage_pytorch_step_vs_float64(dev, feed):
    """GraphSage(24, [16, 3], [6, 4]) over 30 source nodes of a 300-row table, hops as
    Gathered(table, ids) and as pre-gathered table[ids]: every parameter and the table."""
    from graphneuralnetwork_amd.graphsage import Gathered
    from graphneuralnetwork_amd.graphsage_pytorch import GraphSage
    nt, B, nbrs = 300, 30, [6, 4]
    torch.manual_seed(6000)
    rng = np.random.default_rng(60)
    hops = [torch.from_numpy(rng.choice(nt, B, replace=False))]
    for k in nbrs:
        hops.append(torch.from_numpy(rng.integers(0, nt, hops[-1].numel() * k)))
    model = GraphSage(24, [16, 3], nbrs).train()
    table = torch.randn(nt, 24)
    labels = torch.randint(0, 3, (B,))

    def kinks():
        rec = []
        _ref_sagepy(_params(model), [table.double()[h] for h in hops], nbrs, rec)
        return rec
    _settle(kinks, lambda stage, name, cols: _redraw_cols(model.gcn[stage].weight,
                                                         model.gcn[stage].aggregator.weight)(cols))
    _assert_kinks(kinks(), "GraphSage")
    P, t64 = _params(model), table.double().requires_grad_()
    ref = _ce_step(lambda q: _ref_sagepy(q, [t64[h] for h in hops], nbrs), P, {"table": t64},
                   labels)
    layers = [(_np(m.weight), _np(m.aggregator.weight)) for m in model.gcn]
    np.testing.assert_allclose(_np(ref["logits"]),
                               O.graphsage_tree([table.numpy()[h.numpy()] for h in hops], layers,
                                                nbrs),
                               rtol=1e-9, atol=1e-9)
    model.to(dev)
    tg = table.to(dev).requires_grad_()
    feats = [Gathered(tg, h.to(dev)) if feed == "gathered" else tg[h.to(dev)] for h in hops]
    y = model(feats)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    got = {"logits": y, "loss": loss, "grad:table": tg.grad, **_param_grads(model)}
    _compare(f"GraphSage {feed}", got, ref)


@pytest.mark.parametrize("hidden", ["sum", "concat"])
@pytest.mark.parametrize("neigh", ["mean", "sum", "max"])
def test_sage_gcn_step_vs_float64(dev, neigh, hidden):
    """One SageGCN(24, 16) per aggr_neighbor_method / aggr_hidden_method the class accepts; 'max'
    is accepted by the constructor and fails in forward exactly as the reference's does
    (Tensor.max(dim=1) is a (values, indices) pair: TypeError from matmul)."""
    from graphneuralnetwork_amd.graphsage_pytorch import SageGCN
    B, k, fin, hid = 50, 6, 24, 16
    torch.manual_seed(6100 + len(neigh) + len(hidden))
    layer = SageGCN(fin, hid, aggr_neighbor_method=neigh, aggr_hidden_method=hidden).train()
    src, nb = torch.randn(B, fin), torch.randn(B, k, fin)
    if neigh == "max":
        with pytest.raises(TypeError):
            layer.to(dev)(src.to(dev).requires_grad_(), nb.to(dev).requires_grad_())
        return
    width = hid if hidden == "sum" else 2 * hid
    labels = torch.randint(0, width, (B,))

    def pre(P, s, b):
        return _ref_sage_gcn(s, b, P["weight"], P["aggregator.weight"], neigh, hidden)

    def kinks():
        d = pre(_params(layer), src.double(), nb.double()).detach().abs()
        return [(0, "relu", d.min(0).values, float(d.max()))]

    def redraw(stage, name, cols):
        for cc in cols:
            ws = (layer.weight, layer.aggregator.weight) if hidden == "sum" else \
                ((layer.weight,) if cc < hid else (layer.aggregator.weight,))
            _redraw_cols(*ws)([cc % hid])
    _settle(kinks, redraw)
    _assert_kinks(kinks(), f"SageGCN {neigh} {hidden}")
    P, s64, b64 = _params(layer), src.double().requires_grad_(), nb.double().requires_grad_()
    ref = _ce_step(lambda q: torch.relu(pre(q, s64, b64)), P, {"src": s64, "neigh": b64}, labels)
    np.testing.assert_allclose(_np(ref["logits"]),
                               O.sage_gcn(src.numpy(), nb.numpy(), _np(layer.weight),
                                          _np(layer.aggregator.weight), None, neigh, hidden),
                               rtol=1e-9, atol=1e-9)
    layer.to(dev)
    sg, bg = src.to(dev).requires_grad_(), nb.to(dev).requires_grad_()
    y = layer(sg, bg)
    loss = F.cross_entropy(y, labels.to(dev))
    loss.backward()
    got = {"logits": y, "loss": loss, "grad:src": sg.grad, "grad:neigh": bg.grad,
           **_param_grads(layer)}
    _compare(f"SageGCN {neigh} {hidden}", got, ref)
