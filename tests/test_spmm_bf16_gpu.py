"""GCN aggregation over bf16-stored feature rows (gnn_spmm_csr_bf16 and its hub / tasks forms).

A bf16 value widens to fp32 exactly and all arithmetic after the load is the fp32 kernel's, so
the float64 oracle is fed the bf16-rounded inputs upcast to fp32 and the fp32 tolerance of
tests/test_spmm_gpu.py applies unchanged: rtol 1e-4, atol 1e-5 * max|y|; regrouped sums are
compared with each other at rtol 1e-5.
"""
import numpy as np
import pytest
import torch

from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def close(a, b, rtol=RTOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale)


def _graph(rowptr, col, val, n_cols, dev):
    from graphneuralnetwork_amd.graph import CsrGraph
    return CsrGraph(torch.as_tensor(rowptr, dtype=torch.int64, device=dev),
                    torch.as_tensor(col, dtype=torch.int32, device=dev),
                    torch.as_tensor(val, dtype=torch.float32, device=dev),
                    len(rowptr) - 1, n_cols)


def _rand_graph(n, e, seed, hub_deg=0, n_cols=None):
    rng = np.random.default_rng(seed)
    n_cols = n if n_cols is None else n_cols
    src = rng.integers(0, n, e)
    dst = rng.integers(0, n_cols, e)
    if hub_deg:
        src = np.concatenate([src, np.full(hub_deg, 3), np.full(hub_deg // 2, n - 1)])
        dst = np.concatenate([dst, rng.integers(0, n_cols, hub_deg + hub_deg // 2)])
    val = rng.standard_normal(src.size).astype(np.float32)
    return O.coo_to_csr(src, dst, val, n)


def _bf16(x: np.ndarray, dev):
    """(device bf16 tensor, the same values as a host fp32 array)."""
    t = torch.from_numpy(x).to(dev).bfloat16()
    return t, t.float().cpu().numpy()


# 2056: one 8-column lane past the 2048-column block of the vector layout (64 lanes x 4 chunks
# x 8 bf16); 515: past the 512-column block of the one-element-per-lane path
@pytest.mark.parametrize("F", [1, 3, 7, 8, 16, 24, 33, 64, 96, 128, 256, 264, 520, 1000, 515,
                               2056])
def test_feature_widths(dev, F):
    """Scalar path (odd widths), every lanes-per-row case, multi-chunk rows, the block split."""
    from graphneuralnetwork_amd.ops import spmm_forward
    n = 700 if F < 1000 else 300
    rowptr, col, val = _rand_graph(n, 9 * n, F, hub_deg=700)
    rng = np.random.default_rng(F)
    Xd, X = _bf16(rng.standard_normal((n, F)).astype(np.float32), dev)
    b = rng.standard_normal(F).astype(np.float32)
    g = _graph(rowptr, col, val, n, dev)
    Y = spmm_forward(g, Xd, torch.from_numpy(b).to(dev))
    assert Y.dtype == torch.float32
    close(Y.cpu().numpy(), O.spmm_csr(rowptr, col, val, X, b))


@pytest.mark.parametrize("seg_len", [1, 2, 7, 64, 1000])
def test_long_row_split(dev, seg_len):
    from graphneuralnetwork_amd.ops import spmm_forward
    n, F = 500, 128
    rowptr, col, val = _rand_graph(n, 20 * n, 11, hub_deg=3000)
    Xd, X = _bf16(np.random.default_rng(1).standard_normal((n, F)).astype(np.float32), dev)
    g = _graph(rowptr, col, val, n, dev)
    Y = spmm_forward(g, Xd, seg_len=seg_len).cpu().numpy()
    close(Y, O.spmm_csr(rowptr, col, val, X))


def _class_graph(n, seed):
    """~40 % one-edge rows, ~10 % edgeless rows, the rest 2..40 edges, two long rows."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    deg = np.where(u < 0.1, 0, np.where(u < 0.5, 1, rng.integers(2, 40, n)))
    deg[5], deg[n - 2] = 900, 400
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)
    val = rng.standard_normal(rowptr[-1]).astype(np.float32)
    return rowptr, col, val, deg


@pytest.mark.parametrize("tasks", [False, True])
@pytest.mark.parametrize("F", [24, 128])
def test_row_classes_and_epilogues(dev, F, tasks, monkeypatch):
    from graphneuralnetwork_amd import ops
    monkeypatch.setattr(ops, "SPMM_TASKS", tasks)
    n = 1200
    rowptr, col, val, deg = _class_graph(n, 7 + F)
    g = _graph(rowptr, col, val, n, dev)
    rng = np.random.default_rng(F)
    Xd, X = _bf16(rng.standard_normal((n, F)).astype(np.float32), dev)
    b = rng.standard_normal(F).astype(np.float32)
    bd = torch.from_numpy(b).to(dev)
    ref = O.spmm_csr(rowptr, col, val, X, b)
    want = {None: ref, "relu": np.maximum(ref, 0),
            "elu": np.where(ref > 0, ref, np.expm1(np.minimum(ref, 0)))}
    for act in (None, "relu", "elu"):
        y = ops.spmm_forward(g, Xd, bd, activation=act, seg_len=128)
        close(y.cpu().numpy(), want[act])
    base = rng.standard_normal((n, F)).astype(np.float32)
    out = torch.from_numpy(base).to(dev)
    ops.spmm_forward(g, Xd, None, out=out, accumulate=True, seg_len=128)
    got = out.cpu().numpy()
    close(got, base + O.spmm_csr(rowptr, col, val, X))
    np.testing.assert_array_equal(got[deg == 0], base[deg == 0])  # rows without edges keep out
    out = torch.from_numpy(base).to(dev)
    ops.spmm_forward(g, Xd, bd, out=out, accumulate=True, seg_len=128)
    close(out.cpu().numpy(), base + ref)


@pytest.mark.parametrize("F", [3, 128, 264])
def test_hub_staging_bitexact(dev, F):
    """Staging hub rows into a compact bf16 table (gnn_gather_rows_bf16) changes no bit; on a
    column-degree-ordered graph the hub rows are read in place: the natural-order result."""
    from graphneuralnetwork_amd.graph import degree_order
    from graphneuralnetwork_amd.ops import spmm_forward
    n = 900
    rowptr, col, val = _rand_graph(n, 12 * n, 40 + F, hub_deg=4000)
    g = _graph(rowptr, col, val, n, dev)
    X = torch.randn(n, F, device=dev).bfloat16()
    b = torch.randn(F, device=dev)
    base = torch.randn(n, F, device=dev)
    o = degree_order(g, rows=False)
    Xp = o.permute_rows(X.float()).bfloat16()  # a permutation of bf16 values: exact
    for seg_len in (None, 16):
        ref = spmm_forward(g, X, b, activation="relu", seg_len=seg_len, hubs=0)
        acc_ref = spmm_forward(g, X, None, out=base.clone(), accumulate=True, seg_len=seg_len,
                               hubs=0)
        for k in (1, 17, 300, n):
            y = spmm_forward(g, X, b, activation="relu", seg_len=seg_len, hubs=k)
            assert torch.equal(y, ref), (F, seg_len, k)
            y = spmm_forward(g, X, None, out=base.clone(), accumulate=True, seg_len=seg_len,
                             hubs=k)
            assert torch.equal(y, acc_ref), (F, seg_len, k, "accumulate")
            y = spmm_forward(o.graph, Xp, b, activation="relu", seg_len=seg_len, hubs=k)
            assert o.graph.hub_plan(k).prefix
            assert torch.equal(y, ref), (F, seg_len, k, "in place")
    close(ref.cpu().numpy(), np.maximum(O.spmm_csr(rowptr, col, val, X.float().cpu().numpy(),
                                                   b.cpu().numpy()), 0))


@pytest.mark.parametrize("F", [8, 128])
def test_packed_tasks(dev, F, monkeypatch):
    from graphneuralnetwork_amd import ops
    rng = np.random.default_rng(F)
    n = 3000
    deg = rng.integers(0, 12, n)
    deg[rng.integers(0, n, 30)] = rng.integers(60, 700, 30)
    deg[100:190] = 0  # a run longer than one task
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)
    val = rng.standard_normal(rowptr[-1]).astype(np.float32)
    g = _graph(rowptr, col, val, n, dev)
    Xd, X = _bf16(rng.standard_normal((n, F)).astype(np.float32), dev)
    b = rng.standard_normal(F).astype(np.float32)
    bd = torch.from_numpy(b).to(dev)
    ref = O.spmm_csr(rowptr, col, val, X, b)
    monkeypatch.setattr(ops, "SPMM_TASKS", False)
    per_row = ops.spmm_forward(g, Xd, bd, seg_len=256, hubs=0)
    close(per_row.cpu().numpy(), ref)
    monkeypatch.setattr(ops, "SPMM_TASKS", True)
    for max_deg, cost in ((8, 16), (128, 256)):
        monkeypatch.setattr(ops, "TASK_MAX_DEG", max_deg)
        monkeypatch.setattr(ops, "TASK_COST", cost)
        monkeypatch.setattr(ops, "TASK_COST_NARROW", cost)
        for hubs in (0, 50):
            y = ops.spmm_forward(g, Xd, bd, seg_len=256, hubs=hubs)
            assert any(k[0] == "_tasks" for k in g._plans if isinstance(k, tuple))
            close(y.cpu().numpy(), ref)
            close(y.cpu().numpy(), per_row.cpu().numpy(), rtol=1e-5)
    assert torch.equal(ops.spmm_forward(g, Xd, bd, seg_len=256),
                       ops.spmm_forward(g, Xd, bd, seg_len=256))  # deterministic


def _xcd_graph(n, seed):
    """tests/test_spmm_gpu.py's XCD corner graph: one-edge rows whose edge is a hub column,
    edgeless rows, rows whose every edge duplicates one hub column, two long rows."""
    rng = np.random.default_rng(seed)
    src = rng.integers(120, n, 16 * n)
    dst = rng.integers(0, n, 16 * n)
    hub = np.concatenate([np.full(5000, 3), np.full(2500, n - 1)])
    src = np.concatenate([src, hub, np.arange(100), np.repeat(np.arange(110, 120), 8)])
    dst = np.concatenate([dst, rng.integers(0, n, hub.size), np.full(100, 7),
                          np.full(80, 11)])
    src = np.concatenate([src, rng.integers(120, n, 6000)])
    dst = np.concatenate([dst, np.repeat([7, 11], 3000)])
    val = rng.standard_normal(src.size).astype(np.float32)
    return O.coo_to_csr(src, dst, val, n)


@pytest.mark.parametrize("tasks", [False, True])
@pytest.mark.parametrize("F", [64, 128, 600])
def test_xcd_direct(dev, F, tasks, monkeypatch):
    """The XCD-sliced direct form over a degree-ordered graph (pass 1: bf16 X -> fp32 partial
    rows; pass 2: bf16 X and the fp32 partial rows through xh), and the documented fallback on
    a natural-order graph."""
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.graph import degree_order
    from graphneuralnetwork_amd.ops import spmm_forward
    monkeypatch.setattr(ops, "XCD_MIN_DEG", 4)
    monkeypatch.setattr(ops, "XCD_CHUNK", 8)
    monkeypatch.setattr(ops, "SPMM_TASKS", tasks)
    n = 1500
    rowptr, col, val = _xcd_graph(n, 90 + F)
    g = _graph(rowptr, col, val, n, dev)
    o = degree_order(g, rows=False)
    X = torch.randn(n, F, device=dev).bfloat16()
    Xp = o.permute_rows(X.float()).bfloat16()
    b = torch.randn(F, device=dev)
    want = O.spmm_csr(rowptr, col, val, X.float().cpu().numpy(), b.cpu().numpy())
    for seg_len in (None, 16):
        for k in (200, n):
            y = spmm_forward(o.graph, Xp, b, seg_len=seg_len, hubs=k, xcd=True)
            key = ("_xcd", k, 4, min(8, seg_len or 10 ** 9), 1, None, None)
            assert o.graph._plans[key].prefix  # the XCD plan was built and is in place
            close(y.cpu().numpy(), want)
            assert torch.equal(y, spmm_forward(o.graph, Xp, b, seg_len=seg_len, hubs=k, xcd=True))
            y0 = spmm_forward(o.graph, Xp, b, seg_len=seg_len, hubs=0, xcd=False)
            close(y.cpu().numpy(), y0.cpu().numpy(), rtol=1e-5)
            # natural order: no in-place hub rows, so xcd=True takes the hub-staged path
            nat = spmm_forward(g, X, b, seg_len=seg_len, hubs=k, xcd=True)
            assert torch.equal(nat, spmm_forward(g, X, b, seg_len=seg_len, hubs=k, xcd=False))
            assert not any(isinstance(q, tuple) and q[0] == "_xcd" for q in g._plans)


@pytest.mark.parametrize("F", [8, 126, 128])
def test_views(dev, F):
    """A [:, 1:F+1] slice of a wider bf16 tensor (2-byte-misaligned, odd pitch) and a
    non-contiguous column stride."""
    from graphneuralnetwork_amd.ops import spmm_forward
    n = 600
    rowptr, col, val = _rand_graph(n, 10 * n, 3 + F, hub_deg=900)
    g = _graph(rowptr, col, val, n, dev)
    Xw = torch.randn(n, F + 5, device=dev).bfloat16()
    b = torch.randn(F, device=dev)
    Xs = Xw[:, 1:F + 1]
    assert Xs.data_ptr() % 4 == 2 and Xs.stride(0) % 2 == 1
    for hubs in (0, 40):
        y = spmm_forward(g, Xs, b, hubs=hubs)
        close(y.cpu().numpy(), O.spmm_csr(rowptr, col, val, Xs.float().cpu().numpy(),
                                          b.cpu().numpy()))
    X2 = torch.randn(n, 2 * F, device=dev).bfloat16()[:, ::2]
    assert X2.stride(1) == 2
    y = spmm_forward(g, X2, b)
    close(y.cpu().numpy(), O.spmm_csr(rowptr, col, val, X2.float().cpu().numpy(),
                                      b.cpu().numpy()))


@pytest.mark.parametrize("F", [33, 128])
def test_relation_to_fp32(dev, F):
    from graphneuralnetwork_amd.ops import spmm_forward
    n = 800
    rowptr, col, val = _rand_graph(n, 12 * n, 21, hub_deg=2000)
    g = _graph(rowptr, col, val, n, dev)
    X = torch.randn(n, F, device=dev).bfloat16()
    b = torch.randn(F, device=dev)
    close(spmm_forward(g, X, b).cpu().numpy(), spmm_forward(g, X.float(), b).cpu().numpy(),
          rtol=1e-5)


@pytest.mark.parametrize("tasks", [False, True])
@pytest.mark.parametrize("F", [5, 128])
def test_nonfinite(dev, F, tasks, monkeypatch):
    """NaN / +-inf rows of X reach exactly the outputs they reach in the fp32 kernel; one in a
    row no edge references reaches nothing."""
    from graphneuralnetwork_amd import ops
    monkeypatch.setattr(ops, "SPMM_TASKS", tasks)
    n = 600
    rng = np.random.default_rng(F)
    src = rng.integers(0, n, 8 * n)
    dst = rng.integers(0, n - 1, 8 * n)  # column n - 1 is referenced by no edge
    val = rng.random(src.size).astype(np.float32) + 0.5  # positive: inf stays inf
    rowptr, col, val = O.coo_to_csr(src, dst, val, n)
    g = _graph(rowptr, col, val, n, dev)
    X = torch.randn(n, F, device=dev)
    X[10, 0] = float("nan")
    X[20, F - 1] = float("inf")
    X[30, F // 2] = float("-inf")
    X[n - 1] = float("nan")
    X[n - 1, 0] = float("inf")
    Xb = X.bfloat16()
    y = ops.spmm_forward(g, Xb, hubs=0)
    y32 = ops.spmm_forward(g, Xb.float(), hubs=0)
    assert torch.equal(torch.isnan(y), torch.isnan(y32))
    inf = torch.isinf(y32)
    assert torch.equal(torch.isinf(y), inf) and torch.equal(y[inf], y32[inf])
    fin = torch.isfinite(y32)
    assert bool(torch.isnan(y32).any()) and bool(inf.any())
    close(y[fin].cpu().numpy(), y32[fin].cpu().numpy(), rtol=1e-5)
    # without the three poisoned rows every output is finite: row n - 1 reached nothing
    Xc = Xb.clone()
    Xc[[10, 20, 30]] = 0
    assert bool(torch.isfinite(ops.spmm_forward(g, Xc, hubs=0)).all())


def test_degenerate_shapes(dev):
    from graphneuralnetwork_amd.graph import CsrGraph
    from graphneuralnetwork_amd.ops import spmm_forward
    bf = torch.bfloat16

    def graph(rowptr, col, n_cols):
        return CsrGraph(torch.tensor(rowptr, dtype=torch.int64, device=dev),
                        torch.tensor(col, dtype=torch.int32, device=dev),
                        torch.ones(len(col), device=dev), len(rowptr) - 1, n_cols)

    y = spmm_forward(graph([0], [], 4), torch.randn(4, 16, device=dev).to(bf))
    assert y.shape == (0, 16) and y.dtype == torch.float32
    y = spmm_forward(graph([0, 1, 2], [0, 1], 3), torch.empty(3, 0, device=dev, dtype=bf))
    assert y.shape == (2, 0) and y.dtype == torch.float32
    b = torch.randn(16, device=dev)
    y = spmm_forward(graph([0, 0, 0, 0], [], 5), torch.randn(5, 16, device=dev).to(bf), b)
    assert torch.equal(y, b.expand(3, 16))
    y = spmm_forward(graph([0, 0, 0], [], 0), torch.empty(0, 16, device=dev, dtype=bf), b)
    assert torch.equal(y, b.expand(2, 16))


def test_errors(dev):
    from graphneuralnetwork_amd import ops
    n, F = 50, 16
    rowptr, col, val = _rand_graph(n, 4 * n, 2)
    g = _graph(rowptr, col, val, n, dev)
    X = torch.randn(n, F, device=dev)
    with pytest.raises(TypeError):
        ops.spmm_forward(g, X.half())
    with pytest.raises(ValueError):
        ops.spmm_forward(g, X.bfloat16(), out=torch.empty(n, F, device=dev, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="fp32"):
        ops.spmm(g, X.bfloat16().requires_grad_())
    # without grad, ops.spmm is the forward
    close(ops.spmm(g, X.bfloat16()).cpu().numpy(),
          O.spmm_csr(rowptr, col, val, X.bfloat16().float().cpu().numpy()))
