"""Graph_conv_layer / GCN_Model inference with a bf16 support tensor (ops.support_dtype).

Bound against the fp32 layer: S_bf16 = S (1 + d), |d| <= 2^-9 (round to nearest), so
|A S_bf16 - A S| <= 2^-9 |A| |S|; the fp32 accumulation of either side adds its own rounding,
absorbed by a factor two and the suite's absolute term: |y_bf16 - y_fp32| <= 2^-8 (|A| |S|) +
1e-4 max|y|.
"""
import numpy as np
import pytest
import torch

from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def close(a, b, rtol=1e-4):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale)


def _rand_graph(n, e, seed, hub_deg):
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, n, e), np.full(hub_deg, 3), np.full(hub_deg // 2, n - 1)])
    dst = rng.integers(0, n, src.size)
    val = rng.standard_normal(src.size).astype(np.float32)
    return O.coo_to_csr(src, dst, val, n)


def _graph(rowptr, col, val, n, dev):
    from graphneuralnetwork_amd.graph import CsrGraph
    return CsrGraph(torch.as_tensor(rowptr, dtype=torch.int64, device=dev),
                    torch.as_tensor(col, dtype=torch.int32, device=dev),
                    torch.as_tensor(val, dtype=torch.float32, device=dev), n, n)


def _abs_spmm(rowptr, col, val, S):
    return O.spmm_csr(rowptr, col, np.abs(val), np.abs(np.asarray(S, np.float64)))


def _within_bound(y16, y32, abs_as):
    y16, y32 = (np.asarray(t, np.float64) for t in (y16, y32))
    bound = 2.0 ** -8 * abs_as + 1e-4 * np.abs(y32).max()
    err = np.abs(y16 - y32)
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("big,xcd", [(True, True), (True, False), (False, False)])
def test_layer_bf16_support(dev, big, xcd, monkeypatch):
    """big: the column-degree order with the hub rows read in place (thresholds lowered as in
    test_gcn_layer_column_order) -- through the XCD-sliced direct form (ops.XCD_BF16 on) and
    through the hub-staged kernel (its default); else a small graph on the plain path."""
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.gcn import Graph_conv_layer
    monkeypatch.setattr(ops, "XCD_BF16", xcd)
    if big:
        monkeypatch.setattr(ops, "HUB_MIN_X_BYTES", 0)
        monkeypatch.setattr(ops, "XCD_MIN_NNZ", 1)
        monkeypatch.setattr(ops, "XCD_MIN_DEG", 4)
        n, e, hub = 2000, 30 * 2000, 6000
    else:
        n, e, hub = 300, 5 * 300, 200
    F = 128
    rowptr, col, val = _rand_graph(n, e, 5, hub)
    g = _graph(rowptr, col, val, n, dev)
    layer = Graph_conv_layer(64, F).to(dev)
    with torch.no_grad():
        layer.bias.normal_()
    X = torch.randn(n, 64, device=dev)
    W, b = layer.dense.weight.detach(), layer.bias.detach()
    with torch.no_grad():
        y32 = layer(X, g)
        S = ops.gcn_transform(X, W)
        with ops.support_dtype(BF16):
            y16 = layer(X, g)
            y16_relu = layer._forward(X, g, "relu")
        assert torch.equal(layer(X, g), y32)  # outside the context: the default
    assert y16.dtype == torch.float32
    S16 = S.to(BF16)
    order = g._plans.get(("_colorder",))
    assert (order is not None) == big
    if big:  # the composition: transform rows in the column order, SpMM over A P^T
        Sp = torch.empty_like(S16)
        Sp[order.inv] = S16
        want = ops.spmm_forward(order.graph, Sp, b, xcd=xcd)
        other = ops.spmm_forward(order.graph, Sp, b, xcd=not xcd)  # the other route: regrouped
        close(other.cpu().numpy(), want.cpu().numpy(), rtol=1e-5)
        assert order.graph.hub_plan(ops.hub_rows_for(n, F, 2)).prefix  # hub rows in place
    else:
        want = ops.spmm_forward(g, S16, b)
    assert torch.equal(y16, want)
    assert torch.equal(y16_relu, torch.relu(y16))
    close(y16.cpu().numpy(), O.spmm_csr(rowptr, col, val, S16.float().cpu().numpy(),
                                        b.cpu().numpy()))
    _within_bound(y16.cpu().numpy(), y32.cpu().numpy(), _abs_spmm(rowptr, col, val, S.cpu().numpy()))
    assert float((y16 - y32).abs().max()) > 0  # the bf16 path did run


def test_grad_enabled_stays_fp32(dev):
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.gcn import Graph_conv_layer
    n = 300
    rowptr, col, val = _rand_graph(n, 5 * n, 9, 200)
    g = _graph(rowptr, col, val, n, dev)
    layer = Graph_conv_layer(64, 128).to(dev)
    X = torch.randn(n, 64, device=dev)
    y32 = layer(X, g)
    with ops.support_dtype(BF16):
        y = layer(X, g)
        assert torch.equal(y, y32)
        y.square().sum().backward()
        # grad mode on but nothing requires grad: the inference path, still fp32
        frozen = Graph_conv_layer(64, 128).to(dev).requires_grad_(False)
        frozen.load_state_dict(layer.state_dict())
        y_frozen = frozen(X, g)
    assert torch.equal(y_frozen, frozen(X, g))
    with torch.no_grad(), ops.support_dtype(BF16):
        assert not torch.equal(frozen(X, g), y_frozen)  # without grad the same layer takes bf16
    assert layer.dense.weight.grad is not None and layer.bias.grad is not None
    assert bool(torch.isfinite(layer.dense.weight.grad).all())
    assert float(layer.dense.weight.grad.abs().max()) > 0


def test_context_nests_and_restores():
    from graphneuralnetwork_amd import ops
    assert ops.SUPPORT_DTYPE == torch.float32
    with ops.support_dtype(BF16):
        with ops.support_dtype(torch.float32):
            assert ops.SUPPORT_DTYPE == torch.float32
        assert ops.SUPPORT_DTYPE == BF16
        with pytest.raises(RuntimeError):
            with ops.support_dtype(BF16):
                raise RuntimeError("restored on an exception too")
        assert ops.SUPPORT_DTYPE == BF16
    assert ops.SUPPORT_DTYPE == torch.float32


def test_model_first_layer_bf16_classifier_fp32(dev):
    """GCN_Model(128, 128, 7): the 128 -> 128 layer takes the bf16 support, the 7-class layer
    (no MFMA transform for that shape) stays fp32."""
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.gcn import GCN_Model
    n = 600
    rowptr, col, val = _rand_graph(n, 6 * n, 13, 300)
    val = np.abs(val) / 8  # a normalised-adjacency-like operator: activations stay O(1)
    g = _graph(rowptr, col, val, n, dev)
    model = GCN_Model(128, 128, 7, 2, 0.5).to(dev).eval()
    X = torch.randn(n, 128, device=dev)
    l0, l1 = model.gcn_blocks.gcn0, model.gcn_blocks.gcn1
    with torch.no_grad():
        l0.bias.normal_()
        l1.bias.normal_()
        y32 = model(X, g)
        with ops.support_dtype(BF16):
            y16 = model(X, g)
            h16 = torch.relu(l0(X, g))
            assert ops.gcn_transform(h16, l1.dense.weight, out_dtype=BF16) is None
            assert torch.equal(y16, l1(h16, g))
        y0 = l0(X, g)
        h32 = torch.relu(y0)
        # the 7-class layer in fp32 on the bf16 path's hidden activations
        assert torch.equal(y16, l1(h16, g))
        S0 = ops.gcn_transform(X, l0.dense.weight)
    assert float((h16 - h32).abs().max()) > 0
    # first-layer bound on h (ReLU is 1-Lipschitz), pushed through |W1| and |A|
    A0 = _abs_spmm(rowptr, col, val, S0.cpu().numpy())
    dh = 2.0 ** -8 * A0 + 1e-4 * float(y0.abs().max())
    assert bool((np.abs((h16 - h32).cpu().numpy().astype(np.float64)) <= dh).all())
    W1 = np.abs(l1.dense.weight.detach().cpu().numpy().astype(np.float64))
    bound = O.spmm_csr(rowptr, col, np.abs(val), dh @ W1.T) + 1e-4 * float(y32.abs().max())
    err = np.abs((y16 - y32).cpu().numpy().astype(np.float64))
    assert (err <= bound).all(), float((err / bound).max())
