"""GTN without a GPU: the dense path and the sparse path (through the torch restatements of the
kernels) against the reference's golden run (tests/golden/gtn.npz, made by
tests/golden/make_gtn_golden.py), the edge-type graph builder against the dense stack, and the
restatements themselves against dense float64 numpy."""
from pathlib import Path

import numpy as np
import pytest
import torch

from graphneuralnetwork_amd import GTConv, GTLayer, GTN_Model, gtn, ops  # noqa: F401
from graphneuralnetwork_amd.graph import from_dense
from graphneuralnetwork_amd.hetero import EdgeTypeGraph, edge_type_graph

GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "gtn.npz")
LAYERS = (1, 2, 3)


def close(got, ref, what):
    """The project's training tolerance (tests/test_training_gpu.py)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    scale = max(float(np.abs(ref).max()), 1e-30)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5 * scale, err_msg=what)


def golden_model(L, w_out=8):
    model = GTN_Model(5, 2, 12, w_out, 3, L, True)
    keys = [str(k) for k in GOLDEN[f"L{L}_keys"]]
    state = {k: torch.from_numpy(GOLDEN[f"L{L}_param_{k}"]) for k in keys}
    assert list(model.state_dict()) == keys
    model.load_state_dict(state)
    return model


def golden_inputs():
    return (torch.from_numpy(GOLDEN["A"].astype(np.float32)), torch.from_numpy(GOLDEN["X"]),
            torch.from_numpy(GOLDEN["target_x"]), torch.from_numpy(GOLDEN["labels"]))


def check_against_golden(model, A, X, target, labels, L):
    y, Ws = model(A, X, target)
    torch.nn.functional.cross_entropy(y, labels).backward()
    close(y, GOLDEN[f"L{L}_y"], "y")
    assert len(Ws) == L and [len(W) for W in Ws] == [2] + [1] * (L - 1)
    for i, W in enumerate(Ws):
        for j, w in enumerate(W):
            assert not w.requires_grad
            close(w, GOLDEN[f"L{L}_W_{i}_{j}"], f"Ws[{i}][{j}]")
    grads = [k[len(f"L{L}_grad_"):] for k in GOLDEN.files if k.startswith(f"L{L}_grad_")]
    assert grads
    for name, p in model.named_parameters():
        if name in grads:
            close(p.grad, GOLDEN[f"L{L}_grad_{name}"], f"grad {name}")
        else:
            assert p.grad is None or not p.requires_grad, name


@pytest.mark.parametrize("L", LAYERS)
def test_dense_path_matches_reference(L):
    A, X, target, labels = golden_inputs()
    check_against_golden(golden_model(L), A, X, target, labels, L)


@pytest.mark.parametrize("L", LAYERS)
def test_sparse_path_on_cpu_matches_reference(L):
    A, X, target, labels = golden_inputs()
    check_against_golden(golden_model(L), edge_type_graph(A), X, target, labels, L)


def test_state_dict_keys_and_shapes():
    model = GTN_Model(5, 2, 12, 8, 3, 3, True)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes == {
        "weight": (12, 8), "bias": (8,),
        "layers.0.conv1.weight": (2, 5, 1, 1), "layers.0.conv1.scale": (1,),
        "layers.0.conv2.weight": (2, 5, 1, 1), "layers.0.conv2.scale": (1,),
        "layers.1.conv1.weight": (2, 5, 1, 1), "layers.1.conv1.scale": (1,),
        "layers.2.conv1.weight": (2, 5, 1, 1), "layers.2.conv1.scale": (1,),
        "linear1.weight": (8, 16), "linear1.bias": (8,),
        "linear2.weight": (3, 8), "linear2.bias": (3,)}
    assert not model.layers[0].conv1.scale.requires_grad
    # defect (a): the reference never initialises the conv weights; here they are 0.1
    assert torch.equal(model.layers[1].conv1.weight, torch.full((2, 5, 1, 1), 0.1))
    assert model.layers[0].conv1.bias is None


def test_edge_type_graph_against_dense_stack():
    A = GOLDEN["A"]
    n, T = A.shape[0], A.shape[2]
    etg = edge_type_graph(torch.from_numpy(A))
    assert isinstance(etg, EdgeTypeGraph) and (etg.n, etg.T) == (n, T)
    union = from_dense(torch.from_numpy((A.sum(2) > 0).astype(np.float32)), "positive")
    assert torch.equal(etg.U.rowptr, union.rowptr) and torch.equal(etg.U.col, union.col)
    rows = ops._entry_rows(etg.U).numpy()
    cols = etg.U.col.numpy()
    for t in range(T):
        np.testing.assert_array_equal(etg.tval[t].numpy(), A[rows, cols, t].astype(np.float32))
    # the same graph from COO lists with a duplicate (summed) and from CsrGraphs
    rels = []
    for t in range(T):
        row = torch.from_numpy(GOLDEN[f"rel{t}_row"].astype(np.int64))
        col = torch.from_numpy(GOLDEN[f"rel{t}_col"].astype(np.int64))
        rels.append(torch.sparse_coo_tensor(torch.stack([row, col]), torch.ones(row.numel()),
                                            (n, n)))
    again = edge_type_graph(rels)
    assert torch.equal(again.U.col, etg.U.col) and torch.equal(again.tval, etg.tval)
    row = torch.tensor([0, 0, 1]), torch.tensor([1, 1, 0])
    dup = edge_type_graph([torch.sparse_coo_tensor(torch.stack(row), torch.tensor([1., 2., 4.]),
                                                   (2, 2))])
    assert dup.U.col.tolist() == [1, 0] and dup.tval.tolist() == [[3.0, 4.0]]
    with pytest.raises(ValueError, match="negative"):
        edge_type_graph([torch.tensor([[0., -1.], [1., 0.]])])
    # S_2 is the pattern of the dense product
    u = (A.sum(2) > 0).astype(np.float64)
    s2 = from_dense(torch.from_numpy(u @ u), "positive")
    assert torch.equal(etg.S(2).g.col, s2.col) and torch.equal(etg.S(2).g.rowptr, s2.rowptr)


def random_pattern(rng, n, m, density):
    mask = rng.random((n, m)) < density
    g = from_dense(torch.from_numpy(mask.astype(np.float32)), "positive")
    return g, mask


def dense_of(g, v):
    out = np.zeros((v.shape[0], g.n_rows, g.n_cols))
    rows = ops._entry_rows(g).numpy()
    out[:, rows, g.col.numpy()] = v
    return out


def test_restatements_against_dense_float64():
    rng = np.random.default_rng(5)
    n, k, m, C = 13, 9, 11, 3
    for mode in (0, 1):
        a, _ = random_pattern(rng, n, k, 0.4)
        b, _ = random_pattern(rng, *((k, m) if mode == 0 else (m, k)), 0.4)
        p, pm = random_pattern(rng, n, m, 0.5)
        av, bv = rng.standard_normal((C, a.nnz)), rng.standard_normal((C, b.nnz))
        da, db = dense_of(a, av), dense_of(b, bv)
        full = da @ db if mode == 0 else da @ db.transpose(0, 2, 1)
        got = ops.masked_product_torch(mode, a, torch.from_numpy(av), b, torch.from_numpy(bv), p)
        np.testing.assert_allclose(dense_of(p, got.numpy()), full * pm, rtol=1e-12, atol=1e-12)
    g, gm = random_pattern(rng, n, n, 0.4)
    v = rng.standard_normal((C, g.nnz))
    x, xc = rng.standard_normal((n, 6)), rng.standard_normal((C, n, 6))
    dv = dense_of(g, v)
    off = 1 - np.eye(n)
    for skip in (False, True):
        d = dv * off if skip else dv
        np.testing.assert_allclose(
            ops.edge_aggregate_torch(g, torch.from_numpy(v), torch.from_numpy(x), skip).numpy(),
            d @ x, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(
            ops.edge_aggregate_torch(g, torch.from_numpy(v), torch.from_numpy(xc), skip).numpy(),
            d @ xc, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(
            ops.edge_rowsum_torch(g, torch.from_numpy(v), skip).numpy(), d.sum(2),
            rtol=1e-12, atol=1e-12)
        full = (xc @ x.T) * gm * (off if skip else 1)
        got = ops.edge_dot_torch(g, torch.from_numpy(xc), torch.from_numpy(x), skip).numpy()
        np.testing.assert_allclose(dense_of(g, got), full, rtol=1e-12, atol=1e-12)


def test_empty_columns_sparse_finite_dense_nan():
    """Defect (b): with isolated authors some off-diagonal columns of H are empty. The forward
    of the two paths agrees; the dense path's conv gradients are NaN as the reference's are; the
    sparse path's are finite."""
    A = GOLDEN["A"].astype(np.float32).copy()
    iso = [70, 71, 95]                                   # authors: cut every edge but the identity
    A[iso, :, :4] = 0
    A[:, iso, :4] = 0
    A, (_, X, target, labels) = torch.from_numpy(A), golden_inputs()
    dense, sparse = golden_model(2), golden_model(2)
    yd, _ = dense(A, X, target)
    ys, _ = sparse(edge_type_graph(A), X, target)
    close(ys, yd.detach().numpy(), "forward")
    torch.nn.functional.cross_entropy(yd, labels).backward()
    torch.nn.functional.cross_entropy(ys, labels).backward()
    assert torch.isnan(dense.layers[0].conv1.weight.grad).any()
    for name, p in sparse.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), name
    assert sparse.layers[0].conv1.weight.grad.abs().max() > 0


def test_product_entry_refuses_before_any_launch():
    """A workspace one byte short of the query, a mode outside {0, 1} and C outside [1, 8] are
    refused before anything reaches the device (host buffers stand in for the pointers)."""
    import ctypes
    from graphneuralnetwork_amd import _lib
    lib = _lib.load(build_if_missing=True)
    need = lib.gnn_masked_product_workspace_bytes(0, 0, 0, 0, 0, 0, 1)
    assert need > 0
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(mode, C, nbytes):
        return lib.gnn_masked_product_f32(mode, p, None, None, 0, p, None, None, 0, p, None, 0,
                                          0, 0, 0, C, None, 1, p, nbytes, None)

    assert call(0, 1, need - 1) == -1
    assert call(2, 1, need) == -1
    assert call(0, 9, need) == -3 and call(1, 0, need) == -3
    assert bytes(buf) == bytes(4096)
    lane_max, chunk = ops.masked_product_class_limits()
    assert 1 <= lane_max <= chunk == 64
