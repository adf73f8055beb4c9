"""Metapath graphs without a device: the torch restatement of the boolean relation product and
``HeteroGraph`` on CPU tensors against the reference-generated fixture (tests/golden/
metapath.npz, the reference's own HeteroGraph) and a numpy dense product, and the C entries'
argument rejection before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


def _dense(g):
    a = np.zeros((g.n_rows, g.n_cols), np.uint8)
    rp = g.rowptr.numpy()
    a[np.repeat(np.arange(g.n_rows), np.diff(rp)), g.col.numpy()] = 1
    return a


def _check_sorted_set(g):
    rp, col = g.rowptr.numpy(), g.col.numpy()
    assert rp[0] == 0 and rp[-1] == col.size and (np.diff(rp) >= 0).all()
    for i in range(g.n_rows):
        assert (np.diff(col[rp[i]:rp[i + 1]]) > 0).all()   # ascending, no duplicate
    assert g.val.dtype == torch.float32 and bool((g.val == 1).all())


def _relation(gd, key):
    shape = tuple(int(v) for v in gd[f"{key}_shape"])
    idx = torch.from_numpy(np.stack([gd[f"{key}_row"], gd[f"{key}_col"]]).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(gd[f"{key}_val"]), shape)


def test_torch_restatement_equals_reference(golden):
    from graphneuralnetwork_amd import hetero
    from graphneuralnetwork_amd.graph import from_dense
    gd = golden("metapath")
    for key in gd["keys"]:
        rel = _relation(gd, key)
        n, k = rel.shape
        row, col = rel._indices()
        g = hetero.relation_product_torch((row, col, (n, k)), (col, row, (k, n)))
        _check_sorted_set(g)
        np.testing.assert_array_equal(_dense(g), gd[f"{key}_adj"])
        ref = from_dense(torch.from_numpy(gd[f"{key}_adj"]), "positive")
        assert torch.equal(g.rowptr, ref.rowptr) and torch.equal(g.col, ref.col)
        m = hetero.metapath_graph(rel)                       # CPU operands: the same restatement
        assert m.symmetric and torch.equal(m.rowptr, ref.rowptr) and torch.equal(m.col, ref.col)


def test_heterograph_cpu_equals_reference(golden):
    from graphneuralnetwork_amd.graph import from_torch_sparse
    from graphneuralnetwork_amd.hetero import HeteroGraph
    gd = golden("metapath")
    keys = [str(k) for k in gd["keys"]]
    hg = HeteroGraph({k: _relation(gd, k) for k in keys}, device="cpu")
    assert len(hg) == len(keys)
    for key, g in zip(keys, hg):
        assert g.n_rows == g.n_cols == int(gd[f"{key}_shape"][0]) and g.symmetric
        np.testing.assert_array_equal(_dense(g), gd[f"{key}_adj"])
        np.testing.assert_array_equal(_dense(hg.get_mate_path_graph(key)), gd[f"{key}_adj"])
    # every accepted relation type gives the same graph
    key = keys[0]
    rel = _relation(gd, key)
    want = gd[f"{key}_adj"]
    forms = {"csr": rel.coalesce().to_sparse_csr(), "dense": rel.to_dense()}
    forms["graph"] = from_torch_sparse(rel.coalesce(), "all")
    try:
        import scipy.sparse as sp
        forms["scipy"] = sp.csr_matrix((gd[f"{key}_val"], (gd[f"{key}_row"], gd[f"{key}_col"])),
                                       shape=tuple(gd[f"{key}_shape"]))
    except ImportError:
        pass
    for name, f in forms.items():
        np.testing.assert_array_equal(
            _dense(HeteroGraph({"x": f}, device="cpu").get_mate_path_graph("x")), want, name)


def test_heterograph_entry_semantics():
    from graphneuralnetwork_amd.hetero import HeteroGraph
    # entries > 0 are edges: a stored zero links nothing
    idx = torch.tensor([[0, 1, 2, 2], [0, 0, 0, 1]])
    rel = torch.sparse_coo_tensor(idx, torch.tensor([2.0, 0.0, 3.0, 1.0]), (3, 2))
    g = HeteroGraph({"r": rel}, device="cpu").get_mate_path_graph("r")
    np.testing.assert_array_equal(_dense(g), [[1, 0, 1], [0, 0, 0], [1, 0, 1]])
    bad = torch.sparse_coo_tensor(idx, torch.tensor([2.0, -1.0, 3.0, 1.0]), (3, 2))
    with pytest.raises(ValueError):
        HeteroGraph({"r": bad}, device="cpu").get_mate_path_graph("r")


def test_rectangular_product_equals_numpy():
    from graphneuralnetwork_amd import hetero
    rng = np.random.default_rng(5)
    n, k, m = 57, 23, 91
    A = rng.random((n, k)) < 0.08
    B = rng.random((k, m)) < 0.10
    A[5] = False                                             # an empty row of A
    B[3] = False                                             # an empty row of B, named by A
    A[:, 3] |= rng.random(n) < 0.3
    ar, ac = np.nonzero(A)
    br, bc = np.nonzero(B)
    dup = rng.integers(0, ar.size, 40)                       # duplicates, and a shuffled order
    ar, ac = np.concatenate([ar, ar[dup]]), np.concatenate([ac, ac[dup]])
    p = rng.permutation(ar.size)
    g = hetero.relation_product((torch.from_numpy(ar[p]), torch.from_numpy(ac[p]), (n, k)),
                                (torch.from_numpy(br), torch.from_numpy(bc), (k, m)))
    assert (g.n_rows, g.n_cols) == (n, m)
    _check_sorted_set(g)
    np.testing.assert_array_equal(_dense(g), ((A.astype(np.int64) @ B.astype(np.int64)) > 0))
    # degenerate shapes
    e = torch.zeros(0, dtype=torch.int64)
    g0 = hetero.relation_product_torch((e, e, (4, 3)), (e, e, (3, 6)))
    assert g0.nnz == 0 and g0.rowptr.tolist() == [0] * 5
    with pytest.raises(IndexError):
        hetero.relation_product_torch((torch.tensor([0]), torch.tensor([3]), (1, 3)),
                                      (e, e, (3, 2)))
    with pytest.raises(ValueError):
        hetero.relation_product_torch((e, e, (4, 3)), (e, e, (5, 6)))


def test_capi_rejects_without_launch(lib):
    """null pointers and negative sizes -> GNN_E_ARG, a dimension at or above 2^31 - 1 ->
    GNN_E_UNSUPPORTED (the workspace query included), before anything reaches the device."""
    E_ARG, E_UNSUPPORTED = -1, -3
    ws_bytes = lib.gnn_relation_product_workspace_bytes
    lim = 2 ** 31 - 1
    assert ws_bytes(10, 10, 10, 5, 5) > 0
    assert ws_bytes(0, 0, 0, 0, 0) > 0
    for bad in ((-1, 1, 1, 0, 0), (1, -1, 1, 0, 0), (1, 1, -1, 0, 0), (1, 1, 1, -1, 0),
                (1, 1, 1, 0, -1)):
        assert ws_bytes(*bad) == E_ARG
    for big in ((lim, 1, 1, 0, 0), (1, lim, 1, 0, 0), (1, 1, lim, 0, 0), (2 ** 40, 1, 1, 0, 0)):
        assert ws_bytes(*big) == E_UNSUPPORTED
    assert ws_bytes(lim - 1, 1, 1, 0, 0) > 0
    # the size does not depend on how the entries are spread: it is a function of the five sizes
    small, big_nnz = ws_bytes(1000, 50, 1000, 3000, 3000), ws_bytes(1000, 50, 1000, 10 ** 9, 10 ** 9)
    assert small == big_nnz
    s, m = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.gnn_relation_product_class_limits(None, ctypes.byref(m)) == E_ARG
    assert lib.gnn_relation_product_class_limits(ctypes.byref(s), None) == E_ARG
    assert lib.gnn_relation_product_class_limits(ctypes.byref(s), ctypes.byref(m)) == 0
    assert 1 <= s.value < m.value
    nnz = ctypes.c_int64(0)
    out = ctypes.addressof(nnz)
    count, fill = lib.gnn_relation_product_count, lib.gnn_relation_product_fill
    # (a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b, n, k, m, c_rowptr, nnz_out, ws, bytes, s)
    assert count(None, None, 0, None, None, 0, 4, 4, 4, None, out, None, 0, None) == E_ARG
    assert count(None, None, 0, None, None, 0, -4, 4, 4, None, out, None, 0, None) == E_ARG
    assert count(None, None, -1, None, None, 0, 4, 4, 4, None, out, None, 0, None) == E_ARG
    assert count(None, None, 0, None, None, 0, lim, 4, 4, None, out, None, 0, None) == E_UNSUPPORTED
    # plausible (never dereferenced) addresses, but no workspace / a workspace too small
    p = 4096
    assert count(p, p, 3, p, p, 3, 4, 4, 4, p, out, None, 1 << 30, None) == E_ARG
    assert count(p, p, 3, p, p, 3, 4, 4, 4, p, out, p, 16, None) == E_ARG
    assert count(p, None, 3, p, p, 3, 4, 4, 4, p, out, p, 1 << 30, None) == E_ARG
    assert count(p, p, 3, p, p, 3, 4, 4, 4, p, None, p, 1 << 30, None) == E_ARG
    assert fill(None, None, 0, None, None, 0, 4, 4, 4, None, None, 0, None, 0, None) == E_ARG
    assert fill(p, p, 3, p, p, 3, 4, 4, 4, p, None, 5, p, 1 << 30, None) == E_ARG
    assert fill(p, p, 3, p, p, 3, 4, 4, 4, p, p, -1, p, 1 << 30, None) == E_ARG
    assert fill(p, p, 3, p, p, 3, 4, 4, 4, p, p, 5, p, 16, None) == E_ARG
    assert fill(p, p, 3, p, p, 3, 4, lim, 4, p, p, 5, p, 1 << 30, None) == E_UNSUPPORTED
