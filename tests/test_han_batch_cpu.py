"""HAN mini-batches without a device: the torch restatement of the induced subgraph
A[idx][:, idx] and ``collect_f`` on CPU tensors against the reference-generated fixture
(tests/golden/han_batch.npz, the reference's own collect_f) and dense numpy slicing, and the C
entries' argument rejection before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


def _relation(gd, key):
    shape = tuple(int(v) for v in gd[f"{key}_shape"])
    idx = torch.from_numpy(np.stack([gd[f"{key}_row"], gd[f"{key}_col"]]).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(gd[f"{key}_val"]), shape)


def _valued_graph(n, seed):
    """A seeded [n, n] graph with distinct values, columns in scrambled order within a row,
    edgeless rows and a self-loop on every third node; returns (CsrGraph, dense float32)."""
    from graphneuralnetwork_amd.graph import CsrGraph
    rng = np.random.default_rng(seed)
    dense = np.zeros((n, n), np.float32)
    mask = rng.random((n, n)) < 0.06
    mask[rng.choice(n, 12, replace=False)] = False
    mask[np.arange(0, n, 3), np.arange(0, n, 3)] = True
    rows = [rng.permutation(np.nonzero(mask[i])[0]) for i in range(n)]
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([r.size for r in rows])
    col = np.concatenate(rows).astype(np.int32)
    val = (np.arange(col.size) + 1).astype(np.float32)       # distinct: a misplaced value shows
    dense[np.repeat(np.arange(n), np.diff(rp)), col] = val
    g = CsrGraph(torch.from_numpy(rp), torch.from_numpy(col), torch.from_numpy(val), n, n)
    return g, dense


def _assert_is_slice(c, dense, idx):
    from graphneuralnetwork_amd.graph import from_dense
    idx = np.asarray(idx, np.int64)
    want = from_dense(torch.from_numpy(dense[idx][:, idx]), "positive")
    assert (c.n_rows, c.n_cols) == (idx.size, idx.size)
    assert c.rowptr.dtype == torch.int64 and c.col.dtype == torch.int32
    assert c.val.dtype == torch.float32
    assert torch.equal(c.rowptr, want.rowptr) and torch.equal(c.col, want.col)
    assert torch.equal(c.val, want.val)


def test_restatement_equals_numpy_slicing():
    from graphneuralnetwork_amd import hetero
    n = 200
    g, dense = _valued_graph(n, 7)
    rng = np.random.default_rng(8)
    cases = {"permuted": rng.permutation(n), "prefix": rng.permutation(n)[:37],
             "reversed": np.arange(n)[::-1].copy(), "identity": np.arange(n),
             "repeated": rng.integers(0, n, 90), "single": np.array([3]),
             "single_no_loop": np.array([4]), "empty": np.zeros(0, np.int64)}
    for name, idx in cases.items():
        c = hetero.induced_subgraph_torch(g, torch.from_numpy(idx.astype(np.int64)))
        _assert_is_slice(c, dense, idx)
        _assert_is_slice(hetero.induced_subgraph(g, idx.tolist()), dense, idx)  # CPU operands
    assert np.unique(cases["repeated"]).size < 90                # ids do repeat
    ident = hetero.induced_subgraph_torch(g, np.arange(n).tolist())
    # A's columns are scrambled within rows, so identity sorts them; a sorted A comes back as is
    again = hetero.induced_subgraph_torch(ident, torch.arange(n))
    assert torch.equal(again.rowptr, ident.rowptr) and torch.equal(again.col, ident.col)
    assert torch.equal(again.val, ident.val)


def test_collect_f_cpu_equals_reference(golden):
    from graphneuralnetwork_amd.graph import CsrGraph, from_dense
    from graphneuralnetwork_amd.hetero import HeteroGraph, collect_f
    gd, bd = golden("metapath"), golden("han_batch")
    keys = [str(k) for k in bd["keys"]]
    hg = HeteroGraph({k: _relation(gd, k) for k in keys}, device="cpu")
    batchify = collect_f(hg, bd["features"], bd["labels"])
    assert len(batchify.HGs_adj) == len(keys)
    assert batchify.features.dtype == torch.float32 and batchify.labels.dtype == torch.int64
    forms = {"tensors": lambda ids: [torch.tensor(int(v)) for v in ids],
             "numpy": lambda ids: [np.int64(v) for v in ids],
             "ints": lambda ids: [int(v) for v in ids],
             "tensor": lambda ids: torch.from_numpy(ids)}
    for name in (str(b) for b in bd["batches"]):
        ids = bd[f"{name}_idx"]
        for form, make in forms.items():
            adjs, feat, lab = batchify(make(ids))
            assert torch.equal(feat, torch.from_numpy(bd[f"{name}_features"])), (name, form)
            assert torch.equal(lab, torch.from_numpy(bd[f"{name}_labels"])), (name, form)
            for k, c in zip(keys, adjs):
                want = from_dense(torch.from_numpy(bd[f"{name}_{k}"]), "positive")
                assert isinstance(c, CsrGraph) and c.symmetric
                assert torch.equal(c.rowptr, want.rowptr) and torch.equal(c.col, want.col), \
                    (name, form, k)
                assert torch.equal(c.val, torch.ones_like(c.val))
    # a list of CsrGraphs is taken as it is; a list of dense arrays keeps the reference's line
    ids = bd["b65_idx"]
    graphs = list(hg)
    a1 = collect_f(graphs, bd["features"], bd["labels"])(torch.from_numpy(ids))[0]
    dense = collect_f([gd[f"{k}_adj"] for k in keys], bd["features"], bd["labels"])
    a2, feat, lab = dense([np.int64(v) for v in ids])
    for k, c, d in zip(keys, a1, a2):
        assert torch.equal(d, torch.from_numpy(bd[f"b65_{k}"]))
        want = from_dense(d, "positive")
        assert torch.equal(c.rowptr, want.rowptr) and torch.equal(c.col, want.col)
    assert torch.equal(feat, torch.from_numpy(bd["b65_features"]))
    assert (bd["b65_p_vs_a"].sum(1) == 0).any()                  # the fixture has edgeless rows


def test_collect_f_is_a_dataloader_collate_fn(golden):
    """the reference's own loader lines (load_data :112-115) over an index array and an index
    tensor: every batch is the dense slice of the full golden adjacency at the ids drawn"""
    from torch.utils.data import DataLoader
    from graphneuralnetwork_amd.graph import from_dense
    from graphneuralnetwork_amd.hetero import HeteroGraph, collect_f
    gd, bd = golden("metapath"), golden("han_batch")
    keys = [str(k) for k in bd["keys"]]
    n = int(gd[f"{keys[0]}_shape"][0])
    batchify = collect_f(HeteroGraph({k: _relation(gd, k) for k in keys}, device="cpu"),
                         bd["features"], bd["labels"])
    for index in (np.arange(n)[::3].copy(), torch.arange(n)[1::3]):
        torch.manual_seed(5)
        drawn = [torch.tensor([int(v) for v in d])
                 for d in DataLoader(index, batch_size=32, shuffle=True, collate_fn=list)]
        torch.manual_seed(5)
        batches = list(DataLoader(index, batch_size=32, shuffle=True, collate_fn=batchify))
        assert len(batches) == len(drawn) == -(-len(index) // 32)
        assert drawn[-1].numel() == len(index) % 32              # a short last batch
        for ids, (adjs, feat, lab) in zip(drawn, batches):
            assert torch.equal(feat, torch.from_numpy(bd["features"])[ids])
            assert torch.equal(lab, torch.from_numpy(bd["labels"])[ids])
            for k, c in zip(keys, adjs):
                want = from_dense(torch.from_numpy(gd[f"{k}_adj"])[ids][:, ids], "positive")
                assert torch.equal(c.rowptr, want.rowptr) and torch.equal(c.col, want.col)


def test_refusals():
    from graphneuralnetwork_amd import hetero
    from graphneuralnetwork_amd.graph import CsrGraph
    g, _ = _valued_graph(50, 1)
    for bad in ([0, 50], [-1], [3, 2 ** 40]):
        with pytest.raises(IndexError):
            hetero.induced_subgraph_torch(g, bad)
        with pytest.raises(IndexError):
            hetero.induced_subgraph(g, bad)
    # row 1 stores column 2 twice
    rp = torch.tensor([0, 1, 4, 5], dtype=torch.int64)
    col = torch.tensor([0, 2, 1, 2, 2], dtype=torch.int32)
    rep = CsrGraph(rp, col, torch.arange(5, dtype=torch.float32), 3, 3)
    for ids in ([1, 2], [0, 1, 2], [2, 1, 2]):
        with pytest.raises(ValueError, match="coalesce"):
            hetero.induced_subgraph_torch(rep, ids)
        with pytest.raises(ValueError, match="coalesce"):
            hetero.induced_subgraphs([rep], ids)
    # the repeat in an unselected row, or of an unselected column, passes
    c = hetero.induced_subgraph_torch(rep, [0, 2])
    assert c.rowptr.tolist() == [0, 1, 2] and c.col.tolist() == [0, 1]
    c = hetero.induced_subgraph_torch(rep, [1, 0])               # row 1 selected, column 2 not
    assert c.rowptr.tolist() == [0, 1, 2] and c.col.tolist() == [0, 1]
    assert c.val.tolist() == [2.0, 0.0]
    # a column id outside the graph in a selected row
    bad_col = CsrGraph(rp, torch.tensor([0, 2, 3, 1, 2], dtype=torch.int32),
                       torch.ones(5), 3, 3)
    with pytest.raises(IndexError):
        hetero.induced_subgraph_torch(bad_col, [1])
    assert hetero.induced_subgraph_torch(bad_col, [0, 2]).nnz == 2
    rect = CsrGraph(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                    torch.zeros(0), 3, 5)
    for fn in (hetero.induced_subgraph_torch, hetero.induced_subgraph):
        with pytest.raises(ValueError, match="square"):
            fn(rect, [0])
    with pytest.raises(ValueError):
        hetero.induced_subgraph_torch(g, torch.zeros((2, 2), dtype=torch.int64))
    sym = CsrGraph(rp, torch.tensor([0, 0, 1, 2, 2], dtype=torch.int32), torch.ones(5), 3, 3)
    assert not hetero.induced_subgraph(sym, [0, 1]).symmetric
    sym.symmetric = True
    assert hetero.induced_subgraph(sym, [0, 1]).symmetric


def test_capi_rejects_without_launch(lib):
    """null pointers and negative sizes -> GNN_E_ARG, a dimension at or above 2^31 - 1 ->
    GNN_E_UNSUPPORTED (the workspace query included), before anything reaches the device."""
    from graphneuralnetwork_amd.hetero import subgraph_class_limits
    E_ARG, E_UNSUPPORTED = -1, -3
    ws_bytes = lib.gnn_induced_subgraph_workspace_bytes
    lim = 2 ** 31 - 1
    s, m, bits = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    limits = lib.gnn_induced_subgraph_class_limits
    assert limits(None, ctypes.byref(m), ctypes.byref(bits)) == E_ARG
    assert limits(ctypes.byref(s), None, ctypes.byref(bits)) == E_ARG
    assert limits(ctypes.byref(s), ctypes.byref(m), None) == E_ARG
    assert limits(ctypes.byref(s), ctypes.byref(m), ctypes.byref(bits)) == 0
    assert 1 <= s.value < m.value < bits.value
    assert subgraph_class_limits() == (s.value, m.value, bits.value)
    assert ws_bytes(0, 0) > 0 and ws_bytes(10, 3) > 0
    for bad in ((-1, 1), (1, -1), (-5, -5)):
        assert ws_bytes(*bad) == E_ARG
    for big in ((lim, 1), (1, lim), (2 ** 40, 1), (1, 2 ** 40)):
        assert ws_bytes(*big) == E_UNSUPPORTED
    assert ws_bytes(lim - 1, 1) > 0
    # non-decreasing in n and in b, across the sizes at which the layout changes
    sizes = [0, 1, 63, 64, 65, 1000, m.value, m.value + 1, 10 ** 5, bits.value, bits.value + 1,
             bits.value + 65, 10 ** 6, 10 ** 7]
    for fixed in (0, 1000, 10 ** 6):
        in_n = [ws_bytes(v, fixed) for v in sizes]
        in_b = [ws_bytes(fixed, v) for v in sizes]
        assert all(x > 0 for x in in_n + in_b)
        assert in_n == sorted(in_n) and in_b == sorted(in_b), (fixed, in_n, in_b)
    assert ws_bytes(1000, bits.value + 1) > ws_bytes(1000, bits.value)  # bitmaps leave the LDS
    st = ctypes.c_int32(0)
    stp = ctypes.addressof(st)
    p = 4096                                     # plausible addresses, never dereferenced
    big_ws = 1 << 40
    fmap, count, fill = (lib.gnn_induced_subgraph_map, lib.gnn_induced_subgraph_count,
                         lib.gnn_induced_subgraph_fill)
    # (idx, b, n, status, workspace, workspace_bytes, stream)
    assert fmap(None, 4, 8, stp, p, big_ws, None) == E_ARG
    assert fmap(p, 4, 8, None, p, big_ws, None) == E_ARG
    assert fmap(p, 4, 8, stp, None, big_ws, None) == E_ARG
    assert fmap(p, 4, 8, stp, p, 16, None) == E_ARG
    assert fmap(p, -4, 8, stp, p, big_ws, None) == E_ARG
    assert fmap(p, 4, -8, stp, p, big_ws, None) == E_ARG
    assert fmap(p, lim, 8, stp, p, big_ws, None) == E_UNSUPPORTED
    assert fmap(p, 4, lim, stp, p, big_ws, None) == E_UNSUPPORTED
    # (rowptr, col, nnz, n, idx, b, c_rowptr, status, workspace, workspace_bytes, stream)
    assert count(None, p, 3, 8, p, 4, p, stp, p, big_ws, None) == E_ARG
    assert count(p, None, 3, 8, p, 4, p, stp, p, big_ws, None) == E_ARG
    assert count(p, p, -3, 8, p, 4, p, stp, p, big_ws, None) == E_ARG
    assert count(p, p, 3, -8, p, 4, p, stp, p, big_ws, None) == E_ARG
    assert count(p, p, 3, 8, None, 4, p, stp, p, big_ws, None) == E_ARG
    assert count(p, p, 3, 8, p, -4, p, stp, p, big_ws, None) == E_ARG
    assert count(p, p, 3, 8, p, 4, None, stp, p, big_ws, None) == E_ARG
    assert count(p, p, 3, 8, p, 4, p, None, p, big_ws, None) == E_ARG
    assert count(p, p, 3, 8, p, 4, p, stp, None, big_ws, None) == E_ARG
    assert count(p, p, 3, 8, p, 4, p, stp, p, 16, None) == E_ARG
    assert count(p, p, 3, lim, p, 4, p, stp, p, big_ws, None) == E_UNSUPPORTED
    assert count(p, p, 3, 8, p, lim, p, stp, p, big_ws, None) == E_UNSUPPORTED
    # (rowptr, col, val, nnz, n, idx, b, c_rowptr, c_col, c_val, nnz_c, status, ws, bytes, stream)
    assert fill(None, p, p, 3, 8, p, 4, p, p, p, 5, stp, p, big_ws, None) == E_ARG
    assert fill(p, None, p, 3, 8, p, 4, p, p, p, 5, stp, p, big_ws, None) == E_ARG
    assert fill(p, p, p, -3, 8, p, 4, p, p, p, 5, stp, p, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, None, 4, p, p, p, 5, stp, p, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, p, 4, None, p, p, 5, stp, p, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, p, 4, p, None, p, 5, stp, p, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, p, 4, p, p, p, -5, stp, p, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, p, 4, p, p, p, 5, None, p, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, p, 4, p, p, p, 5, stp, None, big_ws, None) == E_ARG
    assert fill(p, p, p, 3, 8, p, 4, p, p, p, 5, stp, p, 16, None) == E_ARG
    assert fill(p, p, p, 3, lim, p, 4, p, p, p, 5, stp, p, big_ws, None) == E_UNSUPPORTED
    assert fill(p, p, p, 3, 8, p, lim, p, p, p, 5, stp, p, big_ws, None) == E_UNSUPPORTED
    assert st.value == 0                                          # nothing touched the status
