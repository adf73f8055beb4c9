"""Induced subgraph A[idx][:, idx] on the device (csrc/induced_subgraph.hip) against dense numpy
slicing: rowptr, col and val exactly, through the C entries with -1 / -7 filled outputs, guard
tails behind every output and behind a workspace of exactly the queried size. A's values are the
entries' ordinals, so a misplaced value shows. Each case is the smallest shape at which one path
of the kernels can go wrong. Then ``collect_f`` and ``HANModel`` on the reference's batches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
BAD_IDX, BAD_GRAPH, REPEAT = 1, 2, 4


def _graph(rp, col, n, dev):
    """CsrGraph [n, n] of numpy (rowptr, col), columns kept in the order given; the value of an
    entry is its ordinal in col."""
    from graphneuralnetwork_amd.graph import CsrGraph
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64).astype(np.int32)
    return CsrGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev),
                    torch.arange(col.size, dtype=torch.float32, device=dev), n, n)


def _from_rows(rows, dev, n=None):
    n = len(rows) if n is None else n
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows]) if rp[-1] else \
        np.zeros(0, np.int64)
    return _graph(rp, col, n, dev)


def _random_graph(n, p, seed, dev, scramble=True, empty=()):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < p
    mask[list(empty)] = False
    rows = [np.nonzero(mask[i])[0] for i in range(n)]
    if scramble:
        rows = [rng.permutation(r) for r in rows]
    return _from_rows(rows, dev)


def _oracle(g, idx):
    """(rowptr, col, val) of dense(A)[idx][:, idx] read row-major, dense(A) holding ordinal + 1:
    dense numpy slicing up to 25 M entries on either side; else, for an idx without repeats, the
    per-row "positions of the kept columns, sorted" form, which is the same thing stated without
    the array."""
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy().astype(np.int64)
    n, b = g.n_rows, idx.size
    rowptr = np.zeros(b + 1, np.int64)
    if n * n <= 25_000_000 and b * b <= 25_000_000:
        dense = np.zeros((n, n), np.float32)
        row, ok = np.repeat(np.arange(n), np.diff(rp)), (col >= 0) & (col < n)
        assert not np.isin(row[~ok], idx).any()              # a bad id only in an unselected row
        dense[row[ok], col[ok]] = (np.arange(col.size) + 1)[ok]
        S = dense[idx][:, idx] if b else np.zeros((0, 0), np.float32)
        r, c = np.nonzero(S)
        rowptr[1:] = np.cumsum((S != 0).sum(1))
        return rowptr, c.astype(np.int32), S[r, c] - 1
    assert np.unique(idx).size == b
    pos = np.full(n, -1, np.int64)
    pos[idx] = np.arange(b)
    deg = rp[idx + 1] - rp[idx]
    r = np.repeat(np.arange(b), deg)
    src = np.repeat(rp[idx] - (np.cumsum(deg) - deg), deg) + np.arange(int(deg.sum()))
    p = pos[col[src]]
    keep = p >= 0
    r, p, src = r[keep], p[keep], src[keep]
    order = np.lexsort((p, r))
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=b))
    return rowptr, p[order].astype(np.int32), src[order].astype(np.float32)


def _run(gs, idx, dev, with_val=True, ws=None):
    """map, a count per graph, a fill per graph on one workspace through the C entries. Returns
    ([(rowptr, col, val)] as numpy or None after an idx / graph error, status, workspace)."""
    from graphneuralnetwork_amd import _lib
    lib = _lib.load()
    idx = torch.as_tensor(np.asarray(idx, np.int64)).to(dev)
    n, b = gs[0].n_rows, idx.numel()
    nbytes = int(lib.gnn_induced_subgraph_workspace_bytes(n, b))
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    assert ws.numel() == nbytes + 4096
    status = torch.zeros(1 + GUARD, dtype=torch.int32, device=dev)
    batch = dict(idx=idx.data_ptr() or None, b=b, n=n, status=status.data_ptr(),
                 workspace=ws.data_ptr(), workspace_bytes=nbytes,
                 stream=_lib.stream_handle(dev))
    _lib.run("gnn_induced_subgraph_map", **batch)
    rps = []
    for g in gs:
        rp = torch.full((b + 1 + GUARD,), -7, dtype=torch.int64, device=dev)
        _lib.run("gnn_induced_subgraph_count", rowptr=g.rowptr.data_ptr(),
                 col=g.col.data_ptr() or None, nnz=g.nnz, c_rowptr=rp.data_ptr(), **batch)
        rps.append(rp)
    torch.cuda.synchronize(dev)
    st = int(status[0])
    for rp in rps:
        assert bool((rp[b + 1:] == -7).all()), "count wrote past rowptr"
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace query is too small"
    if st & (BAD_IDX | BAD_GRAPH):
        return None, st, ws
    outs = []
    for g, rp in zip(gs, rps):
        nz = int(rp[b])
        assert nz >= 0 and int(rp[0]) == 0
        col = torch.full((nz + GUARD,), -1, dtype=torch.int32, device=dev)
        val = torch.full((nz + GUARD,), -7.0, dtype=torch.float32, device=dev)
        _lib.run("gnn_induced_subgraph_fill", rowptr=g.rowptr.data_ptr(),
                 col=g.col.data_ptr() or None, val=g.val.data_ptr() or None, nnz=g.nnz,
                 c_rowptr=rp.data_ptr(), c_col=col.data_ptr(),
                 c_val=val.data_ptr() if with_val else None, nnz_c=nz, **batch)
        outs.append((rp, col, val, nz))
    torch.cuda.synchronize(dev)
    st = int(status[0])
    res = []
    for rp, col, val, nz in outs:
        assert bool((col[nz:] == -1).all()), "fill wrote ids past nnz"
        assert bool((val[nz:] == -7.0).all()), "fill wrote values past nnz"
        assert bool((rp[b + 1:] == -7).all())
        if st == 0:
            assert not bool((col[:nz] == -1).any()), "fill left ids unwritten"
            if with_val:
                assert not bool((val[:nz] == -7.0).any()), "fill left values unwritten"
            else:
                assert bool((val == -7.0).all()), "a structure-only fill wrote values"
        res.append((rp[:b + 1].cpu().numpy(), col[:nz].cpu().numpy(), val[:nz].cpu().numpy()))
    assert bool((status[1:] == 0).all()), "something wrote behind the status word"
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace query is too small"
    return res, st, ws


def _check(g, idx, dev, with_val=True):
    idx = np.asarray(idx, np.int64)
    res, st, _ = _run([g], idx, dev, with_val)
    assert st == 0
    rp, col, val = res[0]
    want_rp, want_col, want_val = _oracle(g, idx)
    np.testing.assert_array_equal(rp, want_rp)
    np.testing.assert_array_equal(col, want_col)
    if with_val:
        np.testing.assert_array_equal(val, want_val)
    return rp, col, val


@pytest.fixture(scope="module")
def limits(dev):
    from graphneuralnetwork_amd.hetero import subgraph_class_limits
    s, m, bits = subgraph_class_limits()
    assert 1 <= s < m < bits
    return s, m, bits


def test_empty_and_tiny(dev):
    rows = [[], [1, 3, 2], [], [6, 0, 1, 3], [], [6, 2], []]   # edgeless first, last, in between
    g = _from_rows(rows, dev)
    _check(g, [], dev)                                       # b = 0
    _check(g, [1], dev)                                      # b = 1 on a self-loop
    _check(g, [5], dev)                                      # b = 1 without one
    _check(g, [0, 2, 4, 6], dev)                             # only edgeless rows
    _check(g, [0, 1, 2, 3, 4, 5, 6], dev)
    _check(g, [6, 3, 0, 1], dev)
    _check(_from_rows([[0]], dev), [0], dev)                 # n = 1
    _check(_from_rows([[0]], dev), [0, 0, 0], dev)
    _check(_from_rows([[]], dev), [0], dev)
    _check(_from_rows([[], [], [], [], []], dev), [3, 1], dev)  # nnz(A) = 0
    _check(_from_rows([[], [], [], [], []], dev), [], dev)


def test_orders(dev, limits):
    n = 500
    sorted_g = _random_graph(n, 0.1, 11, dev, scramble=False, empty=(0, 17, n - 1))
    assert int((sorted_g.rowptr[1:] - sorted_g.rowptr[:-1]).max()) > limits[0]  # mid rows too
    rp, col, val = _check(sorted_g, np.arange(n), dev)
    np.testing.assert_array_equal(rp, sorted_g.rowptr.cpu().numpy())   # A's arrays bit for bit
    np.testing.assert_array_equal(col, sorted_g.col.cpu().numpy())
    np.testing.assert_array_equal(val, sorted_g.val.cpu().numpy())
    rng = np.random.default_rng(12)
    _check(sorted_g, np.arange(n)[::-1].copy(), dev)
    _check(sorted_g, rng.permutation(n), dev)
    _check(sorted_g, rng.permutation(n)[:211], dev)
    g = _random_graph(n, 0.1, 13, dev, scramble=True, empty=(3,))
    for idx in (np.arange(n), rng.permutation(n), rng.permutation(n)[:333]):
        rp, col, _ = _check(g, idx, dev)
        for r in range(idx.size):
            assert (np.diff(col[rp[r]:rp[r + 1]]) > 0).all()  # ascending out of a scrambled A
    _check(g, rng.permutation(n), dev, with_val=False)       # c_val null: structure only


def test_repeated_ids(dev, limits):
    n = 500
    g = _random_graph(n, 0.08, 21, dev)
    rng = np.random.default_rng(22)
    idx = rng.integers(0, n, 300)
    assert np.unique(idx).size < 300
    _check(g, idx, dev)
    _check(g, np.concatenate([idx, idx[::-1]]), dev)
    # one self-looped node 70 times: every row keeps 70 > short_max entries through one chain
    rows = [[1, 4], [0], [2], [5, 3, 0], [], [3]]
    loop = _from_rows(rows, dev)
    assert 70 > limits[0]
    rp, col, val = _check(loop, [3] * 70, dev)
    assert (np.diff(rp) == 70).all() and (val == 5).all()    # entry 5 is the loop (3, 3)
    _check(loop, [3] * 70 + [5, 0, 3], dev)
    _check(loop, [4, 4, 0, 4, 1], dev)                       # a repeated id whose row is edgeless


def test_rows_on_the_class_limits(dev, limits):
    """kept counts one below, at and one above each class limit; every such row also names three
    times as many unselected columns; b = mid_max + 300 with positions scrambled"""
    s_max, m_max, _ = limits
    b = m_max + 300
    n = 5 * b
    rng = np.random.default_rng(31)
    perm = rng.permutation(n)
    idx, rest = perm[:b], perm[b:]
    kept = (s_max - 1, s_max, s_max + 1, m_max - 1, m_max, m_max + 1)
    rows = [rng.integers(0, n, int(rng.integers(0, 4))) for _ in range(n)]
    for j, k in enumerate(kept):
        cols = np.concatenate([rng.choice(idx, k, replace=False),
                               rng.choice(rest, 3 * k, replace=False)])
        rows[idx[7 * j]] = rng.permutation(cols)
    rows = [np.unique(r) if len(r) < 8 else r for r in rows]  # no repeated column in a row
    g = _from_rows(rows, dev)
    rp, col, val = _check(g, idx, dev)
    for j, k in enumerate(kept):
        assert rp[7 * j + 1] - rp[7 * j] == k


def test_long_row_few_kept(dev):
    """a row of 100,000 entries that keeps 3: its first, its last and the one at ordinal 63 / 64
    (the last lane of the first step, the first lane of the second)"""
    n, deg = 120_000, 100_000
    rng = np.random.default_rng(41)
    perm = rng.permutation(n)
    v, cols, outside = perm[0], perm[1:deg + 1], perm[deg + 1:]
    rows = [np.zeros(0, np.int64)] * n
    rows[v] = cols
    rows[cols[0]] = np.array([v, cols[5]])
    g = _from_rows(rows, dev)
    for mid in (63, 64):
        idx = np.concatenate([outside[:9], [cols[mid], v], outside[9:20], [cols[-1], cols[0]]])
        rp, col, val = _check(g, idx, dev)
        r = 10
        assert rp[r + 1] - rp[r] == 3
        base = int(g.rowptr[v])
        assert sorted(val[rp[r]:rp[r + 1]] - base) == [0, mid, deg - 1]


def test_lds_bitmap_complete_then_sparse(dev, limits):
    """b = 3001 bits (not a multiple of 64) in LDS: complete rows (kept = b, positions 0 and b - 1
    present) and sparse heavy rows, more of them than persistent workgroups, so workgroups take a
    sparse row after a complete one and stale bits would show"""
    s_max, m_max, bits = limits
    b, n = 3001, 4000
    assert m_max < b <= bits
    rng = np.random.default_rng(51)
    perm = rng.permutation(n)
    idx, rest = perm[:b], perm[b:]
    rows = [np.zeros(0, np.int64)] * n
    heavy = idx[:1400]
    for j, v in enumerate(heavy):
        if j % 2 == 0:
            cols = np.concatenate([idx, rng.choice(rest, 50, replace=False)])
        else:
            cols = np.concatenate([rng.choice(idx, m_max + 52, replace=False),
                                   rng.choice(rest, 300, replace=False)])
        rows[v] = rng.permutation(cols)
    for v in idx[1400:]:
        rows[v] = rng.choice(n, int(rng.integers(0, 100)), replace=False)
    g = _from_rows(rows, dev)
    rp, col, val = _check(g, idx, dev)
    assert rp[1] - rp[0] == b and col[0] == 0 and col[rp[1] - 1] == b - 1   # a complete row
    assert rp[2] - rp[1] == m_max + 52


def test_workspace_bitmap_hub_and_sparse(dev, limits):
    """b = lds_bits + 65: the bitmaps live in the workspace. One hub row adjacent to every
    selected node and sparse heavy rows, more than the workspace holds bitmaps for."""
    s_max, m_max, bits = limits
    b = bits + 65
    n = b + 1000
    rng = np.random.default_rng(61)
    perm = rng.permutation(n)
    idx, rest = perm[:b], perm[b:]
    rows = [np.zeros(0, np.int64)] * n
    rows[idx[3]] = rng.permutation(np.concatenate([idx, rest[:100]]))          # the hub
    for j in range(70):
        rows[idx[10 + 13 * j]] = rng.permutation(np.concatenate(
            [rng.choice(idx, m_max + 1 + j, replace=False), rng.choice(rest, 200, replace=False)]))
    for v in idx[2000:2600]:
        rows[v] = rng.choice(n, int(rng.integers(1, 200)), replace=False)      # short and mid rows
    g = _from_rows(rows, dev)
    rp, col, val = _check(g, idx, dev)
    assert rp[4] - rp[3] == b and col[rp[3]] == 0 and col[rp[4] - 1] == b - 1
    assert rp[11] - rp[10] == m_max + 1


def test_errors(dev, limits):
    from graphneuralnetwork_amd import hetero
    s_max, m_max, _ = limits
    n = 2300
    rng = np.random.default_rng(71)
    idx = rng.permutation(n)[:m_max + 152]
    rest = np.setdiff1d(np.arange(n), idx)
    rows = [rng.choice(n, int(rng.integers(0, 6)), replace=False) for _ in range(n)]
    good = _from_rows(rows, dev)
    _, st, ws = _run([good], idx, dev)
    assert st == 0
    # an idx entry outside [0, n): bit 0
    for bad_id in (-1, n, 2 ** 40):
        bad = idx.copy()
        bad[5] = bad_id
        res, st, _ = _run([good], bad, dev, ws=ws)
        assert res is None and st & BAD_IDX
        with pytest.raises(IndexError):
            hetero.induced_subgraph(good, torch.from_numpy(bad).to(dev))
    # a column id outside [0, n) in a selected row: bit 1; in an unselected row it is never read
    for bad_col in (-1, n):
        rows2 = list(rows)
        rows2[idx[9]] = np.array([idx[1], bad_col, idx[2]])
        g2 = _from_rows(rows2, dev, n)
        res, st, _ = _run([g2], idx, dev, ws=ws)
        assert res is None and st == BAD_GRAPH
        with pytest.raises(IndexError):
            hetero.induced_subgraph(g2, torch.from_numpy(idx).to(dev))
        rows2 = list(rows)
        rows2[rest[0]] = np.array([idx[1], bad_col, idx[2]])
        _check(_from_rows(rows2, dev, n), idx, dev)
    # a selected row that repeats a selected column: bit 2, in each class of kept count
    for k in (5, s_max + 36, m_max + 52):
        rows2 = list(rows)
        cols = rng.choice(idx, k, replace=False)
        rows2[idx[4]] = rng.permutation(np.concatenate([cols, cols[:1], rest[:40]]))
        g2 = _from_rows(rows2, dev, n)
        _, st, _ = _run([g2], idx, dev, ws=ws)
        assert st == REPEAT, k
        with pytest.raises(ValueError, match="coalesce"):
            hetero.induced_subgraph(g2, torch.from_numpy(idx).to(dev))
        # the same repeat in an unselected row, or of an unselected column, passes
        rows2[rest[3]] = rows2[idx[4]]
        rows2[idx[4]] = rng.permutation(np.concatenate([cols, rest[:40], rest[:40]]))
        _check(_from_rows(rows2, dev, n), idx, dev)
    # a valid call on the same workspace afterwards succeeds
    res, st, _ = _run([good], idx, dev, ws=ws)
    want = _oracle(good, idx)
    assert st == 0
    for got, exp in zip(res[0], want):
        np.testing.assert_array_equal(got, exp)


def test_one_map_many_graphs(dev):
    from graphneuralnetwork_amd import hetero
    n = 800
    gs = [_random_graph(n, p, 80 + i, dev, empty=(i,)) for i, p in enumerate((0.01, 0.1, 0.3))]
    rng = np.random.default_rng(83)
    idx = np.concatenate([rng.permutation(n)[:350], rng.integers(0, n, 50)])
    together, st, ws = _run(gs, idx, dev)                    # one map, count x 3, fill x 3
    assert st == 0
    again, st2, _ = _run(gs, idx, dev, ws=ws)
    assert st2 == 0
    for g, t, a in zip(gs, together, again):
        single, st1, _ = _run([g], idx, dev)
        want = _oracle(g, idx)
        for x, y, z, w in zip(t, a, single[0], want):
            np.testing.assert_array_equal(x, y)              # two runs are bit-identical
            np.testing.assert_array_equal(x, z)              # and equal a call of their own
            np.testing.assert_array_equal(x, w)
    idx_t = torch.from_numpy(idx).to(dev)
    got = hetero.induced_subgraphs(gs, idx_t)
    for g, c in zip(gs, got):
        t = hetero.induced_subgraph_torch(g, idx_t)
        h = hetero.induced_subgraph_torch(g.to("cpu"), idx_t.cpu())
        assert c.rowptr.is_cuda and (c.n_rows, c.n_cols) == (idx.size, idx.size)
        for x, y, z in ((c.rowptr, t.rowptr, h.rowptr), (c.col, t.col, h.col),
                        (c.val, t.val, h.val)):
            assert torch.equal(x, y) and torch.equal(x.cpu(), z)


def _relation(gd, key, dev):
    shape = tuple(int(v) for v in gd[f"{key}_shape"])
    i = torch.from_numpy(np.stack([gd[f"{key}_row"], gd[f"{key}_col"]]).astype(np.int64))
    return torch.sparse_coo_tensor(i, torch.from_numpy(gd[f"{key}_val"]), shape).to(dev)


@pytest.fixture(scope="module")
def batchify(golden, dev):
    from graphneuralnetwork_amd.hetero import HeteroGraph, collect_f
    gd, bd = golden("metapath"), golden("han_batch")
    keys = [str(k) for k in bd["keys"]]
    return collect_f(HeteroGraph({k: _relation(gd, k, dev) for k in keys}), bd["features"],
                     bd["labels"], device=dev)


def _model(bd, dev, dropout):
    from graphneuralnetwork_amd.han import HANModel
    M, fin, hid, out, heads = (int(v) for v in bd["model"])
    net = HANModel(M, fin, hid, out, [heads], dropout)
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in bd.items()
                         if k.startswith("sd_")}, strict=True)
    return net.to(dev)


def test_golden_collect_f(golden, dev, batchify):
    from graphneuralnetwork_amd.graph import CsrGraph, from_dense
    bd = golden("han_batch")
    keys = [str(k) for k in bd["keys"]]
    assert all(g.rowptr.is_cuda for g in batchify.HGs_adj) and batchify.features.is_cuda
    for name in (str(v) for v in bd["batches"]):
        ids = bd[f"{name}_idx"]
        for data in ([torch.tensor(int(v)) for v in ids], [np.int64(v) for v in ids]):
            adjs, feat, lab = batchify(data)
            assert torch.equal(feat.cpu(), torch.from_numpy(bd[f"{name}_features"]))
            assert torch.equal(lab.cpu(), torch.from_numpy(bd[f"{name}_labels"]))
            for k, c in zip(keys, adjs):
                want = from_dense(torch.from_numpy(bd[f"{name}_{k}"]).to(dev), "positive")
                assert isinstance(c, CsrGraph) and c.rowptr.is_cuda and c.symmetric
                assert torch.equal(c.rowptr, want.rowptr) and torch.equal(c.col, want.col), \
                    (name, k)
                assert torch.equal(c.val, torch.ones_like(c.val))


def test_golden_han_model_on_a_batch(golden, dev, batchify):
    bd = golden("han_batch")
    keys = [str(k) for k in bd["keys"]]
    net = _model(bd, dev, 0.6).eval()
    adjs, feat, _ = batchify(torch.from_numpy(bd["b65_idx"]))
    dense = [torch.from_numpy(bd[f"b65_{k}"]).to(dev).float() for k in keys]
    assert any(bool((d.sum(1) == 0).any()) for d in dense)   # the batch has edgeless rows
    with torch.no_grad():
        got, same = net(adjs, feat), net(dense, feat)
    ref = bd["b65_logits"].astype(np.float64)
    scale = max(1.0, float(np.abs(ref).max()))
    print("max |got - ref| =", float(np.abs(got.cpu().numpy() - ref).max()), "scale", scale)
    # the project's fp32 bar against the reference (tests/test_han_sagepy_gpu.py::close)
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), ref, rtol=1e-4,
                               atol=2e-5 * scale)
    # identical CSR arrays into the same kernels: only fp32 summation order could differ
    print("max |got - dense path| =", float((got - same).abs().max()))
    torch.testing.assert_close(got, same, rtol=1e-5, atol=1e-6)


def test_training_step_on_a_batch(golden, dev, batchify):
    bd = golden("han_batch")
    keys = [str(k) for k in bd["keys"]]
    adjs, feat, lab = batchify(torch.from_numpy(bd["b65_idx"]))
    dense = [torch.from_numpy(bd[f"b65_{k}"]).to(dev).float() for k in keys]
    grads = []
    for graphs in (adjs, dense):
        net = _model(bd, dev, 0.0).train()
        loss = torch.nn.functional.cross_entropy(net(graphs, feat), lab)
        loss.backward()
        grads.append((loss.detach(), {k: p.grad for k, p in net.named_parameters()}))
    (l1, g1), (l2, g2) = grads
    torch.testing.assert_close(l1, l2, rtol=1e-5, atol=1e-6)
    assert g1.keys() == g2.keys() and all(v is not None for v in g1.values())
    worst = max(float((g1[k] - g2[k]).abs().max()) for k in g1)
    print("max |grad(csr) - grad(dense)| =", worst)
    for k in g1:
        assert torch.isfinite(g1[k]).all()
        torch.testing.assert_close(g1[k], g2[k], rtol=1e-5, atol=1e-6, msg=lambda m: f"{k}: {m}")
