"""The GTN kernels (csrc/gtn.hip) through their C entries against dense float64 numpy: ``out``
prefilled with NaN, guard tails behind every output and behind a workspace of exactly the
queried size. Each case is the smallest shape that exercises one path.

Two value regimes. Small integers: every sum stays below 2^24, so fp32 is exact and the
comparison is ``assert_array_equal``. Uniform [0.5, 1.5]: no cancellation, so the bound is
derived, not measured: a chain of K fused multiply-adds (or K products and their sum in any
order) errs by at most (K + 1) 2^-23 sum|terms|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
EPS = 2.0 ** -23
E_ARG = -1


def _csr(rows, n_cols, dev):
    """CsrGraph of per-row id sequences, kept in the order given, duplicates kept."""
    from graphneuralnetwork_amd.graph import CsrGraph
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = (np.concatenate([np.asarray(r, np.int64) for r in rows]) if rp[-1]
           else np.zeros(0, np.int64)).astype(np.int32)
    return CsrGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev),
                    torch.ones(col.size, device=dev), len(rows), n_cols)


def _dense(rows, n_cols, v):
    """[C, n, n_cols] float64 with every stored entry ADDED (a repeated id contributes twice)."""
    out = np.zeros((v.shape[0], len(rows), n_cols))
    e = 0
    for r, ids in enumerate(rows):
        for c in ids:
            out[:, r, c] += v[:, e]
            e += 1
    return out


def _values(rng, regime, C, nnz):
    if regime == "int":
        return rng.integers(1, 4, size=(C, nnz)).astype(np.float32)
    return rng.uniform(0.5, 1.5, size=(C, nnz)).astype(np.float32)


def _call_product(mode, a, av, b, bv, p, dims, C, dev, validate=1):
    """One call through the C entry; (rc, out [C, nnz_p] numpy) after the guard checks."""
    from graphneuralnetwork_amd import _lib
    lib = _lib.load()
    n, k, m = dims
    nbytes = int(lib.gnn_masked_product_workspace_bytes(n, k, m, a.nnz, b.nnz, p.nnz, C))
    assert nbytes > 0
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((C * p.nnz + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    av = torch.from_numpy(av).to(dev)
    bv = torch.from_numpy(bv).to(dev)
    rc = _lib.invoke(
        "gnn_masked_product_f32", mode=mode, a_rowptr=a.rowptr.data_ptr(),
        a_col=a.col.data_ptr() or None, a_val=av.data_ptr() or None, nnz_a=a.nnz,
        b_rowptr=b.rowptr.data_ptr(), b_col=b.col.data_ptr() or None,
        b_val=bv.data_ptr() or None, nnz_b=b.nnz, p_rowptr=p.rowptr.data_ptr(),
        p_col=p.col.data_ptr() or None, nnz_p=p.nnz, n=n, k=k, m=m, C=C, out=out.data_ptr(),
        validate=validate, workspace=ws.data_ptr(), workspace_bytes=nbytes,
        stream=_lib.stream_handle(dev))
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out[C * p.nnz:]).all()), "wrote past the output"
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace query is too small"
    if rc == 0:
        assert not bool(torch.isnan(out[:C * p.nnz]).any()), "a P entry was left unwritten"
    return rc, out[:C * p.nnz].view(C, p.nnz)


def _check_product(mode, a_rows, b_rows, p_rows, dims, C, regime, dev, seed=0):
    """Both operands given as row lists; compares with the dense float64 product on P and
    returns the device result."""
    n, k, m = dims
    rng = np.random.default_rng(seed)
    a = _csr(a_rows, k, dev)
    b = _csr(b_rows, m if mode == 0 else k, dev)
    p = _csr(p_rows, m, dev)
    av, bv = _values(rng, regime, C, a.nnz), _values(rng, regime, C, b.nnz)
    rc, out = _call_product(mode, a, av, b, bv, p, dims, C, dev)
    assert rc == 0
    rc2, again = _call_product(mode, a, av, b, bv, p, dims, C, dev, validate=0)
    assert rc2 == 0 and torch.equal(out, again)
    da, db = _dense(a_rows, k, av), _dense(b_rows, m if mode == 0 else k, bv)
    full = da @ db if mode == 0 else da @ db.transpose(0, 2, 1)
    prow = np.repeat(np.arange(n), [len(r) for r in p_rows])
    pcol = p.col.cpu().numpy().astype(np.int64)
    want = full[:, prow, pcol]
    got = out.cpu().numpy()
    if regime == "int":
        np.testing.assert_array_equal(got, want.astype(np.float32))
    else:
        walked = np.array([len(r) for r in (a_rows if mode == 0 else b_rows)])
        K = walked[prow] if mode == 0 else walked[pcol]
        bound = (K + 1) * EPS * want            # all terms positive: sum|terms| is the sum
        assert (np.abs(got - want) <= bound).all(), float(np.abs(got - want).max())
    # an entry nothing reaches is +0.0 exactly
    assert not np.signbit(got[want == 0]).any() and (got[want == 0] == 0).all()
    return got, want


@pytest.fixture(scope="module")
def limits(dev):
    from graphneuralnetwork_amd.ops import masked_product_class_limits
    lane_max, chunk = masked_product_class_limits()
    assert 1 <= lane_max and chunk == 64
    return lane_max, chunk


def _ascending(rng, hi, size):
    return np.sort(rng.choice(hi, size=min(size, hi), replace=False))


def _random_case(rng, mode, n, k, m, walked_lens, p_lens):
    """Row lists (a_rows, b_rows, p_rows): walked rows unsorted with repeats, searched rows
    strictly ascending, P rows distinct ids in any order (reached and unreached ones)."""
    if mode == 0:
        a_rows = [rng.integers(0, k, size=L) for L in walked_lens]                 # n rows
        b_rows = [_ascending(rng, m, int(rng.integers(0, 9))) for _ in range(k)]
    else:
        a_rows = [_ascending(rng, k, int(rng.integers(0, 9))) for _ in range(n)]
        b_rows = [rng.integers(0, k, size=L) for L in walked_lens]                 # m rows
    p_rows = [rng.choice(m, size=L, replace=False) for L in p_lens]
    return a_rows, b_rows, p_rows


REGIMES = ("int", "uniform")


@pytest.mark.parametrize("mode", (0, 1))
def test_degenerate_shapes(mode, dev):
    # nnz_P = 0
    a_rows, b_rows = [[0, 1], [1], []], [[0], [0, 1]]
    if mode == 1:
        b_rows = [[0, 1], [1]]
    for regime in REGIMES:
        got, _ = _check_product(mode, a_rows, b_rows, [[], [], []], (3, 2, 2), 2, regime, dev)
        assert got.shape == (2, 0)
        # n = 1
        _check_product(mode, [[1, 0]] if mode == 0 else [[0, 1]], b_rows, [[1, 0]], (1, 2, 2), 1,
                       regime, dev)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", (0, 1))
def test_empty_rows_unreached_entries_and_repeats(mode, regime, dev):
    """Empty P rows between non-empty ones, an empty walked row, a P entry nothing reaches
    (exactly 0.0, never unwritten) and a walked row that repeats an id, out of order."""
    if mode == 0:   # A [5, 4] walked, B [4, 6] searched
        a_rows = [[3, 1, 3, 0], [], [2], [0, 0, 0], [1]]
        b_rows = [[0, 2, 5], [1, 2], [], [2, 4]]
        p_rows = [[5, 2, 0, 3], [], [1, 0], [], [2, 1, 5]]   # row 2: B's row 2 is empty
    else:           # A [5, 4] searched, B [6, 4] walked
        a_rows = [[0, 1, 3], [], [2], [0, 3], [1]]
        b_rows = [[3, 1, 3, 0], [], [2, 2], [0, 0, 0], [1], [3, 2, 1, 0, 3]]
        p_rows = [[5, 2, 0, 3], [], [1, 0, 2], [], [2, 4, 5]]  # col 1: B's row 1 is empty
    _check_product(mode, a_rows, b_rows, p_rows, (5, 4, 6), 3, regime, dev)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", (0, 1))
def test_search_positions(mode, regime, dev):
    """Searched rows of 1, 2, 63, 64 and 65 ids (even ids 2, 4, ..., 2 L) with the key first,
    last, absent below, absent above and absent inside."""
    lens = (1, 2, 63, 64, 65)
    width = 2 * 65 + 2
    searched = [2 * (np.arange(L) + 1) for L in lens]
    probes = [sorted({1, 2, 3, 2 * L, 2 * L + 1, L // 2 * 2 + 2}) for L in lens]
    t = len(lens)
    if mode == 0:   # A's row i names B's row i; P's row i probes it
        a_rows, b_rows, dims = [[i] for i in range(t)], searched, (t, t, width)
        p_rows = probes
    else:           # A's row i is searched for col_B of B's row s = [s]; P's row i probes it
        a_rows, b_rows, dims = searched, [[s] for s in range(width)], (t, width, width)
        p_rows = probes
    got, want = _check_product(mode, a_rows, b_rows, p_rows, dims, 2, regime, dev)
    assert (want != 0).sum() > 0 and (want == 0).sum() > 0


@pytest.mark.parametrize("C", (1, 2, 3, 8))
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", (0, 1))
def test_class_limits_and_channels(mode, regime, C, limits, dev):
    """Walked rows one below, at and one above each class limit (the lane class's longest row,
    one and two chunks of the wave class) and P rows around a wavefront's 64 entries; P is a
    strict subset of the full product pattern plus entries nothing reaches."""
    lane_max, chunk = limits
    rng = np.random.default_rng(100 * mode + C)
    walked = [lane_max - 1, lane_max, lane_max + 1, chunk - 1, chunk, chunk + 1,
              2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 0, 3]
    p_lens = [chunk - 1, chunk, chunk + 1, 5, 0, 2 * chunk + 1, 7, 9, 11, 4, 6]
    n = len(walked)
    k, m = 24, 140
    if mode == 1:     # the walked rows are B's: one per column of P, so m = len(walked)
        p_lens = [n, n - 1, 0, 1, n, 3, n, 2, n, n, n]
        m = n
    a_rows, b_rows, p_rows = _random_case(rng, mode, n, k, m, walked, p_lens)
    got, want = _check_product(mode, a_rows, b_rows, p_rows, (n, k, m), C, regime, dev,
                               seed=C)
    assert (want != 0).any()


def test_many_waves_and_grid_stride(dev):
    """P with more entries than one workgroup takes, rows of every class mixed."""
    rng = np.random.default_rng(9)
    n, k, m = 40, 50, 300
    walked = rng.integers(0, 80, size=n)
    a_rows, b_rows, p_rows = _random_case(rng, 0, n, k, m, walked, rng.integers(0, 200, size=n))
    _check_product(0, a_rows, b_rows, p_rows, (n, k, m), 2, "int", dev)


@pytest.mark.parametrize("mode", (0, 1))
def test_malformed_operands_are_refused_and_the_next_call_works(mode, dev):
    rng = np.random.default_rng(1)
    good_s = [[0, 2, 3], [1], [0, 3]]                  # the searched operand, [3, 4]
    walked = [[2, 0], [1, 1], [0], [2]]                # the walked operand
    if mode == 0:   # A [4, 3] walked, B [3, 4] searched, P [4, 4]
        dims, p_rows = (4, 3, 4), [[0, 3], [1], [2, 0], [3]]
    else:           # A [3, 4] searched, B [m, k] = [4, 4] walked
        dims, p_rows = (3, 4, 4), [[0, 3], [1], [2, 0]]
    p = _csr(p_rows, 4, dev)

    def build(s):
        if mode == 0:
            return _csr(walked, 3, dev), _csr(s, 4, dev)
        return _csr(s, 4, dev), _csr(walked, 4, dev)

    def call(s):
        a, b = build(s)
        av, bv = _values(rng, "int", 2, a.nnz), _values(rng, "int", 2, b.nnz)
        return _call_product(mode, a, av, b, bv, p, dims, 2, dev)[0]

    assert call(good_s) == 0
    assert call([[0, 3, 2], [1], [0, 3]]) == E_ARG     # not ascending
    assert call([[0, 2, 2], [1], [0, 3]]) == E_ARG     # not strictly
    assert call([[0, 2, 4], [1], [0, 3]]) == E_ARG     # id out of range
    assert call([[0, 2, -1], [1], [0, 3]]) == E_ARG
    assert call(good_s) == 0
    # a broken rowptr of P
    a, b = build(good_s)
    bad = _csr(p_rows, 4, dev)
    bad.rowptr[1] = 9
    av, bv = _values(rng, "int", 2, a.nnz), _values(rng, "int", 2, b.nnz)
    assert _call_product(mode, a, av, b, bv, bad, dims, 2, dev)[0] == E_ARG
    assert call(good_s) == 0


# ------------------------------------------------------------------- aggregate, dot, rowsum
EDGE_ROWS = (0, 1, 64, 65, 3, 0)                         # edges per row
N_COLS = 70


@pytest.fixture(scope="module")
def edge_graph(dev):
    rng = np.random.default_rng(3)
    rows = [rng.choice(N_COLS, size=L, replace=False) for L in EDGE_ROWS]
    for r in (1, 2, 3):                                  # a diagonal entry in these rows
        if r not in rows[r]:
            rows[r][0] = r
    return rows, _csr(rows, N_COLS, dev)


def _edge_dense(rows, v, skip_diag):
    d = _dense(rows, N_COLS, v)
    if skip_diag:
        for r in range(len(rows)):
            d[:, r, r] = 0
    return d


@pytest.mark.parametrize("C", (1, 2, 3))
@pytest.mark.parametrize("F", (4, 8, 64, 68))
@pytest.mark.parametrize("regime", REGIMES)
def test_edge_aggregate(regime, F, C, edge_graph, dev):
    from graphneuralnetwork_amd import _lib
    rows, g = edge_graph
    n = len(rows)
    rng = np.random.default_rng(F + C)
    v = _values(rng, regime, C, g.nnz)
    for per_channel in (False, True):
        x = _values(rng, regime, C * N_COLS if per_channel else N_COLS, F).reshape(
            (C, N_COLS, F) if per_channel else (N_COLS, F))
        for skip in (0, 1):
            y = torch.full((C * n * F + GUARD,), float("nan"), device=dev)
            vd, xd = torch.from_numpy(v).to(dev), torch.from_numpy(x).to(dev)
            _lib.run("gnn_edge_aggregate_f32", rowptr=g.rowptr.data_ptr(), col=g.col.data_ptr(),
                     val=vd.data_ptr(), nnz=g.nnz, n_rows=n, n_cols=N_COLS, X=xd.data_ptr(),
                     ldx=F, x_stride=N_COLS if per_channel else 0, Y=y.data_ptr(), ldy=F, F=F,
                     C=C, skip_diag=skip, stream=_lib.stream_handle(dev))
            torch.cuda.synchronize(dev)
            assert bool(torch.isnan(y[C * n * F:]).all())
            got = y[:C * n * F].view(C, n, F).cpu().numpy()
            want = _edge_dense(rows, v, skip) @ x.astype(np.float64)
            if regime == "int":
                np.testing.assert_array_equal(got, want.astype(np.float32))
            else:
                K = np.array(EDGE_ROWS)[None, :, None]
                assert (np.abs(got - want) <= (K + 1) * EPS * want).all()


@pytest.mark.parametrize("C", (1, 2, 3))
@pytest.mark.parametrize("F", (4, 8, 64, 68))
@pytest.mark.parametrize("regime", REGIMES)
def test_edge_dot(regime, F, C, edge_graph, dev):
    from graphneuralnetwork_amd import _lib
    rows, g = edge_graph
    n = len(rows)
    rng = np.random.default_rng(7 * F + C)
    grad = _values(rng, regime, C * n, F).reshape(C, n, F)
    x = _values(rng, regime, N_COLS, F)
    prow = np.repeat(np.arange(n), EDGE_ROWS)
    pcol = g.col.cpu().numpy().astype(np.int64)
    for skip in (0, 1):
        dv = torch.full((C * g.nnz + GUARD,), float("nan"), device=dev)
        gd, xd = torch.from_numpy(grad).to(dev), torch.from_numpy(x).to(dev)
        _lib.run("gnn_edge_dot_f32", rowptr=g.rowptr.data_ptr(), col=g.col.data_ptr(),
                 nnz=g.nnz, n_rows=n, n_cols=N_COLS, G=gd.data_ptr(), ldg=F, X=xd.data_ptr(),
                 ldx=F, dv=dv.data_ptr(), F=F, C=C, skip_diag=skip,
                 stream=_lib.stream_handle(dev))
        torch.cuda.synchronize(dev)
        assert bool(torch.isnan(dv[C * g.nnz:]).all())
        got = dv[:C * g.nnz].view(C, g.nnz).cpu().numpy()
        assert not np.isnan(got).any()
        want = (grad.astype(np.float64) @ x.astype(np.float64).T)[:, prow, pcol]
        if skip:
            want = want * (prow != pcol)
        if regime == "int":
            np.testing.assert_array_equal(got, want.astype(np.float32))
        else:
            assert (np.abs(got - want) <= (F + 1) * EPS * want).all()


@pytest.mark.parametrize("regime", REGIMES)
def test_edge_rowsum_and_ops_wrappers(regime, edge_graph, dev):
    """gnn_edge_rowsum_f32, and the ops wrappers of all four entries against their torch
    restatements (which tests/test_gtn_cpu.py pins to dense float64)."""
    from graphneuralnetwork_amd import ops
    rows, g = edge_graph
    rng = np.random.default_rng(11)
    C, F = 3, 8
    v = torch.from_numpy(_values(rng, regime, C, g.nnz)).to(dev)
    x = torch.from_numpy(_values(rng, regime, N_COLS, F)).to(dev)
    grad = torch.from_numpy(_values(rng, regime, C * len(rows), F)).to(dev).view(C, -1, F)
    for skip in (False, True):
        got = ops.edge_rowsum(g, v, skip).cpu().numpy()
        want = _edge_dense(rows, v.cpu().numpy(), skip).sum(2)
        if regime == "int":
            np.testing.assert_array_equal(got, want.astype(np.float32))
        else:
            K = np.array(EDGE_ROWS)[None]
            assert (np.abs(got - want) <= (K + 1) * EPS * want).all()
        torch.testing.assert_close(ops.edge_aggregate(g, v, x, skip),
                                   ops.edge_aggregate_torch(g, v, x, skip))
        torch.testing.assert_close(ops.edge_dot(g, grad, x, skip),
                                   ops.edge_dot_torch(g, grad, x, skip))
    # F outside the kernels' set runs the restatement, not an error
    x6 = torch.ones((N_COLS, 6), device=dev)
    assert ops.edge_aggregate(g, v, x6).shape == (C, len(rows), 6)


def test_unsupported_shapes_are_refused(dev):
    from graphneuralnetwork_amd import _lib
    lib = _lib.load()
    assert lib.gnn_masked_product_workspace_bytes(1, 1, 1, 0, 0, 0, 9) == -3
    assert lib.gnn_masked_product_workspace_bytes(1, 1, 1, 0, 0, 0, 0) == -3
    assert lib.gnn_masked_product_workspace_bytes(-1, 1, 1, 0, 0, 0, 1) == -1
    for F in (0, 2, 6, 260):
        assert lib.gnn_edge_aggregate_f32(None, None, None, 0, 1, 1, None, 8, 0, None, 8, F, 1,
                                          0, None) == -3
        assert lib.gnn_edge_dot_f32(None, None, 0, 1, 1, None, 8, None, 8, None, F, 1, 0,
                                    None) == -3
