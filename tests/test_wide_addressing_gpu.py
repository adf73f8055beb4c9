"""64-bit addressing of the row kernels on operands past 2^31 elements.

Three thresholds at which a narrow index wraps: B1 = 2^31 bytes (a signed 32-bit byte offset),
B2 = 2^32 bytes (an unsigned one), B3 = 2^31 elements (an ``int`` element index). Every entry
below runs on the smallest operand that passes all three with 64 rows to spare.

Method. The big operand is zero-filled by a memset; only the rows ``probe_rows`` names carry
data (multiples of 1/4 below 32: exact in bf16, distinct per row): rows 0 and 1, the three rows
around each threshold and the last two. A wrapped address then reads zeros or another probe's
row (the row at B2 aliases row 0, a probe itself; tests/test_wide_addressing_cpu.py proves the
aliases differ for every layout used here). Large outputs are pre-filled with NaN and the rows
that changed are counted: a store at a wrapped address changes a row nobody asked for.
References: selections (gathers, MAXPOOL values, argmax indices) bit for bit against
oracle.c_oracle / oracle.gnn_oracle on the compacted probe rows, and bit for bit against the
same op on a compact copy with remapped indices; sums and products against float64 over the
nonzero rows with the comparison of the op's own test module (``close`` at RTOL = 1e-4 of
test_spmm_gpu, ``close_sum`` of test_sage_train_gpu, ``_close`` of test_sage_score_gpu).
No test skips: too little free device memory fails with the figure.

Persistent (module fixtures): the fp32 buffer (8 GiB + 2.3 MiB) and the bf16 table (4 GiB).
Peak = persistent 12 GiB + what the test adds.

entry                                   dtype      passes      adds            peak
--------------------------------------  ---------  ----------  --------------  -------
sage_gather_aggregate (+ live)          f32, bf16  B1 B2 B3    < 1 MiB         12 GiB
sage_gather_concat (+ live)             f32, bf16  B1 B2 B3    < 1 MiB         12 GiB
sage_gather_concat_arg / _aggregate_arg f32, bf16  B1 B2 B3    < 1 MiB         12 GiB
sage_layer                              f32        B1 B2 B3    < 1 MiB         12 GiB
gather_rows / permute_rows / dropout    f32, bf16  B1 B2 B3    < 1 MiB         12 GiB
sage_scatter_concat (+ _maxpool)        f32        B1 B2 B3    arg 256 MiB     12.3 GiB
sage_scatter_agg (+ _maxpool)           f32        B1 B2 B3    arg 256 MiB     12.3 GiB
spmm_forward, X side, every path        f32, bf16  B1 B2 B3    < 64 MiB        12 GiB
spmm_forward, Y side (2^24 + 64 rows)   f32        B1 B2 B3    Y 8 GiB         20.5 GiB
gat_aggregate modes 0, 1 (row classes,  f32        B1 B2 B3    er 512 MiB      12.5 GiB
  hub-staged, packed tasks, XCD-sliced)
gcn_transform plain / bias + ReLU       f32        B1 B2 B3    Y 8 GiB         20 GiB
gcn_transform bf16 output               f32->bf16  B1 B2 B3    Y 4 GiB         16 GiB
gcn_transform out_rows                  f32, bf16  B1 B2 B3    Y 8 GiB         20 GiB
gemm_tn wide / narrow / trans, masked   f32        B1 B2 B3    B 8 GiB         20 GiB
linear_small (both kinds)               f32        B1 B2 B3    Y 4 GiB         16 GiB
linear_relu_classify                    f32        B1 B2 B3    Y 8.2 GiB       20.2 GiB
col_mean                                f32        B1 B2 B3    < 1 MiB         12 GiB
gat_project                             f32        B1 B2 B3    Wh 2 GiB + 1    15 GiB
gat_logits vector / scalar              f32        B1 B2 B3    el, er 1 GiB    13 GiB
sage_score / sage_score_backward        f32        B1 B2 B3    dx 8 GiB + 1    21 GiB
bce_logits WIDE and narrow, float y     f32        B1 B2 B3    y 8 + g 8 GiB   29 GiB
bce_logits WIDE and narrow, int64 y     f32, i64   B1 B2 B3    y 16 + g 8 GiB  37 GiB

Out of scope: the GAT backward (six full-size buffers exceed the 40 GiB cap); the switch of
gnn_gat_logits_f32 to its scalar kernel at n * heads >= 2^31 (not reachable below ~34 GB);
graphs of more than 2^31 edges or nodes (the entries decline them, and the CPU C-ABI tests
assert the declines).
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from oracle import c_oracle
from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-4

B1_BYTES = 1 << 31
B2_BYTES = 1 << 32
B3_ELEMS = 1 << 31
SPARE = 64
# (rows, row pitch in elements, element size): the smallest operands past all three thresholds
N32, LD32 = (1 << 24) + SPARE, 128      # the fp32 table
N16, LD16 = (1 << 25) + SPARE, 64       # the bf16 table (B2 and B3 coincide)
MB, LDB = (1 << 21) + SPARE, 1024       # the pitched fp32 gradient buffer of the scatters
LAYOUTS = {"fp32 table": (N32, LD32, 4), "bf16 table": (N16, LD16, 2),
           "pitched gradient buffer": (MB, LDB, 4)}
# bce_logits: rows of BCE_COLS logits at a pitch of BCE_COLS + BCE_PAD, so that an element's
# address depends on the row the kernel's division gives
BCE_COLS, BCE_PAD, BCE_ROWS = 1 << 15, 8, (1 << 16) + 2
BIG32_ELEMS = max(N32 * LD32, MB * LDB, BCE_ROWS * (BCE_COLS + BCE_PAD))
GIB = 1 << 30


# ------------------------------------------------------------------ helpers (pure numpy)
def threshold_rows(ld, elem_size):
    """The first row at or past B1, B2 and B3 for rows of ``ld`` elements."""
    row_bytes = ld * elem_size
    return (-(-B1_BYTES // row_bytes), -(-B2_BYTES // row_bytes), -(-B3_ELEMS // ld))


def probe_rows(n_rows, ld, elem_size):
    """Row 0, row 1, rB - 1, rB, rB + 1 around each of B1, B2, B3 and the last two rows of an
    [n_rows, ld] operand: sorted, distinct int64."""
    rows = {0, 1, n_rows - 2, n_rows - 1}
    for rb in threshold_rows(ld, elem_size):
        rows |= {rb - 1, rb, rb + 1}
    rows = np.array(sorted(rows), np.int64)
    assert rows[0] >= 0 and rows[-1] < n_rows, "the operand does not pass every threshold"
    return rows


def probe_values(n_probes, width, salt=0):
    """float32 [n_probes, width]: multiples of 1/4 in [-31.25, 31.25] (exact in bf16), the rows
    pairwise distinct in every column and none of them zero."""
    assert n_probes < 251
    i = np.arange(n_probes, dtype=np.int64)[:, None]
    f = np.arange(width, dtype=np.int64)[None, :]
    return (((i * 37 + f * 11 + salt * 5) % 251 - 125) / 4.0).astype(np.float32)


def aliases(row, ld, elem_size):
    """The rows a wrapped index reaches instead of ``row``: minus 2^31 bytes, minus 2^32 bytes,
    minus 2^31 elements (those that exist)."""
    row_bytes = ld * elem_size
    assert B1_BYTES % row_bytes == 0 and B3_ELEMS % ld == 0
    cand = (row - B1_BYTES // row_bytes, row - B2_BYTES // row_bytes, row - B3_ELEMS // ld)
    return sorted({a for a in cand if a >= 0})


def close(a, b, rtol=RTOL, what=""):  # test_spmm_gpu.close
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    err = float(np.nanmax(np.abs(a - b))) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale, err_msg=what)


def close_sum(a, b, what=""):  # test_sage_train_gpu.close_sum
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * scale, err_msg=what)


def _close(got, ref, what):  # test_sage_score_gpu._close
    a, b = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=2e-5 * scale, err_msg=what)


# ------------------------------------------------------------------ helpers (device)
def _need(dev, nbytes, what):
    """No skip: a device without the memory fails the test with the figure."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < nbytes + (GIB >> 1):
        pytest.fail(f"{what} needs {nbytes / GIB:.2f} GiB of free device memory "
                    f"(+ 0.5 GiB of slack), found {free / GIB:.2f} GiB")


@contextlib.contextmanager
def planted(view, rows, vals):
    """``view[rows] = vals`` (one small copy per probe row) for the body, zeros again after."""
    vals = torch.as_tensor(vals).to(device=view.device, dtype=view.dtype)
    try:
        for r, v in zip(rows.tolist(), vals):
            view[r].copy_(v)
        yield
    finally:
        for r in rows.tolist():
            view[r].zero_()


def _all_nan_rows(t, step=1 << 20):
    """The number of rows of a 2-D tensor still all NaN (in pieces: no full-size temporary)."""
    left = 0
    for r0 in range(0, t.shape[0], step):
        left += int(torch.isnan(t[r0:r0 + step]).all(1).sum())
    return left


def _fill_rows(c, compact_result, fill):
    """How many rows of a result over the big operand of ``c`` equal ``fill``: every row that is
    no probe, and the probes whose result (the compact run's) happens to equal it."""
    return c.n - c.P + int((compact_result == fill).all(1).sum())


def _rows_equal_to(t, row, step=1 << 20):
    """The number of rows of a 2-D tensor that equal ``row`` bit for bit as values."""
    n = 0
    for r0 in range(0, t.shape[0], step):
        n += int((t[r0:r0 + step] == row).all(1).sum())
    return n


@pytest.fixture(scope="module")
def big32(dev):
    """8 GiB + 2.3 MiB of fp32 zeros: the [N32, 128] table, the [MB, 1024] pitched buffer, the
    pitched logits of bce_logits."""
    _need(dev, BIG32_ELEMS * 4, "the fp32 buffer")
    t = torch.zeros(BIG32_ELEMS, dtype=torch.float32, device=dev)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big16(dev):
    """4 GiB of bf16 zeros: the [N16, 64] table."""
    _need(dev, N16 * LD16 * 2, "the bf16 table")
    t = torch.zeros(N16 * LD16, dtype=torch.bfloat16, device=dev)
    yield t
    del t
    torch.cuda.empty_cache()


def _table32(big32):
    return big32[:N32 * LD32].view(N32, LD32)


def _table16(big16):
    return big16.view(N16, LD16)


class Case:
    """A big table view [n, F] (row pitch ld), its probe rows and their values."""

    def __init__(self, table, F, elem_size):
        self.n, self.ld = table.shape
        self.F = F
        self.table = table[:, :F] if F != self.ld else table
        self.rows = probe_rows(self.n, self.ld, elem_size)
        self.P = self.rows.size
        self.vals = probe_values(self.P, F)
        b1, _, b3 = threshold_rows(self.ld, elem_size)
        self.below_b1 = self.rows[self.rows < b1]
        self.above_b3 = self.rows[self.rows >= b3]
        assert self.below_b1.size >= 3 and self.above_b3.size >= 4

    def compact(self):
        return torch.from_numpy(self.vals).to(device=self.table.device, dtype=self.table.dtype)

    def planted(self):
        return planted(self.table, self.rows, self.vals)

    def index_map(self, M, k, seed=0):
        """[M, k] probe rows. k >= 2: every output row reads a probe below B1 and one at or
        past B3, at columns that move with the row; k = 1: row m reads probe m mod P, so the
        M >= P rows together read every probe."""
        idx = np.empty((M, k), np.int64)
        for m in range(M):
            row = self.rows[(m * 3 + seed + np.arange(k) * 7) % self.P]
            if k >= 2:
                row[0] = self.below_b1[m % self.below_b1.size]
                row[1] = self.above_b3[m % self.above_b3.size]
                row = np.roll(row, m)
            idx[m] = row
        return idx

    def remap(self, idx):
        c = np.searchsorted(self.rows, idx)
        assert np.array_equal(self.rows[c], idx)
        return c


def _case(dtype, F, big32, big16):
    if dtype == "f32":
        return Case(_table32(big32), F, 4)
    return Case(_table16(big16), F, 2)


# (dtype, F): the full row and an 8-wide column slice of it (same pitch)
GATHER_SHAPES = [("f32", 128), ("f32", 8), ("bf16", 64), ("bf16", 8)]
M_GATHER = 64


def _dev_idx(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ A. row gathers
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dtype,F", GATHER_SHAPES)
def test_gather_aggregate(dev, big32, big16, dtype, F, k):
    """sage_gather_aggregate MEAN / MAX / MAXPOOL and the live form over probe rows on both
    sides of every threshold. Peak: the persistent 12 GiB."""
    from graphneuralnetwork_amd import ops
    c = _case(dtype, F, big32, big16)
    idx = c.index_map(M_GATHER, k)
    cidx = c.remap(idx)
    if k >= 2:
        assert ((idx[:, :, None] == c.below_b1).any(2).any(1)
                & (idx[:, :, None] == c.above_b3).any(2).any(1)).all()
    else:
        assert np.unique(idx).size == c.P
    it, ct = _dev_idx(idx, dev), _dev_idx(cidx, dev)
    small = c.compact()
    with c.planted():
        for agg in ("MEAN", "MAX", "MAXPOOL"):
            got = ops.sage_gather_aggregate(c.table, it, agg)
            same = ops.sage_gather_aggregate(small, ct, agg)
            assert torch.equal(got, same), f"{agg}: the big table and its compact copy differ"
            g = got.cpu().numpy()
            if agg == "MAX":
                assert g.dtype == np.int64
                assert np.array_equal(g, c_oracle.sage_argmax(c.vals, cidx))
                assert np.array_equal(g, O.sage_gather_aggregate(c.vals, cidx, "MAX"))
            elif agg == "MAXPOOL":
                assert np.array_equal(g, c_oracle.sage_gather(c.vals, cidx, "MAXPOOL"))
                assert np.array_equal(g.astype(np.float64),
                                      O.sage_gather_aggregate(c.vals, cidx, "MAXPOOL"))
            else:
                close(g, O.sage_gather_aggregate(c.vals, cidx, "MEAN"), what=f"MEAN k={k}")
                close(g, c_oracle.sage_gather(c.vals, cidx, "MEAN"), what=f"MEAN k={k} (C)")
        live = torch.tensor([M_GATHER - 5], device=dev)
        for agg in ("MEAN", "MAXPOOL"):
            full = ops.sage_gather_aggregate(c.table, it, agg)
            out = torch.full((M_GATHER, F), float("nan"), device=dev)
            assert ops.sage_gather_aggregate(c.table, it, agg, out=out, live=live) is out
            assert torch.equal(out[:M_GATHER - 5], full[:M_GATHER - 5])
            assert bool(torch.isnan(out[M_GATHER - 5:]).all())


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dtype,F", GATHER_SHAPES)
def test_gather_concat(dev, big32, big16, dtype, F, k):
    """sage_gather_concat in its four modes, into a pitched ``out`` view and through the live
    form: centre rows and neighbour rows both on every side of the thresholds. Peak: 12 GiB."""
    from graphneuralnetwork_amd import ops
    c = _case(dtype, F, big32, big16)
    idx = c.index_map(M_GATHER, k)
    sidx = c.index_map(M_GATHER, 1, seed=7)[:, 0]
    assert (sidx >= c.above_b3[0]).any() and (sidx < c.below_b1[-1] + 1).any()
    cidx, csidx = c.remap(idx), c.remap(sidx)
    it, st = _dev_idx(idx, dev), _dev_idx(sidx, dev)
    ct, cst = _dev_idx(cidx, dev), _dev_idx(csidx, dev)
    small = c.compact()
    with c.planted():
        for agg in ("MEAN", "SUM", "MAXPOOL", "MAX"):
            got = ops.sage_gather_concat(c.table, st, it, agg)
            same = ops.sage_gather_concat(small, cst, ct, agg)
            assert got.shape == (M_GATHER, 2 * F) and got.dtype == torch.float32
            assert torch.equal(got, same), f"{agg}: the big table and its compact copy differ"
            g = got.cpu().numpy()
            assert np.array_equal(g[:, :F], c.vals[csidx]), f"{agg}: centre rows"
            nb = c.vals[cidx]
            if agg == "MAX":
                assert np.array_equal(g[:, F:], c_oracle.sage_argmax(c.vals, cidx)
                                      .astype(np.float32))
            elif agg == "MAXPOOL":
                assert np.array_equal(g[:, F:], c_oracle.sage_gather(c.vals, cidx, "MAXPOOL"))
            elif agg == "SUM":
                close(g[:, F:], nb.astype(np.float64).sum(1), what=f"SUM k={k}")
            else:
                close(g[:, F:], O.sage_gather_aggregate(c.vals, cidx, "MEAN"),
                      what=f"MEAN k={k}")
            # a pitched out view, and the live form (rows past the count left as they were)
            wide = torch.full((M_GATHER, 2 * F + 8), float("nan"), device=dev)
            out = wide[:, 4:4 + 2 * F]
            assert ops.sage_gather_concat(c.table, st, it, agg, out=out) is out
            assert torch.equal(out, got) and bool(torch.isnan(wide[:, :4]).all())
            assert bool(torch.isnan(wide[:, 4 + 2 * F:]).all())
            live = torch.tensor([M_GATHER - 9], device=dev)
            pend = torch.full((M_GATHER, 2 * F), float("nan"), device=dev)
            ops.sage_gather_concat(c.table, st, it, agg, out=pend, live=live)
            assert torch.equal(pend[:M_GATHER - 9], got[:M_GATHER - 9])
            assert bool(torch.isnan(pend[M_GATHER - 9:]).all())


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dtype,F", GATHER_SHAPES)
def test_gather_arg(dev, big32, big16, dtype, F, k):
    """sage_gather_concat_arg / sage_gather_aggregate_arg: the winner bytes are torch.argmax's
    (the C oracle's), the value is the table's AT that byte. Peak: 12 GiB."""
    from graphneuralnetwork_amd import ops
    c = _case(dtype, F, big32, big16)
    idx = c.index_map(M_GATHER, k)
    sidx = c.index_map(M_GATHER, 1, seed=3)[:, 0]
    cidx, csidx = c.remap(idx), c.remap(sidx)
    it, st = _dev_idx(idx, dev), _dev_idx(sidx, dev)
    ct, cst = _dev_idx(cidx, dev), _dev_idx(csidx, dev)
    small = c.compact()
    want_arg = c_oracle.sage_argmax(c.vals, cidx)
    assert np.array_equal(want_arg, O.sage_gather_aggregate(c.vals, cidx, "MAX"))
    want_val = np.take_along_axis(c.vals[cidx], want_arg[:, None, :], 1)[:, 0]
    with c.planted():
        res, ref = ops.sage_gather_concat_arg(c.table, st, it), \
            ops.sage_gather_concat_arg(small, cst, ct)
        assert res is not None and ref is not None
        (buf, arg), (buf_c, arg_c) = res, ref
        assert torch.equal(buf, buf_c) and torch.equal(arg, arg_c)
        assert arg.dtype == torch.uint8
        assert np.array_equal(arg.cpu().numpy(), want_arg.astype(np.uint8))
        b = buf.cpu().numpy()
        assert np.array_equal(b[:, :F], c.vals[csidx]) and np.array_equal(b[:, F:], want_val)
        res, ref = ops.sage_gather_aggregate_arg(c.table, it), \
            ops.sage_gather_aggregate_arg(small, ct)
        assert res is not None and ref is not None
        (out, arg), (out_c, arg_c) = res, ref
        assert torch.equal(out, out_c) and torch.equal(arg, arg_c)
        assert np.array_equal(arg.cpu().numpy(), want_arg.astype(np.uint8))
        assert np.array_equal(out.cpu().numpy(), want_val)


@pytest.mark.parametrize("k", [1, 10])
def test_fused_sage_layer(dev, big32, k, monkeypatch):
    """sage_layer (F = 128, H = 128): the neighbour rows and the centre rows -- through an index
    and as the last rows of the table itself -- past B3. Peak: 12 GiB."""
    from graphneuralnetwork_amd import ops
    monkeypatch.setattr(ops, "SAGE_FUSED_MIN_ROWS", 1)
    c = Case(_table32(big32), 128, 4)
    H, M = 128, M_GATHER
    idx = c.index_map(M, k)
    sidx = c.index_map(M, 1, seed=7)[:, 0]
    cidx, csidx = c.remap(idx), c.remap(sidx)
    W = (np.random.default_rng(k).standard_normal((H, 256)) * 0.1).astype(np.float32)
    Wd = torch.from_numpy(W).to(dev)
    small = c.compact()
    agg = c.vals[cidx].astype(np.float64).mean(1)
    with c.planted():
        got = ops.sage_layer(c.table, _dev_idx(idx, dev), Wd, c.table, _dev_idx(sidx, dev))
        same = ops.sage_layer(small, _dev_idx(cidx, dev), Wd, small, _dev_idx(csidx, dev))
        assert got is not None and same is not None and torch.equal(got, same)
        ref = np.maximum(np.concatenate([c.vals[csidx], agg], 1) @ W.T.astype(np.float64), 0)
        close(got.cpu().numpy(), ref, what=f"sage_layer k={k} (indexed centre)")
        # no centre index: the centre rows are the table's last M rows, all past B3 and zero
        # except the four probes among them
        tail = c.table[c.n - M:]
        got = ops.sage_layer(c.table, _dev_idx(idx, dev), Wd, tail)
        assert got is not None
        selfm = np.zeros((M, 128), np.float32)
        inside = c.rows >= c.n - M
        selfm[c.rows[inside] - (c.n - M)] = c.vals[inside]
        assert inside.sum() == 4
        ref = np.maximum(np.concatenate([selfm, agg], 1) @ W.T.astype(np.float64), 0)
        close(got.cpu().numpy(), ref, what=f"sage_layer k={k} (centre rows in place)")


@pytest.mark.parametrize("dtype,F", GATHER_SHAPES)
def test_gather_rows_permute_and_dropout(dev, big32, big16, dtype, F):
    """gather_rows in every dtype pairing, permute_rows and dropout_rows with ``idx``: exact
    copies (dropout: of the kept elements, by the oracle's hash). Peak: 12 GiB."""
    from graphneuralnetwork_amd import ops
    c = _case(dtype, F, big32, big16)
    rows = np.concatenate([c.rows, c.rows[::-1], c.rows[::2]])
    crow = c.remap(rows)
    rt = _dev_idx(rows, dev)
    want = c.vals[crow]
    with c.planted():
        got = ops.gather_rows(c.table, rt)
        assert got.dtype == c.table.dtype
        assert np.array_equal(got.float().cpu().numpy(), want)
        if dtype == "bf16":
            out = torch.full((rows.size, F), float("nan"), device=dev)
            assert ops.gather_rows(c.table, rt, out=out) is out
            assert np.array_equal(out.cpu().numpy(), want)
            return
        assert np.array_equal(ops.permute_rows(c.table, rt).cpu().numpy(), want)
        p, seed = 0.5, 1234  # scale 2: the kept values are exact
        cols = np.arange(F)[None, :]
        for by_source, keys in ((False, np.arange(rows.size)), (True, rows)):
            got = ops.dropout_rows(c.table, p, seed, rt, key_by_source=by_source).cpu().numpy()
            keep = c_oracle.dropout_keep(seed, keys[:, None], cols, p)
            assert 0.3 < keep.mean() < 0.7
            assert np.array_equal(got, np.where(keep, want * 2.0, want * 0.0)), by_source


# ------------------------------------------------------------------ B. adjoint scatters
N_PREV = 16


def _scatter_case(big32, F):
    """The pitched gradient buffer [MB, 2F] (pitch 1024 floats: row 2^21 is element 2^31), its
    probes and the maps: every row feeds target m mod 8 (zeros), the probes around B1 / B2 / B3
    feed targets 11 / 12 / 13 alone, rows 0 and 1 target 14, the last two rows target 15."""
    dbuf = big32[:MB * LDB].view(MB, LDB)
    rows = probe_rows(MB, LDB, 4)
    b1, b2, b3 = threshold_rows(LDB, 4)
    tgt = np.empty(rows.size, np.int64)
    for i, r in enumerate(rows.tolist()):
        tgt[i] = (14 if r < 2 else 15 if r >= MB - 2 else
                  11 if abs(r - b1) <= 1 else 12 if abs(r - b2) <= 1 else 13)
    assert np.array_equal(np.unique(tgt), [11, 12, 13, 14, 15])
    return dbuf, rows, tgt


def _scatter_maps(dev, rows, tgt):
    m = torch.arange(MB, device=dev) % 8
    m[_dev_idx(rows, dev)] = _dev_idx(tgt, dev)
    return m


@pytest.mark.parametrize("F", [128, 8])
def test_scatter_concat_and_maxpool(dev, big32, F):
    """sage_scatter_concat and sage_scatter_concat_maxpool over a gradient buffer whose rows pass
    B1, B2 and B3 (k = 1, n_prev = 16). Peak: 12 GiB + the 256 MiB arg bytes."""
    from graphneuralnetwork_amd import ops
    dbuf, rows, tgt = _scatter_case(big32, F)
    view = dbuf[:, :2 * F]
    vals = probe_values(rows.size, 2 * F)
    m = _scatter_maps(dev, rows, tgt)
    tr = ops.sage_maps_transpose(m, m.view(MB, 1), N_PREV, check=False)
    assert tr is not None
    argv = ((np.arange(rows.size)[:, None] + np.arange(F)[None, :]) % 2).astype(np.uint8)
    arg = torch.zeros((MB, F), dtype=torch.uint8, device=dev)
    arg[_dev_idx(rows, dev)] = torch.from_numpy(argv).to(dev)
    v64 = vals.astype(np.float64)
    want = np.zeros((N_PREV, F))
    want_mp = np.zeros((N_PREV, F))
    for i, t in enumerate(tgt):
        want[t] += v64[i, :F] + v64[i, F:]  # k = 1: the neighbour half is not scaled
        want_mp[t] += v64[i, :F] + np.where(argv[i] == 0, v64[i, F:], 0.0)
    with planted(view, rows, vals):
        out = torch.full((N_PREV, F), float("nan"), device=dev)
        assert ops.sage_scatter_concat(view, tr, N_PREV, out=out) is out
        close_sum(out.cpu().numpy(), want, f"scatter_concat F={F}")
        out = torch.full((N_PREV, F), float("nan"), device=dev)
        assert ops.sage_scatter_concat_maxpool(view, arg, tr, N_PREV, out=out) is out
        close_sum(out.cpu().numpy(), want_mp, f"scatter_concat_maxpool F={F}")


@pytest.mark.parametrize("F", [128, 8])
def test_scatter_agg_and_maxpool(dev, big32, F):
    """sage_scatter_agg and sage_scatter_agg_maxpool (the gcn-mode layer: no centre half) over
    the same pitched buffer. Peak: 12 GiB + the 256 MiB arg bytes."""
    from graphneuralnetwork_amd import ops
    dbuf, rows, tgt = _scatter_case(big32, F)
    view = dbuf[:, :F]
    vals = probe_values(rows.size, F, salt=1)
    m = _scatter_maps(dev, rows, tgt)
    tr = ops.sage_maps_transpose_nbr(m.view(MB, 1), N_PREV, check=False)
    assert tr is not None
    argv = ((np.arange(rows.size)[:, None] + np.arange(F)[None, :]) % 2).astype(np.uint8)
    arg = torch.zeros((MB, F), dtype=torch.uint8, device=dev)
    arg[_dev_idx(rows, dev)] = torch.from_numpy(argv).to(dev)
    v64 = vals.astype(np.float64)
    want = np.zeros((N_PREV, F))
    want_mp = np.zeros((N_PREV, F))
    for i, t in enumerate(tgt):
        want[t] += v64[i]
        want_mp[t] += np.where(argv[i] == 0, v64[i], 0.0)
    with planted(view, rows, vals):
        out = torch.full((N_PREV, F), float("nan"), device=dev)
        assert ops.sage_scatter_agg(view, tr, N_PREV, out=out) is out
        close_sum(out.cpu().numpy(), want, f"scatter_agg F={F}")
        out = torch.full((N_PREV, F), float("nan"), device=dev)
        assert ops.sage_scatter_agg_maxpool(view, arg, tr, N_PREV, out=out) is out
        close_sum(out.cpu().numpy(), want_mp, f"scatter_agg_maxpool F={F}")


# ------------------------------------------------------------------ C. CSR gathers
N_CSR_ROWS = 2048


def _csr(dev, rowptr, col, val, n_cols):
    from graphneuralnetwork_amd.graph import CsrGraph
    return CsrGraph(torch.as_tensor(rowptr, dtype=torch.int64, device=dev),
                    torch.as_tensor(col, dtype=torch.int32, device=dev),
                    torch.as_tensor(val, dtype=torch.float32, device=dev),
                    len(rowptr) - 1, n_cols)


def _probe_graph(c, seed, long_row=600, empty_row=True):
    """[2048, n] CSR over the probe columns: row 0 has ``long_row`` edges cycling through all
    probes (cut into segments whose columns straddle B3), row 1 none (``empty_row``), row 2 one,
    the others 2-40; the probes at or past B3 are referenced most (they become the hub rows)."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(2, 41, N_CSR_ROWS)
    deg[0], deg[1], deg[2] = long_row, 0 if empty_row else 3, 1
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nnz = int(rowptr[-1])
    w = np.where(np.isin(c.rows, c.above_b3), 6.0, 1.0)
    pick = rng.choice(c.P, nnz, p=w / w.sum())
    pick[:long_row] = np.arange(long_row) % c.P
    val = (rng.integers(-8, 9, nnz) / 4.0).astype(np.float32)
    return rowptr, c.rows[pick], pick.astype(np.int64), val


@pytest.mark.parametrize("dtype,F", [("f32", 128), ("bf16", 64)])
def test_spmm_gathers_past_b3(dev, big32, big16, dtype, F, monkeypatch):
    """spmm_forward over a rectangular graph whose columns are the probes of the big X: the
    per-row kernels, the packed tasks, the hub-staged forms (hub ids past B3) and the XCD-sliced
    form, with a long row cut into segments. Peak: 12 GiB (+ plans and partials < 64 MiB)."""
    from graphneuralnetwork_amd import ops
    c = _case(dtype, F, big32, big16)
    rowptr, col, ccol, val = _probe_graph(c, 11)
    g = _csr(dev, rowptr, col, val, c.n)
    gc = _csr(dev, rowptr, ccol, val, c.P)
    bias = (np.arange(F) % 7 - 3).astype(np.float32) / 4
    bd = torch.from_numpy(bias).to(dev)
    ref = O.spmm_csr(rowptr, ccol, val, c.vals, bias)
    small = c.compact()
    with c.planted():
        hp = g.hub_plan(4)
        assert int(hp.hub_ids.min()) >= int(c.above_b3[0])  # the staged rows lie past B3
        monkeypatch.setattr(ops, "SPMM_TASKS", False)
        plain = ops.spmm_forward(g, c.table, bd, seg_len=64, hubs=0)
        assert g.plan(64).n_seg >= 9
        close(plain.cpu().numpy(), ref, what="per-row kernels")
        assert torch.equal(plain, ops.spmm_forward(gc, small, bd, seg_len=64, hubs=0))
        assert torch.equal(plain, ops.spmm_forward(g, c.table, bd, seg_len=64, hubs=4))
        monkeypatch.setattr(ops, "SPMM_TASKS", True)
        tasks = ops.spmm_forward(g, c.table, bd, seg_len=64, hubs=0)
        close(tasks.cpu().numpy(), ref, what="packed tasks")
        assert torch.equal(tasks, ops.spmm_forward(gc, small, bd, seg_len=64, hubs=0))
        assert torch.equal(tasks, ops.spmm_forward(g, c.table, bd, seg_len=64, hubs=4))
        assert torch.equal(tasks, ops.spmm_forward(g, c.table, bd, seg_len=64))  # the default
        if dtype == "f32":  # bf16 has the XCD form on degree-ordered graphs only
            monkeypatch.setattr(ops, "XCD_MIN_DEG", 4)
            y = ops.spmm_forward(g, c.table, bd, seg_len=64, hubs=8, xcd=True)
            assert any(isinstance(key, tuple) and key[0] == "_xcd" and p is not None
                       for key, p in g._plans.items())
            close(y.cpu().numpy(), ref, what="XCD-sliced")


def test_spmm_writes_every_row_of_a_big_result(dev, big32):
    """spmm_forward with 2^24 + 64 rows, all empty but the probe rows, into a NaN-filled Y:
    every row is stored (bias for the empty ones), none twice at a wrapped address.
    Peak: 12 GiB + Y 8 GiB + rowptr and plans < 0.5 GiB."""
    from graphneuralnetwork_amd import ops
    F, nx = 128, 32
    _need(dev, N32 * F * 4 + (GIB >> 1), "the [2^24 + 64, 128] result")
    rows = probe_rows(N32, F, 4)
    rng = np.random.default_rng(3)
    deg = np.zeros(N32, np.int64)
    deg[rows] = rng.integers(1, 9, rows.size)
    deg[rows[-1]] = 300  # one long row at the very end
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nnz = int(rowptr[-1])
    col = rng.integers(0, nx, nnz)
    val = (rng.integers(-8, 9, nnz) / 4.0).astype(np.float32)
    X = probe_values(nx, F, salt=2)
    bias = (np.arange(F) % 5 + 1).astype(np.float32) / 4  # nonzero: an empty row is not zeros
    g = _csr(dev, rowptr, col, val, nx)
    bd = torch.from_numpy(bias).to(dev)
    out = torch.empty((N32, F), device=dev)
    out.fill_(float("nan"))
    assert ops.spmm_forward(g, torch.from_numpy(X).to(dev), bd, seg_len=64, out=out) is out
    assert _all_nan_rows(out) == 0
    sub = np.concatenate([[0], np.cumsum(deg[rows])]).astype(np.int64)
    ref = O.spmm_csr(sub, col, val, X, bias)
    got = out[_dev_idx(rows, dev)].cpu().numpy()
    close(got, ref, what="the nonempty rows")
    assert _rows_equal_to(out, bd) == N32 - int((np.abs(got - bias).max(1) > 0).sum())


@pytest.mark.parametrize("mode", [0, 1], ids=["dense", "sparse"])
def test_gat_aggregate_past_b3(dev, big32, mode, monkeypatch):
    """gat_aggregate (8 heads x 16) over the rectangular probe graph: Wh rows and er rows past
    B1 / B2 / B3, through the row-class kernels plain (gnn_gat_csr_f32) and hub-staged
    (gnn_gat_csr_hub_f32), the packed tasks (gnn_gat_csr_tasks_f32, GAT_TASKS) and the
    XCD-sliced form. Not run at size: gnn_gat_csr_ex_f32 (er recomputed from a_dst).
    Peak: 12 GiB + er 512 MiB."""
    from graphneuralnetwork_amd import ops
    assert not ops.GAT_TASKS
    H, fh = 8, 16
    c = Case(_table32(big32), H * fh, 4)
    # no edgeless row (the dense mode's fill is col_mean's business, pinned below)
    rowptr, col, ccol, _ = _probe_graph(c, 13, long_row=300, empty_row=False)
    ones = np.ones(col.size, np.float32)
    g, gc = _csr(dev, rowptr, col, ones, c.n), _csr(dev, rowptr, ccol, ones, c.P)
    erv = probe_values(c.P, H, salt=3) / 16
    elv = (np.random.default_rng(5).integers(-16, 17, (N_CSR_ROWS, H)) / 16.0).astype(np.float32)
    er = torch.zeros((c.n, H), device=dev)
    er[_dev_idx(c.rows, dev)] = torch.from_numpy(erv).to(dev)
    el = torch.from_numpy(elv).to(dev)
    small = c.compact()
    ref = O.gat_csr(rowptr, ccol, c.vals, elv, erv, H, fh, 0.2, mode == 1)
    with c.planted():
        got = ops.gat_aggregate(g, c.table, el, er, H, fh, 0.2, mode)
        close(got.cpu().numpy(), ref, what=f"gat mode {mode}")
        same = ops.gat_aggregate(gc, small, el, torch.from_numpy(erv).to(dev), H, fh, 0.2, mode)
        assert torch.equal(got, same)
        assert torch.equal(got, ops.gat_aggregate(g, c.table, el, er, H, fh, 0.2, mode, hubs=0))
        assert torch.equal(got, ops.gat_aggregate(g, c.table, el, er, H, fh, 0.2, mode, hubs=4))
        monkeypatch.setattr(ops, "GAT_TASKS", True)
        for hubs in (0, 4):
            y = ops.gat_aggregate(g, c.table, el, er, H, fh, 0.2, mode, hubs=hubs)
            close(y.cpu().numpy(), ref, what=f"gat mode {mode}, packed tasks, hubs={hubs}")
        assert any(isinstance(key, tuple) and key[0] == "_tasks" for key in g._plans)
        monkeypatch.setattr(ops, "GAT_TASKS", False)
        monkeypatch.setattr(ops, "XCD_MIN_DEG", 4)
        y = ops.gat_aggregate(g, c.table, el, er, H, fh, 0.2, mode, hubs=8, xcd=True)
        assert any(isinstance(key, tuple) and key[0] == "_xcd" and p is not None
                   for key, p in g._plans.items())
        close(y.cpu().numpy(), ref, what=f"gat mode {mode}, XCD-sliced")


# ------------------------------------------------------------------ D. row-streaming entries
def _weights(dev, fout, k, seed):
    w = (np.random.default_rng(seed).integers(-8, 9, (fout, k)) / 16.0).astype(np.float32)
    return w, torch.from_numpy(w).to(dev)


@pytest.mark.parametrize("form", ["plain", "bias_relu", "bf16out"])
def test_gcn_transform_streams_past_b3(dev, big32, form):
    """gcn_transform over [2^24 + 64, 128] x (zero but the probes) into a NaN-filled result:
    every row stored, the zero rows exactly the epilogue of zeros, the probe rows float64's and
    bit for bit those of the compact run. Peak: 12 GiB + Y 8 GiB (4 GiB as bf16)."""
    from graphneuralnetwork_amd import ops
    c = Case(_table32(big32), 128, 4)
    w, wd = _weights(dev, 128, 128, 1)
    y16 = form == "bf16out"
    _need(dev, c.n * 128 * (2 if y16 else 4), "the transform's result")
    bias = (np.arange(128) % 9 - 4).astype(np.float32) / 4
    kw = dict(relu=True, bias=torch.from_numpy(bias).to(dev)) if form == "bias_relu" else {}
    out = torch.empty((c.n, 128), dtype=torch.bfloat16 if y16 else torch.float32, device=dev)
    out.fill_(float("nan"))
    ref = c.vals.astype(np.float64) @ w.T.astype(np.float64)
    zero_row = np.zeros(128)
    if form == "bias_relu":
        ref, zero_row = np.maximum(ref + bias, 0), np.maximum(bias, 0)
    with c.planted():
        assert ops.gcn_transform(c.table, wd, out=out, **kw) is out
        same = ops.gcn_transform(c.compact(), wd, out_dtype=out.dtype, **kw)
    assert _all_nan_rows(out) == 0
    zr = torch.from_numpy(zero_row).to(device=dev, dtype=out.dtype)
    assert _rows_equal_to(out, zr) == c.n - c.P
    got = out[_dev_idx(c.rows, dev)]
    assert torch.equal(got, same)
    if y16:  # the rounding to bf16 of exactly what the fp32 entry stores
        assert torch.equal(got, ops.gcn_transform(c.compact(), wd).bfloat16())
    else:
        close(got.cpu().numpy(), ref, what=form)


@pytest.mark.parametrize("y16", [False, True], ids=["f32", "bf16out"])
def test_gcn_transform_out_rows_past_b3(dev, big32, y16):
    """gcn_transform(out_rows=): the source rows scattered to the probe rows of a NaN-filled
    [2^24 + 64, 128] result; exactly those rows change. Peak: 12 GiB + Y 8 GiB (4 as bf16)."""
    from graphneuralnetwork_amd import ops
    n = N32
    _need(dev, n * 128 * (2 if y16 else 4), "the transform's result")
    rows = probe_rows(n, 128, 2 if y16 else 4)  # the thresholds of the result's element size
    w, wd = _weights(dev, 128, 128, 2)
    x = probe_values(rows.size, 128, salt=4)
    perm = np.random.default_rng(0).permutation(rows.size)
    out = torch.empty((n, 128), dtype=torch.bfloat16 if y16 else torch.float32, device=dev)
    out.fill_(float("nan"))
    xt = torch.from_numpy(x).to(dev)
    assert ops.gcn_transform(xt, wd, out=out, out_rows=_dev_idx(rows[perm], dev)) is out
    assert _all_nan_rows(out) == n - rows.size
    got = out[_dev_idx(rows[perm], dev)]
    plain = ops.gcn_transform(xt, wd, out_dtype=out.dtype)
    assert torch.equal(got, plain)
    if not y16:
        close(got.cpu().numpy(), x.astype(np.float64) @ w.T.astype(np.float64), what="out_rows")


def _second_operand(dev, c, width, salt):
    """Another zeroed [n, 128] fp32 buffer with its own probe values planted (not re-zeroed:
    the caller drops it)."""
    _need(dev, c.n * LD32 * 4, "the second [2^24 + 64, 128] operand")
    b = torch.zeros((c.n, LD32), device=dev)
    vals = probe_values(c.P, width, salt=salt)
    for r, v in zip(c.rows.tolist(), torch.from_numpy(vals).to(dev)):
        b[r, :width].copy_(v)
    return b, vals


@pytest.mark.parametrize("m,k,trans", [(128, 128, False), (128, 7, False), (128, 128, True)],
                         ids=["wide", "narrow", "trans"])
def test_gemm_tn_past_b3(dev, big32, m, k, trans):
    """gemm_tn with the column sums of D over 2^24 + 64 rows: A^T B and sum(D) are those of the
    probe rows. Peak: 12 GiB + B 8 GiB."""
    from graphneuralnetwork_amd import ops
    c = Case(_table32(big32), m, 4)
    b_full, bv = _second_operand(dev, c, k, salt=6)
    b = b_full[:, :k]
    ref = c.vals.astype(np.float64).T @ bv.astype(np.float64)
    with c.planted():
        res = ops.gemm_tn(c.table, b, b, trans=trans)
        assert res is not None
        got, ds = res
    close(got.cpu().numpy(), ref.T if trans else ref, what=f"gemm_tn {m}x{k}")
    close(ds.cpu().numpy(), bv.astype(np.float64).sum(0), what="column sums")
    small = torch.from_numpy(bv).to(dev)
    same, ds_c = ops.gemm_tn(c.compact(), small, small, trans=trans)
    close(got.cpu().numpy(), same.cpu().numpy(), what="the compact run")
    close(ds.cpu().numpy(), ds_c.cpu().numpy(), what="the compact run's column sums")


def test_gemm_tn_masked_past_b3(dev, big32):
    """gemm_tn_masked (64 x 64; B and the mask's H two column blocks of one buffer).
    Peak: 12 GiB + 8 GiB."""
    from graphneuralnetwork_amd import _lib, ops
    c = Case(_table32(big32), 64, 4)
    full, v = _second_operand(dev, c, 128, salt=8)
    b, h = full[:, :64], full[:, 64:]
    bm = v[:, :64].astype(np.float64) * np.where(v[:, 64:] > 0, 2.0, 0.0)
    assert 0.2 < (v[:, 64:] > 0).mean() < 0.8
    # the masked kernel itself, not the wrapper's torch fallback
    assert _lib.load().gnn_gemm_tn_masked_supported(64, 64)
    with c.planted():
        got, ds = ops.gemm_tn_masked(c.table, b, h, 2.0, True)
    close(got.cpu().numpy(), c.vals.astype(np.float64).T @ bm, what="gemm_tn_masked")
    close(ds.cpu().numpy(), bm.sum(0), what="masked column sums")


@pytest.mark.parametrize("k,fout", [(128, 16), (16, 64)], ids=["narrow_out", "narrow_in"])
def test_linear_small_past_b3(dev, big32, k, fout):
    """linear_small, both kinds, over 2^24 + 64 rows (pitch 128). Peak: 12 GiB + Y up to 4 GiB."""
    from graphneuralnetwork_amd import ops
    c = Case(_table32(big32), k, 4)
    _need(dev, c.n * fout * 4, "linear_small's result")
    w, wd = _weights(dev, fout, k, 3)
    with c.planted():
        y = ops.linear_small(c.table, wd)
        same = ops.linear_small(c.compact(), wd)
    assert y is not None and y.shape == (c.n, fout)
    assert _rows_equal_to(y, torch.zeros(fout, device=dev)) == c.n - c.P
    got = y[_dev_idx(c.rows, dev)]
    assert torch.equal(got, same)
    close(got.cpu().numpy(), c.vals.astype(np.float64) @ w.T.astype(np.float64),
          what=f"linear_small k={k} fout={fout}")


def test_linear_relu_classify_past_b3(dev, big32):
    """linear_relu_classify: the embedding and the 3 logits of every row.
    Peak: 12 GiB + Y 8 GiB + logits 0.2 GiB."""
    from graphneuralnetwork_amd import ops
    c = Case(_table32(big32), 128, 4)
    _need(dev, c.n * 131 * 4, "the classifier layer's results")
    w, wd = _weights(dev, 128, 128, 4)
    wc, wcd = _weights(dev, 3, 128, 5)
    bc = np.array([0.25, -0.5, 1.0], np.float32)
    out = torch.empty((c.n, 128), device=dev)
    out.fill_(float("nan"))
    with c.planted():
        res = ops.linear_relu_classify(c.table, wd, wcd, torch.from_numpy(bc).to(dev), out=out)
        same = ops.linear_relu_classify(c.compact(), wd, wcd, torch.from_numpy(bc).to(dev))
    assert res is not None and res[0] is out
    logits = res[1]
    assert _all_nan_rows(out) == 0
    assert _rows_equal_to(out, torch.zeros(128, device=dev)) == c.n - c.P
    bcd = torch.from_numpy(bc).to(dev)
    assert _rows_equal_to(logits, bcd) == _fill_rows(c, same[1], bcd)
    rt = _dev_idx(c.rows, dev)
    assert torch.equal(out[rt], same[0]) and torch.equal(logits[rt], same[1])
    y = np.maximum(c.vals.astype(np.float64) @ w.T.astype(np.float64), 0)
    close(out[rt].cpu().numpy(), y, what="embedding")
    close(logits[rt].cpu().numpy(), y @ wc.T.astype(np.float64) + bc, what="logits")


def test_col_mean_past_b3(dev, big32):
    """col_mean over 2^24 + 64 rows: the probe rows' sums / n. Peak: 12 GiB."""
    from graphneuralnetwork_amd import ops
    c = Case(_table32(big32), 128, 4)
    with c.planted():
        got = ops.col_mean(c.table)
    close_sum(got.cpu().numpy(), c.vals.astype(np.float64).sum(0) / c.n, "col_mean")


def test_gat_project_past_b3(dev, big32):
    """gat_project (K = 128 -> 8 heads x 4): Wh, el, er of every row.
    Peak: 12 GiB + Wh 2 GiB + el, er 1 GiB."""
    from graphneuralnetwork_amd import ops
    H, fh = 8, 4
    c = Case(_table32(big32), 128, 4)
    _need(dev, c.n * (H * fh + 2 * H) * 4, "the projection's results")
    w, wd = _weights(dev, 128, H * fh, 6)  # [k, fout]
    a_s = (np.arange(H * fh) % 5 - 2).astype(np.float32) / 4
    a_d = (np.arange(H * fh) % 3 - 1).astype(np.float32) / 2
    ad = [torch.from_numpy(a).to(dev) for a in (a_s, a_d)]
    with c.planted():
        res = ops.gat_project(c.table, wd, H, fh, *ad)
        same = ops.gat_project(c.compact(), wd, H, fh, *ad)
    assert res is not None and same is not None
    whn = c.vals.astype(np.float64) @ w.astype(np.float64)
    el_o, er_o = O.gat_logits(whn, H, fh, a_s, a_d)
    rt = _dev_idx(c.rows, dev)
    for name, t, t_c, ref in zip(("Wh", "el", "er"), res, same, (whn, el_o, er_o)):
        assert t.shape[0] == c.n
        z = torch.zeros(t.shape[1], device=dev)
        assert _rows_equal_to(t, z) == _fill_rows(c, t_c, z), name
        assert torch.equal(t[rt], t_c), name
        close(t[rt].cpu().numpy(), ref, what=name)


@pytest.mark.parametrize("fh", [16, 15], ids=["vector", "scalar"])
def test_gat_logits_past_b3(dev, big32, fh):
    """gat_logits over [2^24 + 64, 8 x fh] (pitch 128): fh = 16 takes the float4 kernel with its
    32-bit (node, head) index, fh = 15 the scalar one. Peak: 12 GiB + el, er 1 GiB."""
    from graphneuralnetwork_amd import ops
    H = 8
    c = Case(_table32(big32), H * fh, 4)
    _need(dev, c.n * 2 * H * 4, "el and er")
    a_s = (np.arange(H * fh) % 5 - 2).astype(np.float32) / 4
    a_d = (np.arange(H * fh) % 7 - 3).astype(np.float32) / 4
    ad = [torch.from_numpy(a).to(dev) for a in (a_s, a_d)]
    with c.planted():
        el, er = ops.gat_logits(c.table, H, fh, *ad)
        el_c, er_c = ops.gat_logits(c.compact(), H, fh, *ad)
    el_o, er_o = O.gat_logits(c.vals, H, fh, a_s, a_d)
    rt = _dev_idx(c.rows, dev)
    z = torch.zeros(H, device=dev)
    for name, t, t_c, ref in (("el", el, el_c, el_o), ("er", er, er_c, er_o)):
        assert t.shape == (c.n, H)
        assert _rows_equal_to(t, z) == _fill_rows(c, t_c, z), name
        assert torch.equal(t[rt], t_c), name
        close(t[rt].cpu().numpy(), ref, what=name)


def test_sage_score_past_b3(dev, big32):
    """sage_score and its adjoint with second = [(2^18 + 1) x 64, 128]: row b S + s passes B1,
    B2 and B3. Scores and d_center are those of the probe rows (zero elsewhere); d_second is
    the exact product g[b, s] center[b] for every row. Peak: 12 GiB + d_second 8 GiB + 1 GiB of
    pieces."""
    from graphneuralnetwork_amd import ops
    S, H = 64, 128
    B = N32 // S
    assert B * S == N32
    c = Case(_table32(big32), H, 4)
    _need(dev, N32 * H * 4 + GIB, "d_second")
    b_of, s_of = c.rows // S, c.rows % S
    # centre rows and gradients everywhere: small multiples of 1/4 from the row number
    bi = torch.arange(B, device=dev).view(B, 1)
    center = ((bi * 7 + torch.arange(H, device=dev) * 3) % 17 - 8).float() / 4
    g = ((bi * 5 + torch.arange(S, device=dev) * 11) % 13 - 6).float() / 4
    cn, gn = center[_dev_idx(b_of, dev)].cpu().double().numpy(), g.cpu().double().numpy()
    with c.planted():
        z = ops.sage_score(center, c.table, S)
        assert z is not None and z.shape == (B, S)
        want = torch.zeros((B, S), dtype=torch.float64)
        want[torch.from_numpy(b_of), torch.from_numpy(s_of)] = torch.from_numpy(
            (cn * c.vals.astype(np.float64)).sum(1))
        _close(z, want, "scores")
        del z
        dc, dx = ops.sage_score_backward(g, center, c.table)
    want = torch.zeros((B, H), dtype=torch.float64)
    for i in range(c.P):
        want[b_of[i]] += torch.from_numpy(gn[b_of[i], s_of[i]] * c.vals[i].astype(np.float64))
    _close(dc, want, "d_center")
    assert dx.shape == (N32, H)
    step = 1 << 14
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        exact = (g[b0:b1].unsqueeze(2) * center[b0:b1].unsqueeze(1)).reshape(-1, H)
        assert torch.equal(dx[b0 * S:b1 * S], exact), f"d_second rows {b0 * S}.."


@pytest.mark.parametrize("kind", ["float", "int64"])
def test_bce_logits_both_instantiations(dev, big32, kind):
    """bce_logits with 32768 columns and 2^16 + 2 rows (n = 2^31 + 65536: the WIDE
    instantiation's 64-bit division) and with 2^16 - 2 rows of the same tensors (n = 2^31 -
    65536: the 32-bit one), with and without the gradient, against torch's
    binary_cross_entropy_with_logits in float64 summed over pieces on the device.
    z and y are column slices of rows 8 elements wider (pitch 32776): the kernel addresses
    z[r ldz + col] with (r, col) from its division of the flat index, so a wrong quotient reads
    another element (with contiguous operands every quotient would give the same address).
    z lives in the module's fp32 buffer (refilled with zeros after). Peak: 12 GiB + y 8 GiB
    (16 GiB as int64) + g 8 GiB + 1 GiB of pieces = 29 / 37 GiB."""
    from graphneuralnetwork_amd import ops
    cols, pitch = BCE_COLS, BCE_COLS + BCE_PAD
    rows_w, rows_n = BCE_ROWS, BCE_ROWS - 4
    assert rows_w * cols > 2 ** 31 - 1 >= rows_n * cols and rows_w * pitch <= BIG32_ELEMS
    ybytes = rows_w * pitch * (8 if kind == "int64" else 4)
    _need(dev, ybytes + rows_w * cols * 4 + GIB, "the labels and the gradient")
    z = big32[:rows_w * pitch].view(rows_w, pitch)[:, :cols]
    assert z.stride(0) == pitch
    step = 512  # rows per piece: 2^24 elements
    gen = torch.Generator(device=dev).manual_seed(7)
    try:
        y = torch.zeros((rows_w, pitch), device=dev,
                        dtype=torch.int64 if kind == "int64" else torch.float32)[:, :cols]
        row_sum = torch.empty(rows_w, dtype=torch.float64, device=dev)
        for r0 in range(0, rows_w, step):
            zc, yc = z[r0:r0 + step], y[r0:r0 + step]
            zc.normal_(0.0, 3.0, generator=gen)
            yc.random_(0, 2, generator=gen)
            row_sum[r0:r0 + step] = F_.binary_cross_entropy_with_logits(
                zc.double(), yc.double(), reduction="none").sum(1)
        for rows in (rows_w, rows_n):
            n = rows * cols
            ref = row_sum[:rows].sum() / n
            zz, yy = z[:rows], y[:rows]
            assert zz.stride(0) == yy.stride(0) == pitch
            only, none = ops.bce_logits(zz, yy, want_grad=False)
            assert none is None
            loss, g = ops.bce_logits(zz, yy)
            assert torch.equal(only, loss) and g.shape == (rows, cols)
            _close(loss, ref, f"loss {kind} n={n}")
            worst = 0.0
            for r0 in range(0, rows, step):
                zc, yc = zz[r0:r0 + step].double(), yy[r0:r0 + step].double()
                want = (torch.sigmoid(zc) - yc) / n
                err = (g[r0:r0 + step].double() - want).abs()
                scale = float(want.abs().max())
                worst = max(worst, float(err.max()) / scale)
                bad = err > 2e-5 * scale + 1e-4 * want.abs()  # _close's rule, per piece
                assert not bool(bad.any()), f"gradient rows {r0}.. of n={n}"
            print(f"g {kind} n={n}: max|err| / max|ref| {worst:.3e}")
            del g
    finally:
        big32.zero_()
