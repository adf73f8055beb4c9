"""Packed SpMM tasks (spmm_kernels.hpp packed_rows) at the boundaries of a slot's edge stream.

A slot streams its rows' edges in (col, val) chunks of LPR edges and, within a chunk, in batches
of U neighbour rows: a batch is requested, waited for and summed, and a row is written as soon
as the stream passes its end. So the shapes here put row ends, chunk ends, runs of edgeless rows
and the ends of the slots' streams at every offset of a batch and of a chunk: against the
C oracle (tolerance of tests/test_spmm_gpu.py), and bitwise where the kernel's contract is
bitwise -- a packed row's sum runs in edge order in one slot, so it does not depend on how the
rows are cut into tasks, nor on the run.
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import c_oracle

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# (max_deg, cost) of the task plan: 1-row tasks, short tasks, the default, 63-row tasks
CUTS = ((1, 4), (8, 16), (128, 128), (128, 256))
# F -> (LPR lanes per row, U rows in flight per slot): 2 slots, 4 slots, NCH = 2, the narrow path
SHAPES = {128: (32, 4), 64: (16, 4), 256: (64, 2), 8: (2, 8)}


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


def _stream_degrees(F, rng, n=3000):
    lpr, u = SHAPES[F]
    marks = np.array([0, 1, u - 1, u, u + 1, lpr - 1, lpr, lpr + 1, 2 * lpr + 1])
    deg = rng.choice(marks, n)
    deg[:5] = 0                     # edgeless rows open the first task ...
    deg[400:404] = 0                # ... sit in the middle of one ...
    deg[700:790] = 0                # ... fill more than a whole task ...
    deg[n - 6:] = 0                 # ... and close the last one
    deg[1000:1200] = 1              # 63-row tasks at cost 256
    deg[1200:1210] = [120, 1, 0, 1, 120, 0, 0, 0, 1, 120]  # slots' streams apart by > a chunk
    deg[1300:1304] = [127, 128, 127, 126]  # rows of about a task's cost: 1-row tasks, slot 2 idle
    deg[1500:1503] = [300, 129, 700]       # mid rows and long-row segments between the tasks
    return deg


def _stream_case(F, seed, dev):
    rng = np.random.default_rng(seed)
    deg = _stream_degrees(F, rng)
    n = deg.size
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)
    val = rng.standard_normal(rowptr[-1]).astype(np.float32)
    X = rng.standard_normal((n, F)).astype(np.float32)
    b = rng.standard_normal(F).astype(np.float32)
    return deg, rowptr, col, val, X, b, _graph(rowptr, col, val, n, dev)


def _set_cut(monkeypatch, ops, max_deg, cost):
    monkeypatch.setattr(ops, "TASK_MAX_DEG", max_deg)
    monkeypatch.setattr(ops, "TASK_COST", cost)
    monkeypatch.setattr(ops, "TASK_COST_NARROW", cost)


@pytest.mark.parametrize("F", sorted(SHAPES))
def test_stream_boundaries(dev, F, monkeypatch):
    """Row degrees {0, 1, U-1, U, U+1, LPR-1, LPR, LPR+1, 2 LPR+1}, runs of edgeless rows at the
    start, middle and end of tasks and longer than a task, 1-row and 63-row tasks, idle slots and
    slots whose streams differ by more than a chunk, under four task cuts: each against the
    oracle; the rows packed under two cuts bitwise equal between them; two runs bitwise equal."""
    from graphneuralnetwork_amd import ops
    deg, rowptr, col, val, X, b, g = _stream_case(F, 700 + F, dev)
    Xd, bd = torch.from_numpy(X).to(dev), torch.from_numpy(b).to(dev)
    ref = c_oracle.spmm_csr(rowptr, col, val, X, b)
    ys = {}
    for max_deg, cost in CUTS:
        _set_cut(monkeypatch, ops, max_deg, cost)
        y = ops.spmm_forward(g, Xd, bd, seg_len=256, hubs=0)
        tp = g._plans[("_tasks", 256, max_deg, cost)]
        rows = (tp.task_row[1::2] - tp.task_row[0::2]).cpu().numpy()
        assert rows.min() == 1 and rows.max() == (63 if cost == 256 else rows.max())
        close(y.cpu().numpy(), ref)
        assert torch.equal(y, ops.spmm_forward(g, Xd, bd, seg_len=256, hubs=0))
        ys[(max_deg, cost)] = y
    for a, c in itertools.combinations(CUTS, 2):
        both = torch.from_numpy(deg <= min(a[0], c[0])).to(dev)
        assert torch.equal(ys[a][both], ys[c][both]), (a, c)


@pytest.mark.parametrize("cut", [(8, 16), (128, 128)])
def test_epilogues(dev, cut, monkeypatch):
    """Bias, no bias, ReLU and ELU; accumulate, with the edgeless rows left bit-untouched (-0.0
    included) under SKIP_EMPTY; long-row segments plus the fix-up (seg_len 64)."""
    from graphneuralnetwork_amd import ops
    F = 128
    deg, rowptr, col, val, X, b, g = _stream_case(F, 31, dev)
    Xd, bd = torch.from_numpy(X).to(dev), torch.from_numpy(b).to(dev)
    _set_cut(monkeypatch, ops, *cut)
    plain = c_oracle.spmm_csr(rowptr, col, val, X)
    biased = c_oracle.spmm_csr(rowptr, col, val, X, b).astype(np.float64)
    for seg_len in (256, 64):
        close(ops.spmm_forward(g, Xd, None, seg_len=seg_len, hubs=0).cpu().numpy(), plain)
        close(ops.spmm_forward(g, Xd, bd, seg_len=seg_len, hubs=0).cpu().numpy(), biased)
        close(ops.spmm_forward(g, Xd, bd, activation="relu", seg_len=seg_len, hubs=0).cpu().numpy(),
              np.maximum(biased, 0))
        close(ops.spmm_forward(g, Xd, bd, activation="elu", seg_len=seg_len, hubs=0).cpu().numpy(),
              np.where(biased > 0, biased, np.expm1(np.minimum(biased, 0))))
        base = np.random.default_rng(5).standard_normal((deg.size, F)).astype(np.float32)
        base[deg == 0] = -0.0
        base[402] = 1.5  # an edgeless row with a value to keep
        out = torch.from_numpy(base).to(dev)
        ops.spmm_forward(g, Xd, None, out=out, accumulate=True, seg_len=seg_len, hubs=0)
        got = out.cpu().numpy()
        close(got, base + plain.astype(np.float64))
        assert np.array_equal(got[deg == 0].view(np.uint32), base[deg == 0].view(np.uint32))


def _xcd_graph(n, seed):
    """Random rows with two hot columns, one-edge rows on a hub column, edgeless rows and rows
    that are all duplicates of one hub column (a single partial ref left in pass 2)."""
    from oracle import gnn_oracle as O
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(120, n, 16 * n), np.full(5000, 3), np.full(2500, n - 1),
                          np.arange(100), np.repeat(np.arange(110, 120), 8),
                          rng.integers(120, n, 6000)])
    dst = np.concatenate([rng.integers(0, n, 16 * n + 7500), np.full(100, 7), np.full(80, 11),
                          np.repeat([7, 11], 3000)])
    val = rng.standard_normal(src.size).astype(np.float32)
    return O.coo_to_csr(src, dst, val, n)


@pytest.mark.parametrize("bf16", [False, True])
def test_hub_ids_xcd_direct(dev, bf16, monkeypatch):
    """Column ids c < 0 (refs to pass 1's partial rows) through the XCD-direct form: fp32, and a
    bf16 X with the fp32 partial rows (the mixed instance); with long-row segments."""
    from graphneuralnetwork_amd import ops
    from graphneuralnetwork_amd.graph import degree_order
    monkeypatch.setattr(ops, "XCD_MIN_DEG", 4)
    monkeypatch.setattr(ops, "XCD_CHUNK", 8)
    n, F = 1500, 128
    rowptr, col, val = _xcd_graph(n, 17)
    o = degree_order(_graph(rowptr, col, val, n, dev), rows=False)
    X = torch.randn(n, F, device=dev)
    if bf16:
        X = X.bfloat16()
    Xp = o.permute_rows(X.float()).to(X.dtype)
    b = torch.randn(F, device=dev)
    want = c_oracle.spmm_csr(rowptr, col, val, X.float().cpu().numpy(), b.cpu().numpy())
    for cut in ((8, 16), (128, 128)):
        _set_cut(monkeypatch, ops, *cut)
        for seg_len in (None, 16):
            y = ops.spmm_forward(o.graph, Xp, b, seg_len=seg_len, hubs=200, xcd=True)
            assert o.graph._plans[("_xcd", 200, 4, min(8, seg_len or 10 ** 9), 1, None, None)].prefix
            close(y.cpu().numpy(), want)
            assert torch.equal(y, ops.spmm_forward(o.graph, Xp, b, seg_len=seg_len, hubs=200,
                                                   xcd=True))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_row_stays_in_its_row(dev, bad, monkeypatch):
    """One NaN / Inf row of X gathered as the LAST edge of a row -- at every position of a
    batch, just before the row end -- makes that output row non-finite and no other."""
    from graphneuralnetwork_amd import ops
    F, n = 128, 600
    rng = np.random.default_rng(3)
    deg = rng.integers(1, 12, n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(1, n, rowptr[-1]).astype(np.int32)   # column 0: the non-finite row
    hit = np.arange(3, n, 7)
    col[rowptr[hit + 1] - 1] = 0
    val = rng.standard_normal(rowptr[-1]).astype(np.float32)
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[0] = bad
    g = _graph(rowptr, col, val, n, dev)
    touched = np.zeros(n, bool)
    touched[hit] = True
    for cut in ((8, 16), (128, 128)):
        _set_cut(monkeypatch, ops, *cut)
        y = ops.spmm_forward(g, torch.from_numpy(X).to(dev), None, hubs=0).cpu().numpy()
        assert not np.isfinite(y[touched]).any()
        assert np.isfinite(y[~touched]).all()
        Xf = X.copy()
        Xf[0] = 0.0
        close(y[~touched], c_oracle.spmm_csr(rowptr, col, val, Xf)[~touched])
