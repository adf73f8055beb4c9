"""The gcn-mode GraphSAGE layers on the GPU (GraphSAGE(.., gcn=True): relu(W . agg), no centre
half): the aggregate-only gathers (ops.sage_gather_aggregate_arg, ops.sage_gather_aggregate with
live=), the transposed maps of the neighbour map alone (ops.sage_maps_transpose_nbr), the adjoint
of the gcn gather (ops.sage_scatter_agg / ops.sage_scatter_agg_maxpool), the autograd function
over them (graphsage._SageGcnTrainLayerFn) and the inference layer (graphsage._fused_gcn_layer),
wired into GraphSAGE.forward behind graphsage.SAGE_GCN_FUSED.

The gathers and the transpose are compared bit for bit (with the kernels they restate, torch.argmax
on the CPU, numpy's stable argsort); the scatters with numpy's float64 np.add.at (rtol 1e-4, atol
1e-5 max|ref|, test_sage_train_gpu.close_sum); the layer and the model step with a float64 CPU
restatement on inputs the REFERENCE shows to be away from every kink (test_sage_train_gpu.close);
the inference forward with the switch off under the fp32 rule of test_unsup_sampler_gpu._close.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAP = 1e-3    # a (row, feature) top-two gap of at least GAP max|candidates' table|
KINK = 1e-4   # a pre-activation of at least KINK max|pre|
AGGS = ["MEAN", "MAXPOOL"]


def close(a, b, rtol=1e-4, what=""):  # test_sage_train_gpu.close
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    err = float(np.nanmax(np.abs(a - b))) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale, err_msg=what)


def close_sum(a, b, what=""):  # test_sage_train_gpu.close_sum: no floor at 1
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * scale, err_msg=what)


def close32(got, ref, what):  # test_unsup_sampler_gpu._close: the project's fp32 rule
    a, b = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(np.abs(b).max())
    print(f"{what}: max|err| {np.abs(a - b).max():.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=2e-5 * scale, err_msg=what)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------ the arg gather, bit-exact
N_TABLE = 400


@functools.lru_cache(maxsize=None)
def _fwd_table(F):  # test_sage_maxpool_train_gpu._fwd_table
    """Integer-valued entries in [-3, 3] (exact ties everywhere), +0.0 against -0.0, +-inf, and
    NaNs in chosen rows; every value is bf16-representable."""
    rng = np.random.default_rng(100 + F)
    t = rng.integers(-3, 4, (N_TABLE, F)).astype(np.float32)
    t[rng.random((N_TABLE, F)) < 0.05] = -0.0
    t[rng.random((N_TABLE, F)) < 0.01] = np.inf
    t[rng.random((N_TABLE, F)) < 0.02] = -np.inf
    t[5, :] = -0.0            # rows 5 / 6: -0.0 against +0.0 in every column
    t[6, :] = 0.0
    t[7, ::2] = np.nan        # rows 7 / 8 / 9: NaNs (several per candidate set below)
    t[8, :] = np.nan
    t[9, 1::2] = np.nan
    return t


def _fwd_maps(M, k, seed):  # test_sage_maxpool_train_gpu._fwd_maps
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N_TABLE, (M, k)).astype(np.int64)
    cidx = rng.integers(0, N_TABLE, M).astype(np.int64)
    if k >= 2:
        idx[::3, 1] = idx[::3, 0]                 # a neighbour repeated within a row
        idx[M // 2, :2] = (5, 6)                  # -0.0 then +0.0 ...
        idx[M // 3, :2] = (6, 5)                  # ... and the other way round
    if k >= 10:
        r = M // 4
        idx[r, :] = rng.integers(10, N_TABLE, k)  # NaNs at chosen slots: the first NaN wins
        idx[r, 3], idx[r, 6], idx[r, 8] = 9, 8, 7
        idx[-1, k - 1] = 8                        # a NaN in the last slot of the last row
    return cidx, idx


def _check_arg_gather(dev, F, k, M, bf16):
    from graphneuralnetwork_amd import ops
    t_np = _fwd_table(F)
    _, idx = _fwd_maps(M, k, 7 * F + k + M)
    table = torch.from_numpy(t_np).to(dev)
    if bf16:
        table = table.bfloat16()
        assert np.array_equal(table.float().cpu().numpy(), t_np, equal_nan=True)
    ix = torch.from_numpy(idx).to(dev)
    r = ops.sage_gather_aggregate_arg(table, ix)
    assert r is not None
    out, arg = r
    assert out.shape == (M, F) and out.dtype == torch.float32
    assert arg.shape == (M, F) and arg.dtype == torch.uint8
    out_np, arg_np = out.cpu().numpy(), arg.cpu().numpy()
    # values == the MAXPOOL kernel's (NaN == NaN; +0.0 == -0.0)
    pool = ops.sage_gather_aggregate(table, ix, "MAXPOOL").cpu().numpy()
    assert np.array_equal(out_np, pool, equal_nan=True)
    assert np.array_equal(np.isnan(out_np), np.isnan(pool))
    # arg == the argmax kernel's, and torch.argmax's on the CPU (first maximum, a NaN first)
    amax = ops.sage_gather_aggregate(table, ix, "MAX").cpu().numpy()
    assert amax.max() < k
    assert np.array_equal(arg_np, amax.astype(np.uint8))
    cpu = torch.argmax(torch.from_numpy(t_np)[torch.from_numpy(idx)], dim=1).numpy()
    assert np.array_equal(arg_np.astype(np.int64), cpu)
    # the stored value is the value AT the stored slot, bit for bit
    rows = np.take_along_axis(idx, arg_np.astype(np.int64), 1)
    assert np.array_equal(_bits(out_np), _bits(t_np[rows, np.arange(F)[None, :]]))
    return out_np, arg_np, idx


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 11, 26, 255])
@pytest.mark.parametrize("F", [8, 64, 128])
def test_arg_gather_is_bit_exact(dev, F, k, bf16):
    M = 203  # not a multiple of the 4 waves of a workgroup
    out, arg, idx = _check_arg_gather(dev, F, k, M, bf16)
    if k >= 10:
        r = M // 4   # slots 3 (odd columns), 6 (all), 8 (even columns) hold NaNs
        assert np.isnan(out[r]).all()
        assert (arg[r, 1::2] == 3).all() and (arg[r, 0::2] == 6).all()
    if k >= 2:       # +0.0 ties -0.0: the first slot wins unless a later one is larger
        for r in (M // 2, M // 3):
            t = _fwd_table(F)[idx[r]]
            assert (arg[r][t.max(0) == 0] == 0).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_arg_gather_single_row(dev, bf16):
    for F, k in ((8, 1), (64, 11), (128, 255)):
        _check_arg_gather(dev, F, k, 1, bf16)


def test_arg_gather_declines_what_it_does_not_cover(dev):
    from graphneuralnetwork_amd import ops
    t = torch.zeros((9, 64), device=dev)
    assert ops.sage_gather_aggregate_arg(
        t, torch.zeros((5, 256), dtype=torch.int64, device=dev)) is None          # k = 256
    ix = torch.zeros((5, 3), dtype=torch.int64, device=dev)
    assert ops.sage_gather_aggregate_arg(torch.zeros((9, 36), device=dev), ix) is None  # F = 36
    assert ops.sage_gather_aggregate_arg(torch.zeros((9, 4), device=dev).bfloat16(), ix) is None
    assert ops.sage_gather_aggregate_arg(t, ix) is not None
    with pytest.raises(IndexError):  # an out-of-range index raises, as in the other gathers
        ops.sage_gather_aggregate_arg(t, ix + 9)
    with pytest.raises(IndexError):
        ops.sage_gather_aggregate_arg(t, ix - 1)


# ------------------------------------------------------------------ the live form
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("F", [64, 37])  # whole 16-B lanes, and one element per lane
def test_live_gather(dev, F, agg, bf16):
    """Capacity 203: rows below the device count equal the synced call bit for bit, rows at and
    past it still hold what the output held."""
    from graphneuralnetwork_amd import ops
    rng = np.random.default_rng(F)
    cap, k = 203, 11
    table = torch.from_numpy(rng.standard_normal((N_TABLE, F)).astype(np.float32)).to(dev)
    if bf16:
        table = table.bfloat16()
    ix = torch.from_numpy(rng.integers(0, N_TABLE, (cap, k))).to(dev)
    full = ops.sage_gather_aggregate(table, ix, agg).cpu().numpy()
    assert np.isfinite(full).all()
    fill = _bits(np.full((1, F), np.nan, np.float32))
    for live in (0, 1, 150, 203, 500):
        out = torch.full((cap, F), float("nan"), device=dev)
        lv = torch.tensor([live], dtype=torch.int64, device=dev)
        got = ops.sage_gather_aggregate(table, ix, agg, out=out, live=lv)
        assert got is out
        got = got.cpu().numpy()
        n = min(live, cap)
        assert np.array_equal(_bits(got[:n]), _bits(full[:n])), live
        assert (_bits(got[n:]) == fill).all(), live
    with pytest.raises(ValueError, match="live"):
        ops.sage_gather_aggregate(table, ix, "MAX", live=lv)
    with pytest.raises(ValueError, match="live"):
        ops.sage_gather_aggregate(table, ix, "SUM", live=lv)
    with pytest.raises(IndexError):  # a checked call still reports a bad index below the count
        ops.sage_gather_aggregate(table, ix + N_TABLE, agg, live=lv)


# ------------------------------------------------------------------ the transposed maps
def _np_transpose(idx, n_prev):
    tgt = idx.reshape(-1)
    slot = np.argsort(tgt, kind="stable").astype(np.int32)
    ptr = np.zeros(n_prev + 1, np.int64)
    np.cumsum(np.bincount(tgt, minlength=n_prev), out=ptr[1:])
    return ptr, slot


def _check_transpose(dev, idx_t, n_prev):
    from graphneuralnetwork_amd import ops
    tr = ops.sage_maps_transpose_nbr(idx_t, n_prev)
    ptr, slot = _np_transpose(idx_t.cpu().numpy(), n_prev)
    assert (tr.M, tr.k) == tuple(idx_t.shape) and tr.centre is False
    assert tr.ptr.dtype == torch.int64 and tr.slot.dtype == torch.int32
    assert tr.slot.numel() == idx_t.numel()
    assert np.array_equal(tr.ptr.cpu().numpy(), ptr)
    assert np.array_equal(tr.slot.cpu().numpy(), slot)
    return tr


# the cases of test_sage_train_gpu.py::test_transpose_is_bit_exact (repeats: the targets drawn
# from a third of the range, so every list is long)
@pytest.mark.parametrize("M,k,n_prev", [(1, 1, 1), (7, 3, 5), (300, 25, 64), (1000, 10, 4096)])
@pytest.mark.parametrize("repeats", [False, True])
def test_transpose_is_bit_exact(dev, M, k, n_prev, repeats):
    rng = np.random.default_rng(M + 7 * k)
    hi = max(1, n_prev // 3) if repeats else n_prev
    idx = rng.integers(0, hi, (M, k)).astype(np.int64)
    _check_transpose(dev, torch.from_numpy(idx).to(dev), n_prev)


def test_transpose_unreferenced_targets_one_segment_and_strided_maps(dev):
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 256, (200, 11)).astype(np.int64)  # targets 256.. have no slot
    tr = _check_transpose(dev, torch.from_numpy(idx).to(dev), 512)
    assert (tr.ptr[256:] == 2200).all()
    # n_prev = 1: every slot in one segment
    _check_transpose(dev, torch.zeros((333, 4), dtype=torch.int64, device=dev), 1)
    # a strided [M, k] view of a wider buffer (the sampler's maps are pieces of one buffer)
    wide = torch.from_numpy(rng.integers(0, 512, (200, 16))).to(dev)
    view = wide[:, 3:14]
    assert view.stride(0) == 16 and not view.is_contiguous()
    _check_transpose(dev, view, 512)


def test_transpose_of_no_rows_and_bad_indices(dev):
    from graphneuralnetwork_amd import ops
    tr = ops.sage_maps_transpose_nbr(torch.empty((0, 5), dtype=torch.int64, device=dev), 9)
    assert tr.M == 0 and tr.k == 5 and tr.slot.numel() == 0 and not tr.centre
    assert tr.ptr.shape == (10,) and int(tr.ptr.abs().sum()) == 0
    idx = torch.tensor([[0, 1], [2, 3], [1, 0]], device=dev)
    for bad in (4, -1):  # == n_prev, and the reference's padding value
        b = idx.clone()
        b[1, 1] = bad
        with pytest.raises(IndexError):
            ops.sage_maps_transpose_nbr(b, 4)
    # unchecked: the flawed slot lies past ptr[n_prev], the scatter never reads it
    b = idx.clone()
    b[1, 1] = 4
    tr = ops.sage_maps_transpose_nbr(b, 4, check=False)
    assert int(tr.ptr[-1]) == 5 and int(tr.slot[-1]) == 3
    dx = ops.sage_scatter_agg(torch.ones((3, 4), device=dev), tr, 4)
    want = np.zeros((4, 4))
    for t in b.flatten().tolist():
        if t < 4:
            want[t] += 0.5
    close_sum(dx.cpu().numpy(), want, "flawed slot skipped")
    # the two slot numberings do not mix
    cat = ops.sage_maps_transpose(torch.tensor([0, 1, 2], device=dev), idx, 4)
    assert cat.centre
    with pytest.raises(ValueError):
        ops.sage_scatter_agg(torch.ones((3, 4), device=dev), cat, 4)
    with pytest.raises(ValueError):
        ops.sage_scatter_concat(torch.ones((3, 8), device=dev), tr, 4)


# ------------------------------------------------------------------ the scatters
def _ref_scatter(d, idx, arg, n_prev):
    """numpy float64 np.add.at over the same map (and winners: arg None is MEAN)."""
    M, k = idx.shape
    F = d.shape[1]
    d64 = np.asarray(d, np.float64)
    out = np.zeros((n_prev, F))
    if arg is None:
        np.add.at(out, idx.reshape(-1), np.repeat(d64 / k, k, axis=0))
    else:
        rows = np.take_along_axis(idx, arg.astype(np.int64), 1)          # [M, F] targets
        np.add.at(out, (rows, np.broadcast_to(np.arange(F), rows.shape)), d64)
    return out


def _run_scatter(dev, dbuf_t, arg_t, idx, n_prev):
    from graphneuralnetwork_amd import ops
    tr = ops.sage_maps_transpose_nbr(torch.from_numpy(idx).to(dev), n_prev)
    # unreferenced rows must be WRITTEN as zeros, not left as they were
    out = torch.full((n_prev, dbuf_t.shape[1]), float("nan"), device=dev)
    dx = (ops.sage_scatter_agg(dbuf_t, tr, n_prev, out=out) if arg_t is None else
          ops.sage_scatter_agg_maxpool(dbuf_t, arg_t, tr, n_prev, out=out))
    assert dx is out
    return dx, tr


def _case(rng, M, k, F, agg):
    d = rng.standard_normal((M, F)).astype(np.float32)
    arg = rng.integers(0, k, (M, F)).astype(np.uint8) if agg == "MAXPOOL" else None
    return d, arg  # arg: independent of any forward


def _dev(dev, a):
    return None if a is None else torch.from_numpy(a).to(dev)


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("F", [128, 64, 8])
@pytest.mark.parametrize("k", [1, 11, 26])
@pytest.mark.parametrize("padded", [False, True])
def test_scatter_vs_float64(dev, F, k, padded, agg):
    rng = np.random.default_rng(F + k)
    M, n_prev = 1003, 700
    idx = rng.integers(0, n_prev // 2, (M, k)).astype(np.int64)  # the upper half: unreferenced
    d, arg = _case(rng, M, k, F, agg)
    dt, at = _dev(dev, d), _dev(dev, arg)
    if padded:  # column-padded views: row strides F + 8 floats and F + 4 bytes
        wide = torch.full((M, F + 8), float("nan"), device=dev)
        wide[:, :F] = dt
        dt = wide[:, :F]
        assert dt.stride(0) == F + 8
        if at is not None:
            wa = torch.full((M, F + 4), 255, dtype=torch.uint8, device=dev)
            wa[:, :F] = at
            at = wa[:, :F]
            assert at.stride(0) == F + 4
    dx, _ = _run_scatter(dev, dt, at, idx, n_prev)
    assert dx.shape == (n_prev, F) and dx.dtype == torch.float32
    got = dx.cpu().numpy()
    assert not np.isnan(got).any()
    assert (got[n_prev // 2:] == 0).all()  # nobody references the upper half: written as zeros
    close_sum(got, _ref_scatter(d, idx, arg, n_prev), f"{agg} scatter F={F} k={k}")


def _hub_case(rng, agg, M=300, k=4, F=128):
    """One target referenced by every one of the M k = 1200 slots: the chunk path."""
    d, arg = _case(rng, M, k, F, agg)
    return d, arg, np.ones((M, k), np.int64), 3


@pytest.mark.parametrize("agg", AGGS)
def test_scatter_one_target_takes_every_slot(dev, agg):
    d, arg, idx, n_prev = _hub_case(np.random.default_rng(11), agg)
    dx, tr = _run_scatter(dev, _dev(dev, d), _dev(dev, arg), idx, n_prev)
    assert tr.ptr.tolist() == [0, 0, 1200, 1200]
    got = dx.cpu().numpy()
    assert (got[0] == 0).all() and (got[2] == 0).all()
    close_sum(got, _ref_scatter(d, idx, arg, n_prev), f"{agg} hub")


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("slots", [256, 257])
def test_scatter_list_at_the_chunk_length(dev, slots, agg):
    """A list of exactly 256 slots (the last one summed by one lane group) and one of 257 (the
    first one cut into chunks)."""
    rng = np.random.default_rng(slots)
    k, F = 4, 64
    M = 64 if slots == 256 else 65
    idx = np.zeros((M, k), np.int64)
    idx[64:, 1:] = 1  # M = 65: 256 + 1 slots on target 0, 3 on target 1
    d, arg = _case(rng, M, k, F, agg)
    dx, tr = _run_scatter(dev, _dev(dev, d), _dev(dev, arg), idx, 2)
    assert int(tr.ptr[1]) == slots
    close_sum(dx.cpu().numpy(), _ref_scatter(d, idx, arg, 2), f"{agg} {slots} slots")


def test_scatter_nonfinite_gradients(dev):
    """MAXPOOL selects and never multiplies: a NaN / Inf gradient reaches the target of the slot
    that won it and nobody else. MEAN is a plain sum: it reaches every target of its row."""
    rng = np.random.default_rng(13)
    M, k, F, n_prev = 500, 11, 64, 6000
    idx = np.stack([rng.permutation(n_prev)[:k] for _ in range(M)]).astype(np.int64)  # distinct
    d, arg = _case(rng, M, k, F, "MAXPOOL")
    d[401, 9] = np.nan
    d[17, 5] = np.inf
    d[17, 6] = -np.inf
    for agg in AGGS:
        a = arg if agg == "MAXPOOL" else None
        dx, _ = _run_scatter(dev, _dev(dev, d), _dev(dev, a), idx, n_prev)
        got = dx.cpu().numpy()
        nan_at, pinf, ninf = (np.zeros((n_prev, F), bool) for _ in range(3))
        if agg == "MAXPOOL":
            nan_at[idx[401, arg[401, 9]], 9] = True
            pinf[idx[17, arg[17, 5]], 5] = True
            ninf[idx[17, arg[17, 6]], 6] = True
        else:
            nan_at[idx[401], 9] = True
            pinf[idx[17], 5] = True
            ninf[idx[17], 6] = True
        assert not (nan_at & (pinf | ninf)).any()  # (the rows' targets are distinct)
        assert np.array_equal(np.isnan(got), nan_at), agg
        assert np.array_equal(np.isposinf(got), pinf), agg
        assert np.array_equal(np.isneginf(got), ninf), agg
        ref = _ref_scatter(d, idx, a, n_prev)
        if agg == "MAXPOOL":  # the slots that did not win: finite, the sum without them
            for m, f in ((401, 9), (17, 5), (17, 6)):
                losers = np.delete(idx[m], arg[m, f])
                assert np.isfinite(got[losers, f]).all() and np.isfinite(ref[losers, f]).all()
        fin = ~(nan_at | pinf | ninf)
        assert np.isfinite(ref[fin]).all()
        close_sum(got[fin], ref[fin], f"{agg} finite rest")


@pytest.mark.parametrize("agg", AGGS)
def test_scatter_is_deterministic(dev, agg):
    from graphneuralnetwork_amd import _lib
    d, arg, idx, n_prev = _hub_case(np.random.default_rng(12), agg)
    dt, at = _dev(dev, d), _dev(dev, arg)
    a, tr = _run_scatter(dev, dt, at, idx, n_prev)
    a = a.clone()
    b, _ = _run_scatter(dev, dt, at, idx, n_prev)
    assert torch.equal(a, b)
    # the same maps, a workspace full of garbage: the entry itself clears what it reads
    lib = _lib.load()
    M, k, F = tr.M, tr.k, d.shape[1]
    c = torch.full((n_prev, F), float("nan"), device=dev)
    if agg == "MAXPOOL":
        nbytes = int(lib.gnn_sage_scatter_agg_maxpool_workspace_bytes(M, k, F))
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        _lib.check(lib.gnn_sage_scatter_agg_maxpool_f32(
            dt.data_ptr(), F, at.data_ptr(), F, tr.ptr.data_ptr(), tr.slot.data_ptr(), M, k, F,
            n_prev, c.data_ptr(), F, ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
            "gnn_sage_scatter_agg_maxpool_f32")
    else:
        nbytes = int(lib.gnn_sage_scatter_agg_workspace_bytes(M, k, F))
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        _lib.check(lib.gnn_sage_scatter_agg_f32(
            dt.data_ptr(), F, tr.ptr.data_ptr(), tr.slot.data_ptr(), M, k, F, n_prev,
            c.data_ptr(), F, ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
            "gnn_sage_scatter_agg_f32")
    assert torch.equal(a, c)
    close_sum(a.cpu().numpy(), _ref_scatter(d, idx, arg, n_prev), f"{agg} hub, deterministic")
    # a mixed case: hubs past the chunk length among many short lists
    rng = np.random.default_rng(14)
    M2, k2, n2 = 3000, 11, 2000
    i2 = rng.integers(0, n2 // 2, (M2, k2)).astype(np.int64)
    i2[rng.random((M2, k2)) < 0.3] = 7
    d2, a2 = _case(rng, M2, k2, 64, agg)
    x, _ = _run_scatter(dev, _dev(dev, d2), _dev(dev, a2), i2, n2)
    x = x.clone()
    y, _ = _run_scatter(dev, _dev(dev, d2), _dev(dev, a2), i2, n2)
    assert torch.equal(x, y)
    close_sum(x.cpu().numpy(), _ref_scatter(d2, i2, a2, n2), f"{agg} mixed")


def test_scatter_declines_what_it_does_not_cover(dev):
    from graphneuralnetwork_amd import ops
    rng = np.random.default_rng(15)
    i64 = functools.partial(torch.zeros, dtype=torch.int64, device=dev)
    u8 = functools.partial(torch.zeros, dtype=torch.uint8, device=dev)
    tr = ops.sage_maps_transpose_nbr(
        torch.from_numpy(rng.integers(0, 40, (50, 3)).astype(np.int64)).to(dev), 40)
    assert ops.sage_scatter_agg(torch.zeros((50, 36), device=dev), tr, 40) is None       # F = 36
    assert ops.sage_scatter_agg(torch.zeros((50, 512), device=dev), tr, 40) is None      # F = 512
    assert ops.sage_scatter_agg(torch.zeros((50, 2), device=dev), tr, 40) is None        # F = 2
    assert ops.sage_scatter_agg_maxpool(torch.zeros((50, 36), device=dev), u8((50, 36)), tr,
                                        40) is None
    wide = u8((50, 11))
    assert ops.sage_scatter_agg_maxpool(torch.zeros((50, 8), device=dev), wide[:, :8], tr,
                                        40) is None   # rows of arg not whole words
    wd = torch.zeros((50, 10), device=dev)
    assert ops.sage_scatter_agg(wd[:, :8], tr, 40) is None   # rows of dbuf not 16-B aligned
    assert ops.sage_scatter_agg(torch.zeros((50, 8), device=dev), tr, 40) is not None
    tr3 = ops.sage_maps_transpose_nbr(i64((5, 256)), 40)
    assert ops.sage_scatter_agg_maxpool(torch.zeros((5, 8), device=dev), u8((5, 8)), tr3,
                                        40) is None   # k = 256: the winner does not fit a byte
    tr0 = ops.sage_maps_transpose_nbr(i64((5, 0)), 40)
    assert ops.sage_scatter_agg(torch.zeros((5, 8), device=dev), tr0, 40) is None  # k = 0


# ------------------------------------------------------------------ kinks of the reference
def _settle(run, redraw, tries=400):  # test_sage_maxpool_train_gpu._settle
    """run() -> [(stage, name, per-column smallest distance, bound)]; redraw(stage, name, columns)
    redraws what owns the columns whose distance is below the bound, earliest stage first. Fails
    if the fixture does not settle."""
    for _ in range(tries):
        with torch.no_grad():
            rec = run()
        bad = None
        for stage, name, m, bound in rec:
            cols = torch.nonzero(m < bound).flatten().tolist()
            if cols and (bad is None or stage < bad[0]):
                bad = (stage, name, cols)
        if bad is None:
            return rec
        redraw(*bad)
    raise AssertionError("the fixture does not clear its kinks")


def _assert_kinks(rec, tag):
    assert rec
    for stage, name, m, bound in rec:
        print(f"{tag} {name}: smallest distance {float(m.min()):.3e}, bound {bound:.3e}")
        assert float(m.min()) >= bound, (tag, stage, name)


def _gap(table, idx, zero_sets_ok=False):  # test_sage_maxpool_train_gpu._gap
    """Per column, the smallest top-two gap of max_j table[idx[m, j], f] over the rows m, taken
    among DIFFERENT table rows (a neighbour drawn twice ties with itself: the same row gets the
    gradient either way). zero_sets_ok: a candidate set that is all zeros (post-ReLU rows whose
    gradient the ReLU stops anyway) counts as no kink."""
    vals = table[idx]                                        # [M, k, F]
    top, am = vals.max(dim=1)
    win = idx.gather(1, am)                                  # [M, F] the winning table row
    same = idx.unsqueeze(2) == win.unsqueeze(1)              # [M, k, F]
    second = vals.masked_fill(same, -float("inf")).max(dim=1).values
    gap = top - second                                       # inf where one row is drawn k times
    if zero_sets_ok:
        gap = torch.where((vals == 0).all(dim=1), torch.full_like(gap, float("inf")), gap)
    return gap.min(dim=0).values


def _bf16_normal(gen, *shape):
    return torch.randn(*shape, generator=gen).bfloat16().float()


def _uniform(gen, bound, *shape):
    return (torch.rand(*shape, generator=gen) * 2 - 1) * bound


def _agg(nf, agg):
    return nf.max(dim=1).values if agg == "MAXPOOL" else nf.mean(dim=1)


# ------------------------------------------------------------------ the layer
@functools.lru_cache(maxsize=None)
def _layer_fixture(agg):
    """F, H = 64, 128; M = 200, k = 6, n_prev = 300: a bf16-representable table and a weight
    whose float64 forward relu(W . agg(table[idx])) is away from kinks, and the float64
    gradients of sum(y * G)."""
    F, H, M, k, n_prev = 64, 128, 200, 6, 300
    gen = torch.Generator().manual_seed(43)
    rng = np.random.default_rng(43)
    idx = torch.from_numpy(rng.integers(0, n_prev, (M, k)))
    table = _bf16_normal(gen, n_prev, F)
    W = _uniform(gen, F ** -0.5, H, F)
    G = torch.randn(M, H, generator=gen)

    def run():
        t, w = table.double(), W.double()
        pre = _agg(t[idx], agg) @ w.t()
        rec = [(1, "W", pre.abs().min(dim=0).values, KINK * float(pre.abs().max()))]
        if agg == "MAXPOOL":
            rec.append((0, "table", _gap(t, idx), GAP * float(t.abs().max())))
        return rec

    def redraw(stage, name, cols):
        if stage == 0:
            table[:, cols] = _bf16_normal(gen, n_prev, len(cols))
        else:
            W[cols] = _uniform(gen, F ** -0.5, len(cols), F)

    _assert_kinks(_settle(run, redraw), f"{agg} layer")  # on the CPU, before any device work
    t64, w64 = table.double().requires_grad_(), W.double().requires_grad_()
    y = torch.relu(_agg(t64[idx], agg) @ w64.t())
    (y * G.double()).sum().backward()
    return dict(table=table, W=W, idx=idx, G=G, y=y.detach().numpy(), dW=w64.grad.numpy(),
                dT=t64.grad.numpy())


@pytest.mark.parametrize("kind", ["fp32_grad", "fp32", "bf16"])
@pytest.mark.parametrize("agg", AGGS)
def test_layer_gradients_vs_float64(dev, agg, kind):
    from graphneuralnetwork_amd.graphsage import _SageGcnTrainLayerFn
    fx = _layer_fixture(agg)
    t = fx["table"].to(dev)
    t = t.bfloat16() if kind == "bf16" else t.requires_grad_(kind == "fp32_grad")
    W = fx["W"].to(dev).requires_grad_()
    y = _SageGcnTrainLayerFn.apply(t, W, fx["idx"].to(dev), agg)
    (y * fx["G"].to(dev)).sum().backward()
    close(y.detach().cpu().numpy(), fx["y"], what=f"{agg} {kind} y")
    close(W.grad.cpu().numpy(), fx["dW"], what=f"{agg} {kind} dW")
    if kind == "fp32_grad":
        close(t.grad.cpu().numpy(), fx["dT"], what=f"{agg} d table")
        assert np.abs(fx["dT"]).max() > 0
    else:
        assert t.grad is None


@pytest.mark.parametrize("agg", AGGS)
def test_layer_refuses_a_bf16_table_that_requires_grad(dev, agg):
    from graphneuralnetwork_amd.graphsage import GraphSAGE, Gathered
    fx = _layer_fixture(agg)
    t = fx["table"].to(dev).bfloat16().requires_grad_()
    net = GraphSAGE(1, 64, 128, True, agg).to(dev).train()
    cidx = fx["idx"][:, 0].contiguous().to(dev)
    with pytest.raises(TypeError, match="bfloat16"):
        net(Gathered(t, cidx, True), [], Gathered(t, fx["idx"].to(dev), True), [], None, None,
            None, None, None)


# ------------------------------------------------------------------ the model step
@functools.lru_cache(maxsize=None)
def _graph():  # test_sage_train_gpu._graph
    from graphneuralnetwork_amd.sampler import symmetric_adjacency
    rng = np.random.default_rng(21)
    n = 2000
    s, d = rng.integers(0, n, 20000), rng.integers(0, n, 20000)
    adj = symmetric_adjacency(s, d, n, device=torch.device("cuda:0"))
    deg = (adj.rowptr[1:] - adj.rowptr[:-1]).cpu().numpy()
    return n, adj, torch.from_numpy(np.flatnonzero(deg > 0)[:40])


@functools.lru_cache(maxsize=None)
def _batch(unsup):
    from graphneuralnetwork_amd.sampler import sample_batch, sample_unsupervised_batch
    n, adj, seeds = _graph()
    if unsup:  # 8 seeds: with their 2 contexts and 4 negatives each, 48 in the second tower
        b = sample_unsupervised_batch(adj, seeds[:8].to(adj.device), (5, 3), window=2, K=2,
                                      seed=3, gcn=True)
        assert b.center.frontier_nbrs.shape[1] == 4 and b.center.neigh_maps[0].shape[1] == 6
        return b
    b = sample_batch(adj, seeds.to(adj.device), (5, 3), seed=3, gcn=True)
    assert b.frontier_nbrs.shape[1] == 4 and b.neigh_maps[0].shape[1] == 6  # fanout + 1
    return b


W0, W1 = "sage_blocks.sage_layer0.weight.weight", "sage_blocks.sage_layer1.weight.weight"


def _ref_tower(P, table, b, agg, rec=None):
    """GraphSAGE.forward in gcn mode, one branch (GraphSAGE/GraphSAGE.py:13-14, 42-57: the
    aggregate alone into Linear), on the CPU in the dtype of its arguments. rec: a list that
    receives the kink distances of every maximum and pre-activation."""
    ni = b.frontier_nbrs.cpu()
    src, feats = table, None
    L = len(b.neigh_maps) + 1
    for i in range(L):
        pre = _agg(src[ni], agg) @ P[f"sage_blocks.sage_layer{i}.weight.weight"].t()
        feats = torch.relu(pre)
        if rec is not None:
            if agg == "MAXPOOL":
                rec.append((2 * i, f"max{i}", _gap(src, ni, zero_sets_ok=i > 0),
                            GAP * float(src.abs().max())))
            rec.append((2 * i + 1, f"pre{i}", pre.abs().min(dim=0).values,
                        KINK * float(pre.abs().max())))
        if i != L - 1:
            src, ni = feats, b.neigh_maps[i].cpu()
    return feats


def _loss(unsup, second, labels):
    if unsup:
        return torch.nn.functional.binary_cross_entropy_with_logits(
            second.squeeze(1), labels.to(second.dtype))
    return torch.nn.functional.cross_entropy(second, labels)


def _ref_forward(P, table, batch, unsup, labels, agg, rec=None):
    if unsup:
        emb = _ref_tower(P, table, batch.center, agg, rec)
        ctx = _ref_tower(P, table, batch.context, agg, rec).reshape(*labels.shape, -1)
        second = torch.bmm(emb.unsqueeze(1), ctx.permute(0, 2, 1))
    else:
        emb = _ref_tower(P, table, batch, agg, rec)
        second = emb @ P["dense.weight"].t() + P["dense.bias"]
    return emb, second


N_CLS = 4  # (the classifier epilogue of the inference layer takes up to 4 classes)


@functools.lru_cache(maxsize=None)
def _model_fixture(agg, unsup):
    """The parameters of GraphSAGE(2, 64, 128, True, agg), a bf16-representable table and labels
    such that the float64 forward is away from kinks (asserted here, on the CPU), and the float64
    step: output, loss and every gradient."""
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    n, F, H = _graph()[0], 64, 128
    batch = _batch(unsup)
    gen = torch.Generator().manual_seed(61 + unsup + 2 * (agg == "MEAN"))
    torch.manual_seed(0)
    net = GraphSAGE(2, F, H, True, agg, Unsupervised=unsup, class_size=None if unsup else N_CLS)
    P = {k_: v.detach().clone() for k_, v in net.named_parameters()}
    assert P[W0].shape == (H, F) and P[W1].shape == (H, H)
    table = _bf16_normal(gen, n, F)
    labels = (batch.labels.cpu() if unsup else
              torch.from_numpy(np.random.default_rng(52).integers(0, N_CLS, 40)))

    def run():
        rec = []
        _ref_forward({k_: v.double() for k_, v in P.items()}, table.double(), batch, unsup, labels,
                     agg, rec=rec)
        return rec

    def redraw(stage, name, cols):
        if stage == 0:    # a maximum over table rows: the table's columns
            table[:, cols] = _bf16_normal(gen, n, len(cols))
        elif stage <= 2:  # a layer-0 pre-activation, or a maximum over layer 0's output
            P[W0][cols] = _uniform(gen, F ** -0.5, len(cols), F)
        else:
            P[W1][cols] = _uniform(gen, H ** -0.5, len(cols), H)

    _assert_kinks(_settle(run, redraw), f"{agg} {'unsupervised' if unsup else 'supervised'}")
    P64 = {k_: v.double().requires_grad_() for k_, v in P.items()}
    t64 = table.double().requires_grad_()
    emb, second = _ref_forward(P64, t64, batch, unsup, labels, agg)
    loss = _loss(unsup, second, labels)
    loss.backward()
    ref = {"emb": emb.detach().numpy(), "second": second.detach().numpy(),
           "loss": loss.detach().numpy(), "table": t64.grad.numpy()}
    ref.update({k_: v.grad.numpy() for k_, v in P64.items()})
    return P, table, labels, ref


def _forward(net, table, batch, unsup):
    args = batch.forward_args(table)
    if not unsup:
        args = (*args, None, None, None, None, None)
    return net(*args)


def _gpu_step(net, table, batch, unsup, labels):
    net.zero_grad()
    with torch.enable_grad():
        emb, second = _forward(net, table, batch, unsup)
        loss = _loss(unsup, second, labels)
        loss.backward()
    out = {"emb": emb.detach().cpu().numpy(), "second": second.detach().cpu().numpy(),
           "loss": loss.detach().cpu().numpy()}
    if table.requires_grad:
        out["table"] = table.grad.cpu().numpy().copy()
    out.update({k_: p.grad.cpu().numpy().copy() for k_, p in net.named_parameters()})
    return out, emb.grad_fn


def _net(dev, unsup, P, agg, gcn=True):
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    net = GraphSAGE(2, 64, 128, gcn, agg, Unsupervised=unsup, class_size=None if unsup else N_CLS)
    if P is not None:
        net.load_state_dict(P)
    return net.to(dev)


FUSED, OLD = "_SageGcnTrainLayerFnBackward", "ReluBackward0"


@pytest.mark.parametrize("unsup", [False, True], ids=["supervised", "unsupervised"])
@pytest.mark.parametrize("agg", AGGS)
def test_model_step(dev, monkeypatch, agg, unsup):
    from graphneuralnetwork_amd import graphsage
    P, table, labels, ref = _model_fixture(agg, unsup)
    batch, labels_d = _batch(unsup), labels.to(dev)
    net = _net(dev, unsup, P, agg).train()
    layer_fns = []
    real = graphsage._sage_gcn_train_layer

    def seen(*a, **k):
        y = real(*a, **k)
        layer_fns.append(None if y is None else type(y.grad_fn).__name__)
        return y

    monkeypatch.setattr(graphsage, "_sage_gcn_train_layer", seen)
    towers = 2 if unsup else 1
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(graphsage, "SAGE_GCN_FUSED", fused)
        for kind in ("fp32_grad", "fp32", "bf16"):
            t = table.to(dev)
            t = t.bfloat16() if kind == "bf16" else t.requires_grad_(kind == "fp32_grad")
            del layer_fns[:]
            runs[fused, kind], fn = _gpu_step(net, t, batch, unsup, labels_d)
            # every layer of every tower is the one autograd function, or none of them is
            assert layer_fns == ([FUSED] * (2 * towers) if fused else []), (fused, kind)
            assert type(fn).__name__ == (FUSED if fused else OLD)
    names = ["emb", "second", "loss"] + list(P)
    for kind in ("fp32_grad", "fp32", "bf16"):
        for name in names + (["table"] if kind == "fp32_grad" else []):
            on, off = runs[True, kind][name], runs[False, kind][name]
            close(on, ref[name], what=f"{agg} {kind} {name}: switch on vs float64")
            close(on, off, what=f"{agg} {kind} {name}: switch on vs off")
    assert np.abs(ref["table"]).max() > 0
    for name in P:
        assert np.abs(ref[name]).max() > 0, name


@pytest.mark.parametrize("agg", AGGS)
def test_model_step_when_the_scatter_declines(dev, monkeypatch, agg):
    """A None from the scatter inside the layer's backward drops that gradient to the previous
    formulation of the same sum (the SpMM over a Python-built CSR / index_put_): same numbers."""
    from graphneuralnetwork_amd import graphsage
    P, table, labels, ref = _model_fixture(agg, False)
    monkeypatch.setattr(graphsage, "SAGE_GCN_FUSED", True)
    net = _net(dev, False, P, agg).train()
    asked = []
    name = "sage_scatter_agg_maxpool" if agg == "MAXPOOL" else "sage_scatter_agg"
    monkeypatch.setattr(graphsage, name, lambda *a, **k: asked.append(1))  # returns None
    t = table.to(dev).requires_grad_()
    run, fn = _gpu_step(net, t, _batch(False), False, labels.to(dev))
    assert len(asked) == 2 and type(fn).__name__ == FUSED
    for key in run:
        close(run[key], ref[key], what=f"{agg} {key}: scatter declined vs float64")


# ------------------------------------------------------------------ inference
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("unsup", [False, True], ids=["supervised", "unsupervised"])
@pytest.mark.parametrize("agg", AGGS)
def test_inference_forward(dev, monkeypatch, agg, unsup, bf16):
    """Eval forward on the sampler's batches: the switch on (one gather-aggregate + the MFMA GEMM
    per layer, the classifier in the last GEMM's epilogue) against the switch off."""
    from graphneuralnetwork_amd import graphsage
    P, table, _, ref = _model_fixture(agg, unsup)
    batch = _batch(unsup)
    net = _net(dev, unsup, P, agg).eval()
    t = table.to(dev).bfloat16() if bf16 else table.to(dev)
    calls = {"layer": 0, "cls": 0, "centre": 0}
    real_layer, real_cls, real_rows = (graphsage._fused_gcn_layer, graphsage.linear_relu_classify,
                                       graphsage.gather_rows)

    def layer(*a, **k):
        calls["layer"] += 1
        return real_layer(*a, **k)

    def cls(*a, **k):
        r = real_cls(*a, **k)
        calls["cls"] += r is not None
        return r

    def rows(*a, **k):
        calls["centre"] += 1
        return real_rows(*a, **k)

    monkeypatch.setattr(graphsage, "_fused_gcn_layer", layer)
    monkeypatch.setattr(graphsage, "linear_relu_classify", cls)
    monkeypatch.setattr(graphsage, "gather_rows", rows)
    out = {}
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(graphsage, "SAGE_GCN_FUSED", on)
            for key in calls:
                calls[key] = 0
            out[on] = _forward(net, t, batch, unsup)
            towers = 2 if unsup else 1
            if on:  # every layer of every tower, no centre gather, the classifier epilogue
                assert calls == {"layer": 2 * towers, "cls": 0 if unsup else 1, "centre": 0}
            else:
                assert calls["layer"] == 0 and calls["cls"] == 0 and calls["centre"] == 2 * towers
    tag = f"{agg} {'bf16' if bf16 else 'fp32'}"
    close32(out[True][0], out[False][0], f"{tag} embeddings: switch on vs off")
    close32(out[True][1], out[False][1], f"{tag} scores / logits: switch on vs off")
    close32(out[True][0], torch.from_numpy(ref["emb"]), f"{tag} embeddings vs float64")
    close32(out[True][1], torch.from_numpy(ref["second"]), f"{tag} scores / logits vs float64")


def _ring_graph(dev, n, chords, seed=0):  # test_unsup_sampler_gpu._ring_graph
    """Connected symmetric graph: a ring plus random chords (no node without neighbours)."""
    from graphneuralnetwork_amd.sampler import symmetric_adjacency
    rs = np.random.default_rng(seed)
    ring = np.arange(n)
    src = np.concatenate([ring, rs.integers(0, n, chords)])
    dst = np.concatenate([(ring + 1) % n, rs.integers(0, n, chords)])
    return symmetric_adjacency(src, dst, n, device=dev)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("unsup", [False, True], ids=["supervised", "unsupervised"])
@pytest.mark.parametrize("agg", AGGS)
def test_pending_batch_stays_pending(dev, agg, unsup, bf16):
    """sync=False in gcn mode: no host read between the sampler and the end of the inference
    forward (torch's sync debug mode raises on one); the result equals the synced batch's bit
    for bit. The graph of test_unsup_sampler_gpu.py::test_pending_unsupervised_batch."""
    from graphneuralnetwork_amd import sampler as S
    adj = _ring_graph(dev, 2000, 6000, seed=3)
    seeds = torch.arange(100, 164, device=dev)
    table = torch.randn(2000, 64, device=dev)
    if bf16:
        table = table.bfloat16()
    torch.manual_seed(7)
    net = _net(dev, unsup, None, agg).eval()

    def sample(sync):
        if unsup:
            return S.sample_unsupervised_batch(adj, seeds, (5, 3), seed=4, gcn=True, sync=sync)
        return S.sample_batch(adj, seeds, (5, 3), seed=4, gcn=True, sync=sync)

    with torch.no_grad():
        e1, s1 = _forward(net, table, sample(True), unsup)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            p = sample(False)
            e2, s2 = _forward(net, table, p, unsup)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert p.pending
    assert e1.shape == (64, 128) and torch.equal(e1, e2) and torch.equal(s1, s2)
    assert float(e1.abs().max()) > 0
    assert not p.sync().pending


# ------------------------------------------------------------------ the others
def test_other_layers_keep_their_paths(dev, monkeypatch):
    from graphneuralnetwork_amd import graphsage
    from graphneuralnetwork_amd.graphsage import GraphSAGE, Gathered
    from graphneuralnetwork_amd.sampler import sample_batch
    monkeypatch.setattr(graphsage, "SAGE_GCN_FUSED", True)
    n, adj, seeds = _graph()
    table = torch.randn(n, 64, generator=torch.Generator().manual_seed(9)).to(dev)
    labels = torch.zeros(40, dtype=torch.int64, device=dev)
    plain = sample_batch(adj, seeds.to(adj.device), (5, 3), seed=3)
    # the cat[self, agg] nets: their own functions, whatever the new switch says
    for agg, want in (("MEAN", "_SageTrainLayerFnBackward"),
                      ("MAXPOOL", "_SageMaxPoolTrainLayerFnBackward")):
        _, fn = _gpu_step(_net(dev, False, None, agg, gcn=False).train(), table, plain, False,
                          labels)
        assert type(fn).__name__ == want
    rng = np.random.default_rng(61)
    cidx = torch.from_numpy(rng.integers(0, n, 50)).to(dev)
    idx = torch.from_numpy(rng.integers(0, n, (50, 6))).to(dev)

    def one(net, trusted=True):
        return net(Gathered(table, cidx, trusted), [], Gathered(table, idx, trusted), [], None,
                   None, None, None, None)

    for agg in AGGS:
        net = GraphSAGE(1, 64, 128, True, agg).to(dev).train()
        assert type(one(net)[0].grad_fn).__name__ == FUSED
        # untrusted maps keep the previous path (relu of torch's linear)
        assert type(one(net, trusted=False)[0].grad_fn).__name__ == OLD
        # H = 16: a width the transform does not take
        narrow = GraphSAGE(1, 64, 16, True, agg).to(dev).train()
        assert type(one(narrow)[0].grad_fn).__name__ == OLD
        # pre-gathered tensors
        y, _ = net(table[cidx], [], table[idx], [], None, None, None, None, None)
        assert type(y.grad_fn).__name__ == OLD
    # a fan-out of 300 does not fit the byte: MAXPOOL keeps the previous path, MEAN has no byte
    wide = torch.from_numpy(rng.integers(0, n, (50, 300))).to(dev)
    for agg, want in (("MAXPOOL", OLD), ("MEAN", FUSED)):
        net = GraphSAGE(1, 64, 128, True, agg).to(dev).train()
        y, _ = net(Gathered(table, cidx, True), [], Gathered(table, wide, True), [], None, None,
                   None, None, None)
        assert type(y.grad_fn).__name__ == want, agg
    # gcn + MAX fails in the reference itself (Linear over int64 indices): as it does today
    mx = GraphSAGE(1, 64, 128, True, "MAX").to(dev)
    raised = {}
    for on in (True, False):
        monkeypatch.setattr(graphsage, "SAGE_GCN_FUSED", on)
        for mode in ("train", "eval"):
            getattr(mx, mode)()
            with torch.set_grad_enabled(mode == "train"):
                with pytest.raises(RuntimeError) as e:
                    one(mx)
            raised[on, mode] = str(e.value)
    assert raised[True, "train"] == raised[False, "train"]
    assert raised[True, "eval"] == raised[False, "eval"]
