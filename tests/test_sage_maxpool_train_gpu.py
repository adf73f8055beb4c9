"""The MAXPOOL GraphSAGE training layer on the GPU: the concat gather that records the winner
(ops.sage_gather_concat_arg), the masked adjoint (ops.sage_scatter_concat_maxpool) and the
autograd function over them (graphsage._SageMaxPoolTrainLayerFn), wired into GraphSAGE.forward.

The forward is compared bit for bit with the kernels it fuses (the centre rows, 'MAXPOOL' values,
'MAX' indices) and with torch.argmax on the CPU; the scatter with numpy's float64 np.add.at over
the same maps and winners (rtol 1e-4, atol 1e-5 max|ref|, test_sage_train_gpu.close_sum); the
layer and the model step with a float64 CPU restatement that takes its own maxima, on inputs the
REFERENCE shows to be away from every kink (a top-two gap or a pre-activation near zero), at the
project's gradient tolerance (test_sage_train_gpu.close).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAP = 1e-3    # a (row, feature) top-two gap of at least GAP max|candidates' table|
KINK = 1e-4   # a pre-activation of at least KINK max|pre|


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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------ forward, bit-exact
N_TABLE = 400


@functools.lru_cache(maxsize=None)
def _fwd_table(F):
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


def _fwd_maps(M, k, seed):
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


def _check_forward(dev, F, k, M, bf16):
    from graphneuralnetwork_amd import ops
    t_np = _fwd_table(F)
    cidx, idx = _fwd_maps(M, k, 7 * F + k + M)
    table = torch.from_numpy(t_np).to(dev)
    if bf16:
        table = table.bfloat16()
        assert np.array_equal(table.float().cpu().numpy(), t_np, equal_nan=True)
    ci, ix = torch.from_numpy(cidx).to(dev), torch.from_numpy(idx).to(dev)
    r = ops.sage_gather_concat_arg(table, ci, ix)
    assert r is not None
    buf, arg = r
    assert buf.shape == (M, 2 * F) and buf.dtype == torch.float32
    assert arg.shape == (M, F) and arg.dtype == torch.uint8
    buf_np, arg_np = buf.cpu().numpy(), arg.cpu().numpy()
    # centre half: table[cidx], widened (bit for bit, NaNs included)
    assert np.array_equal(_bits(buf_np[:, :F]), _bits(t_np[cidx]))
    # value half == the MAXPOOL kernel's (NaN == NaN; +0.0 == -0.0)
    pool = ops.sage_gather_concat(table, ci, ix, "MAXPOOL").cpu().numpy()
    assert np.array_equal(buf_np[:, F:], pool[:, F:], equal_nan=True)
    assert np.array_equal(np.isnan(buf_np[:, F:]), np.isnan(pool[:, F:]))
    # arg == the argmax kernel's, and torch.argmax's on the CPU (first maximum, a NaN first)
    amax = ops.sage_gather_aggregate(table, ix, "MAX").cpu().numpy()
    assert amax.max() < k
    assert np.array_equal(arg_np, amax.astype(np.uint8))
    cpu = torch.argmax(torch.from_numpy(t_np)[torch.from_numpy(idx)], dim=1).numpy()
    assert np.array_equal(arg_np.astype(np.int64), cpu)
    # the stored value is the value AT the stored slot, bit for bit
    rows = np.take_along_axis(idx, arg_np.astype(np.int64), 1)
    at = t_np[rows, np.arange(F)[None, :]]
    assert np.array_equal(_bits(buf_np[:, F:]), _bits(at))
    return buf_np, arg_np, idx


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 10, 25, 255])
@pytest.mark.parametrize("F", [8, 64, 128])
def test_forward_is_bit_exact(dev, F, k, bf16):
    M = 203  # not a multiple of the 4 waves of a workgroup
    buf, arg, idx = _check_forward(dev, F, k, M, bf16)
    if k >= 10:
        r = M // 4   # slots 3 (odd columns), 6 (all), 8 (even columns) hold NaNs
        assert np.isnan(buf[r, F:]).all()
        assert (arg[r, 1::2] == 3).all() and (arg[r, 0::2] == 6).all()
    if k >= 2:       # +0.0 ties -0.0: the first slot wins unless a later one is larger
        for r in (M // 2, M // 3):
            t = _fwd_table(F)[idx[r]]
            assert (arg[r][t.max(0) == 0] == 0).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_forward_single_row(dev, bf16):
    for F, k in ((8, 1), (64, 10), (128, 255)):
        _check_forward(dev, F, k, 1, bf16)


def test_forward_declines_what_it_does_not_cover(dev):
    from graphneuralnetwork_amd import ops
    ci = torch.zeros(5, dtype=torch.int64, device=dev)
    t = torch.zeros((9, 64), device=dev)
    assert ops.sage_gather_concat_arg(t, ci, torch.zeros((5, 256), dtype=torch.int64,
                                                         device=dev)) is None     # k = 256
    ix = torch.zeros((5, 3), dtype=torch.int64, device=dev)
    assert ops.sage_gather_concat_arg(torch.zeros((9, 36), device=dev), ci, ix) is None  # F = 36
    assert ops.sage_gather_concat_arg(torch.zeros((9, 4), device=dev).bfloat16(), ci, ix) is None
    assert ops.sage_gather_concat_arg(t, ci, ix) is not None
    with pytest.raises(IndexError):  # an out-of-range index raises, as in the other gathers
        ops.sage_gather_concat_arg(t, ci, ix + 9)


# ------------------------------------------------------------------ the scatter
def _ref_scatter(d, cidx, idx, arg, n_prev):
    """numpy float64 np.add.at over the same maps and winners."""
    F = d.shape[1] // 2
    d64 = np.asarray(d, np.float64)
    out = np.zeros((n_prev, F))
    np.add.at(out, cidx, d64[:, :F])
    rows = np.take_along_axis(idx, arg.astype(np.int64), 1)              # [M, F] targets
    np.add.at(out, (rows, np.broadcast_to(np.arange(F), rows.shape)), d64[:, F:])
    return out


def _run_scatter(dev, dbuf_t, arg_t, cidx, idx, n_prev):
    from graphneuralnetwork_amd import ops
    tr = ops.sage_maps_transpose(torch.from_numpy(cidx).to(dev), torch.from_numpy(idx).to(dev),
                                 n_prev)
    # unreferenced rows must be WRITTEN as zeros, not left as they were
    out = torch.full((n_prev, dbuf_t.shape[1] // 2), float("nan"), device=dev)
    dx = ops.sage_scatter_concat_maxpool(dbuf_t, arg_t, tr, n_prev, out=out)
    assert dx is out
    return dx, tr


def _maps(rng, M, k, n_prev):
    hi = max(1, n_prev // 2)  # the upper half of the targets is never referenced
    idx = rng.integers(0, hi, (M, k)).astype(np.int64)
    cidx = rng.integers(0, max(1, hi // 3), M).astype(np.int64)
    return cidx, idx


@pytest.mark.parametrize("F", [128, 64, 8])
@pytest.mark.parametrize("k", [1, 10, 25])
@pytest.mark.parametrize("padded", [False, True])
def test_scatter_vs_float64(dev, F, k, padded):
    rng = np.random.default_rng(F + k)
    M, n_prev = 1003, 700
    cidx, idx = _maps(rng, M, k, n_prev)
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    arg = rng.integers(0, k, (M, F)).astype(np.uint8)  # independent of any forward
    dt, at = torch.from_numpy(d).to(dev), torch.from_numpy(arg).to(dev)
    if padded:  # column-padded views: row strides 2F + 8 floats and F + 4 bytes
        wide = torch.full((M, 2 * F + 8), float("nan"), device=dev)
        wide[:, :2 * F] = dt
        dt = wide[:, :2 * F]
        wa = torch.full((M, F + 4), 255, dtype=torch.uint8, device=dev)
        wa[:, :F] = at
        at = wa[:, :F]
        assert dt.stride(0) == 2 * F + 8 and at.stride(0) == F + 4
    dx, _ = _run_scatter(dev, dt, at, cidx, idx, n_prev)
    assert dx.shape == (n_prev, F) and dx.dtype == torch.float32
    got = dx.cpu().numpy()
    assert not np.isnan(got).any()
    assert (got[n_prev // 2:] == 0).all()  # nobody references the upper half: written as zeros
    close_sum(got, _ref_scatter(d, cidx, idx, arg, n_prev), f"scatter F={F} k={k}")


def _hub_case(rng, M=300, k=3, F=128):
    """One target referenced by every one of the M (k + 1) slots: the chunk path."""
    cidx = np.ones(M, np.int64)
    idx = np.ones((M, k), np.int64)
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    arg = rng.integers(0, k, (M, F)).astype(np.uint8)
    return d, arg, cidx, idx, 3


def test_scatter_one_target_takes_every_slot(dev):
    d, arg, cidx, idx, n_prev = _hub_case(np.random.default_rng(11))
    dx, tr = _run_scatter(dev, torch.from_numpy(d).to(dev), torch.from_numpy(arg).to(dev), cidx,
                          idx, n_prev)
    assert tr.ptr.tolist() == [0, 0, 1200, 1200]
    got = dx.cpu().numpy()
    assert (got[0] == 0).all() and (got[2] == 0).all()
    close_sum(got, _ref_scatter(d, arg=arg, cidx=cidx, idx=idx, n_prev=n_prev), "hub")


@pytest.mark.parametrize("slots", [256, 257])
def test_scatter_list_at_the_chunk_length(dev, slots):
    """A list of exactly 256 slots (the last one summed by one lane group) and one of 257 (the
    first one cut into chunks)."""
    rng = np.random.default_rng(slots)
    k, F = 3, 64
    M = 64 if slots == 256 else 65
    cidx = np.zeros(M, np.int64)
    idx = np.zeros((M, k), np.int64)
    idx[64:] = 1  # M = 65: 65 centre + 192 neighbour slots on target 0, 3 on target 1
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    arg = rng.integers(0, k, (M, F)).astype(np.uint8)
    dx, tr = _run_scatter(dev, torch.from_numpy(d).to(dev), torch.from_numpy(arg).to(dev), cidx,
                          idx, 2)
    assert int(tr.ptr[1]) == slots
    close_sum(dx.cpu().numpy(), _ref_scatter(d, cidx, idx, arg, 2), f"{slots} slots")


def test_scatter_selects_and_never_multiplies(dev):
    """A NaN / Inf gradient reaches the target of the slot that won it and nobody else: the
    targets of the slots that did not win stay finite and equal to the float64 sum."""
    rng = np.random.default_rng(13)
    M, k, F, n_prev = 500, 10, 64, 6000
    cidx = rng.integers(0, n_prev, M).astype(np.int64)
    idx = np.stack([rng.permutation(n_prev)[:k] for _ in range(M)]).astype(np.int64)  # distinct
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    arg = rng.integers(0, k, (M, F)).astype(np.uint8)
    d[401, F + 9] = np.nan
    d[17, F + 5] = np.inf
    d[17, F + 6] = -np.inf
    d[33, 2] = np.nan          # the centre half has no mask: it reaches cidx[33]
    dx, _ = _run_scatter(dev, torch.from_numpy(d).to(dev), torch.from_numpy(arg).to(dev), cidx,
                         idx, n_prev)
    got = dx.cpu().numpy()
    nan_at = np.zeros((n_prev, F), bool)
    nan_at[idx[401, arg[401, 9]], 9] = True
    nan_at[cidx[33], 2] = True
    pinf = np.zeros((n_prev, F), bool)
    pinf[idx[17, arg[17, 5]], 5] = True
    ninf = np.zeros((n_prev, F), bool)
    ninf[idx[17, arg[17, 6]], 6] = True
    assert np.array_equal(np.isnan(got), nan_at)
    assert np.array_equal(np.isposinf(got), pinf & ~nan_at)
    assert np.array_equal(np.isneginf(got), ninf & ~nan_at)
    # the slots of (401, 9), (17, 5), (17, 6) that did not win: finite, the sum without them
    ref = _ref_scatter(d, cidx, idx, arg, n_prev)
    for m, f in ((401, 9), (17, 5), (17, 6)):
        losers = np.delete(idx[m], arg[m, f])
        assert np.isfinite(got[losers, f]).all() and np.isfinite(ref[losers, f]).all()
    fin = ~(nan_at | pinf | ninf)
    assert np.isfinite(ref[fin]).all()
    close_sum(got[fin], ref[fin], "finite rest")


def test_scatter_is_deterministic(dev):
    from graphneuralnetwork_amd import _lib
    d, arg, cidx, idx, n_prev = _hub_case(np.random.default_rng(12))
    dt, at = torch.from_numpy(d).to(dev), torch.from_numpy(arg).to(dev)
    a, tr = _run_scatter(dev, dt, at, cidx, idx, n_prev)
    a = a.clone()
    b, _ = _run_scatter(dev, dt, at, cidx, idx, n_prev)
    assert torch.equal(a, b)
    # the same maps, a workspace full of garbage: the entry itself clears what it reads
    lib = _lib.load()
    M, k, F = tr.M, tr.k, d.shape[1] // 2
    nbytes = int(lib.gnn_sage_scatter_concat_maxpool_workspace_bytes(M, k, F))
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
    c = torch.full((n_prev, F), float("nan"), device=dev)
    _lib.check(lib.gnn_sage_scatter_concat_maxpool_f32(
        dt.data_ptr(), 2 * F, at.data_ptr(), F, tr.ptr.data_ptr(), tr.slot.data_ptr(), M, k, F,
        n_prev, c.data_ptr(), F, ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
        "gnn_sage_scatter_concat_maxpool_f32")
    assert torch.equal(a, c)
    close_sum(a.cpu().numpy(), _ref_scatter(d, cidx, idx, arg, n_prev), "hub, deterministic")
    # a mixed case: hubs past the chunk length among many short lists
    rng = np.random.default_rng(14)
    M2, k2, n2 = 3000, 10, 2000
    c2, i2 = _maps(rng, M2, k2, n2)
    i2[rng.random((M2, k2)) < 0.3] = 7
    d2 = torch.from_numpy(rng.standard_normal((M2, 128)).astype(np.float32)).to(dev)
    a2 = torch.from_numpy(rng.integers(0, k2, (M2, 64)).astype(np.uint8)).to(dev)
    x, _ = _run_scatter(dev, d2, a2, c2, i2, n2)
    x = x.clone()
    y, _ = _run_scatter(dev, d2, a2, c2, i2, n2)
    assert torch.equal(x, y)


def test_scatter_declines_what_it_does_not_cover(dev):
    from graphneuralnetwork_amd import ops
    rng = np.random.default_rng(15)
    cidx, idx = _maps(rng, 50, 3, 40)
    tr = ops.sage_maps_transpose(torch.from_numpy(cidx).to(dev), torch.from_numpy(idx).to(dev), 40)
    u8 = functools.partial(torch.zeros, dtype=torch.uint8, device=dev)
    assert ops.sage_scatter_concat_maxpool(torch.zeros((50, 72), device=dev), u8((50, 36)), tr,
                                           40) is None   # F = 36
    wide = u8((50, 11))
    assert ops.sage_scatter_concat_maxpool(torch.zeros((50, 16), device=dev), wide[:, :8], tr,
                                           40) is None   # rows of arg not whole words
    c3, i3 = _maps(rng, 5, 256, 40)
    tr3 = ops.sage_maps_transpose(torch.from_numpy(c3).to(dev), torch.from_numpy(i3).to(dev), 40)
    assert ops.sage_scatter_concat_maxpool(torch.zeros((5, 16), device=dev), u8((5, 8)), tr3,
                                           40) is None   # k = 256


# ------------------------------------------------------------------ kinks of the reference
def _settle(run, redraw, tries=400):
    """test_model_grads_gpu._settle: run() -> [(stage, name, per-column smallest distance,
    bound)]; redraw(stage, name, columns) redraws what owns the columns whose distance is below
    the bound, earliest stage first. Fails if the fixture does not settle."""
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


def _gap(table, idx, zero_sets_ok=False):
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


# ------------------------------------------------------------------ the layer
def _ref_layer(table, W, cidx, idx):
    buf = torch.cat([table[cidx], table[idx].max(dim=1).values], dim=1)
    pre = buf @ W.t()
    return pre, torch.relu(pre)


@functools.lru_cache(maxsize=None)
def _layer_fixture():
    """F, H = 64, 128; M = 200, k = 5, n_prev = 300: a bf16-representable table and a weight
    whose float64 forward is away from kinks, and the float64 gradients of sum(y * G)."""
    F, H, M, k, n_prev = 64, 128, 200, 5, 300
    gen = torch.Generator().manual_seed(41)
    rng = np.random.default_rng(41)
    cidx = torch.from_numpy(rng.integers(0, n_prev, M))
    idx = torch.from_numpy(rng.integers(0, n_prev, (M, k)))
    table = _bf16_normal(gen, n_prev, F)
    W = _uniform(gen, (2 * F) ** -0.5, H, 2 * F)
    G = torch.randn(M, H, generator=gen)

    def run():
        t, w = table.double(), W.double()
        pre, _ = _ref_layer(t, w, cidx, idx)
        return [(0, "table", _gap(t, idx), GAP * float(t.abs().max())),
                (1, "W", pre.abs().min(dim=0).values, KINK * float(pre.abs().max()))]

    def redraw(stage, name, cols):
        if stage == 0:
            table[:, cols] = _bf16_normal(gen, n_prev, len(cols))
        else:
            W[cols] = _uniform(gen, (2 * F) ** -0.5, len(cols), 2 * F)

    _assert_kinks(_settle(run, redraw), "layer")  # on the CPU, before anything runs on the device
    t64, w64 = table.double().requires_grad_(), W.double().requires_grad_()
    _, y = _ref_layer(t64, w64, cidx, idx)
    (y * G.double()).sum().backward()
    return dict(table=table, W=W, cidx=cidx, idx=idx, G=G, y=y.detach().numpy(),
                dW=w64.grad.numpy(), dT=t64.grad.numpy())


@pytest.mark.parametrize("kind", ["fp32_grad", "fp32", "bf16"])
def test_layer_gradients_vs_float64(dev, kind):
    from graphneuralnetwork_amd.graphsage import _SageMaxPoolTrainLayerFn
    fx = _layer_fixture()
    t = fx["table"].to(dev)
    t = t.bfloat16() if kind == "bf16" else t.requires_grad_(kind == "fp32_grad")
    W = fx["W"].to(dev).requires_grad_()
    y = _SageMaxPoolTrainLayerFn.apply(t, W, fx["cidx"].to(dev), fx["idx"].to(dev))
    (y * fx["G"].to(dev)).sum().backward()
    close(y.detach().cpu().numpy(), fx["y"], what=f"{kind} y")
    close(W.grad.cpu().numpy(), fx["dW"], what=f"{kind} dW")
    if kind == "fp32_grad":
        close(t.grad.cpu().numpy(), fx["dT"], what="d table")
        assert np.abs(fx["dT"]).max() > 0
    else:
        assert t.grad is None


def test_layer_refuses_a_bf16_table_that_requires_grad(dev):
    from graphneuralnetwork_amd.graphsage import GraphSAGE, Gathered
    fx = _layer_fixture()
    t = fx["table"].to(dev).bfloat16().requires_grad_()
    net = GraphSAGE(1, 64, 128, False, "MAXPOOL").to(dev).train()
    with pytest.raises(TypeError, match="bfloat16"):
        net(Gathered(t, fx["cidx"].to(dev), True), [], Gathered(t, fx["idx"].to(dev), True), [],
            None, None, None, None, None)


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
        return sample_unsupervised_batch(adj, seeds[:8].to(adj.device), (5, 3), window=2, K=2,
                                         seed=3)
    return sample_batch(adj, seeds.to(adj.device), (5, 3), seed=3)


W0, W1 = "sage_blocks.sage_layer0.weight.weight", "sage_blocks.sage_layer1.weight.weight"


def _ref_tower(P, table, b, agg="MAXPOOL", rec=None):
    """GraphSAGE.forward, one branch (GraphSAGE/GraphSAGE.py:42-57 with torch.max(...).values or
    torch.mean as the aggregate), on the CPU in the dtype of its arguments. rec: a list that
    receives the kink distances of every maximum and pre-activation."""
    ci, ni = b.frontier.cpu(), b.frontier_nbrs.cpu()
    src, feats = table, None
    L = len(b.center_maps) + 1
    for i in range(L):
        nf = src[ni]
        agg_f = nf.max(dim=1).values if agg == "MAXPOOL" else nf.mean(dim=1)
        pre = torch.cat([src[ci], agg_f], dim=1) @ P[f"sage_blocks.sage_layer{i}.weight.weight"].t()
        feats = torch.relu(pre)
        if rec is not None:
            mx = float(src.abs().max())
            rec.append((2 * i, f"max{i}", _gap(src, ni, zero_sets_ok=i > 0), GAP * mx))
            rec.append((2 * i + 1, f"pre{i}", pre.abs().min(dim=0).values,
                        KINK * float(pre.abs().max())))
        if i != L - 1:
            src, ci, ni = feats, b.center_maps[i].cpu(), b.neigh_maps[i].cpu()
    return feats


def _loss(unsup, second, labels):
    if unsup:
        return torch.nn.functional.binary_cross_entropy_with_logits(
            second.squeeze(1), labels.to(second.dtype))
    return torch.nn.functional.cross_entropy(second, labels)


def _ref_forward(P, table, batch, unsup, labels, agg="MAXPOOL", rec=None):
    if unsup:
        emb = _ref_tower(P, table, batch.center, agg, rec)
        ctx = _ref_tower(P, table, batch.context, agg, rec).reshape(*labels.shape, -1)
        second = torch.bmm(emb.unsqueeze(1), ctx.permute(0, 2, 1))
    else:
        emb = _ref_tower(P, table, batch, agg, rec)
        second = emb @ P["dense.weight"].t() + P["dense.bias"]
    return emb, second


@functools.lru_cache(maxsize=None)
def _model_fixture(unsup):
    """The parameters of GraphSAGE(2, 64, 128, False, 'MAXPOOL'), a bf16-representable table and
    labels such that the float64 forward is away from kinks (asserted here, on the CPU), and the
    float64 step: output, loss and every gradient."""
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    n, F, H = _graph()[0], 64, 128
    batch = _batch(unsup)
    gen = torch.Generator().manual_seed(51 + unsup)
    torch.manual_seed(0)
    net = GraphSAGE(2, F, H, False, "MAXPOOL", Unsupervised=unsup, class_size=None if unsup else 7)
    P = {k_: v.detach().clone() for k_, v in net.named_parameters()}
    table = _bf16_normal(gen, n, F)
    labels = (batch.labels.cpu() if unsup else
              torch.from_numpy(np.random.default_rng(52).integers(0, 7, 40)))

    def run():
        rec = []
        _ref_forward({k_: v.double() for k_, v in P.items()}, table.double(), batch, unsup, labels,
                     rec=rec)
        return rec

    def redraw(stage, name, cols):
        if stage == 0:    # a maximum over table rows: the table's columns
            table[:, cols] = _bf16_normal(gen, n, len(cols))
        elif stage <= 2:  # a layer-0 pre-activation, or a maximum over layer 0's output
            P[W0][cols] = _uniform(gen, (2 * F) ** -0.5, len(cols), 2 * F)
        else:
            P[W1][cols] = _uniform(gen, (2 * H) ** -0.5, len(cols), 2 * H)

    _assert_kinks(_settle(run, redraw), "unsupervised" if unsup else "supervised")
    P64 = {k_: v.double().requires_grad_() for k_, v in P.items()}
    t64 = table.double().requires_grad_()
    emb, second = _ref_forward(P64, t64, batch, unsup, labels)
    loss = _loss(unsup, second, labels)
    loss.backward()
    ref = {"emb": emb.detach().numpy(), "second": second.detach().numpy(),
           "loss": loss.detach().numpy(), "table": t64.grad.numpy()}
    ref.update({k_: v.grad.numpy() for k_, v in P64.items()})
    return P, table, labels, ref


def _gpu_step(net, table, batch, unsup, labels):
    net.zero_grad()
    with torch.enable_grad():
        args = batch.forward_args(table)
        if not unsup:
            args = (*args, None, None, None, None, None)
        emb, second = net(*args)
        loss = _loss(unsup, second, labels)
        loss.backward()
    out = {"emb": emb.detach().cpu().numpy(), "second": second.detach().cpu().numpy(),
           "loss": loss.detach().cpu().numpy()}
    if table.requires_grad:
        out["table"] = table.grad.cpu().numpy().copy()
    out.update({k_: p.grad.cpu().numpy().copy() for k_, p in net.named_parameters()})
    return out, emb.grad_fn


def _net(dev, unsup, P, agg="MAXPOOL"):
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    net = GraphSAGE(2, 64, 128, False, agg, Unsupervised=unsup, class_size=None if unsup else 7)
    net.load_state_dict(P)
    return net.to(dev).train()


FUSED, OLD = "_SageMaxPoolTrainLayerFnBackward", "ReluBackward0"


@pytest.mark.parametrize("unsup", [False, True], ids=["supervised", "unsupervised"])
def test_model_step(dev, monkeypatch, unsup):
    from graphneuralnetwork_amd import graphsage
    P, table, labels, ref = _model_fixture(unsup)
    batch, labels_d = _batch(unsup), labels.to(dev)
    net = _net(dev, unsup, P)
    layer_fns = []
    real = graphsage._sage_train_layer

    def seen(*a, **k):
        y = real(*a, **k)
        layer_fns.append(None if y is None else type(y.grad_fn).__name__)
        return y

    monkeypatch.setattr(graphsage, "_sage_train_layer", seen)
    towers = 2 if unsup else 1
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(graphsage, "SAGE_TRAIN_FUSED_MAXPOOL", fused)
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
            close(on, ref[name], what=f"{kind} {name}: switch on vs float64")
            close(on, off, what=f"{kind} {name}: switch on vs off")
    assert np.abs(ref["table"]).max() > 0
    for name in P:
        assert np.abs(ref[name]).max() > 0, name


def test_model_step_when_the_scatter_declines(dev, monkeypatch):
    """A None from sage_scatter_concat_maxpool inside the layer's backward drops that gradient to
    the torch formulation of the same masked sum: same numbers."""
    from graphneuralnetwork_amd import graphsage
    P, table, labels, ref = _model_fixture(False)
    monkeypatch.setattr(graphsage, "SAGE_TRAIN_FUSED_MAXPOOL", True)
    net = _net(dev, False, P)
    asked = []
    monkeypatch.setattr(graphsage, "sage_scatter_concat_maxpool",
                        lambda *a, **k: asked.append(1))  # returns None
    t = table.to(dev).requires_grad_()
    run, fn = _gpu_step(net, t, _batch(False), False, labels.to(dev))
    assert len(asked) == 2 and type(fn).__name__ == FUSED
    for name in run:
        close(run[name], ref[name], what=f"{name}: scatter declined vs float64")


def test_other_layers_keep_their_paths(dev, monkeypatch):
    from graphneuralnetwork_amd import graphsage
    from graphneuralnetwork_amd.graphsage import GraphSAGE, Gathered
    monkeypatch.setattr(graphsage, "SAGE_TRAIN_FUSED_MAXPOOL", True)
    P, table, labels, _ = _model_fixture(False)
    # MEAN batches: the MEAN function, whatever the new switch says
    net = _net(dev, False, P, agg="MEAN")
    _, fn = _gpu_step(net, table.to(dev), _batch(False), False, labels.to(dev))
    assert type(fn).__name__ == "_SageTrainLayerFnBackward"
    # a fan-out of 300 does not fit the byte: the previous path (relu of torch's addmm)
    rng = np.random.default_rng(61)
    t = table.to(dev)
    cidx = torch.from_numpy(rng.integers(0, t.shape[0], 50)).to(dev)
    one = GraphSAGE(1, 64, 128, False, "MAXPOOL").to(dev).train()
    for k, want in ((255, FUSED), (300, OLD)):
        idx = torch.from_numpy(rng.integers(0, t.shape[0], (50, k))).to(dev)
        y, _ = one(Gathered(t, cidx, True), [], Gathered(t, idx, True), [], None, None, None,
                   None, None)
        assert type(y.grad_fn).__name__ == want, k
    # untrusted maps, and MAX (argmax indices as features), keep the previous path too
    idx = torch.from_numpy(rng.integers(0, t.shape[0], (50, 5))).to(dev)
    y, _ = one(Gathered(t, cidx, False), [], Gathered(t, idx, False), [], None, None, None, None,
               None)
    assert type(y.grad_fn).__name__ == OLD
    mx = GraphSAGE(1, 64, 128, False, "MAX").to(dev).train()
    y, _ = mx(Gathered(t, cidx, True), [], Gathered(t, idx, True), [], None, None, None, None,
              None)
    assert type(y.grad_fn).__name__ == OLD
