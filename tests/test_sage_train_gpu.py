"""The GraphSAGE training layer on the GPU: the device-built transposed maps
(ops.sage_maps_transpose), the adjoint of the concat gather (ops.sage_scatter_concat) and the
autograd function that uses them (graphsage._SageTrainLayerFn), wired into GraphSAGE.forward.

The builder is compared bit for bit with numpy's stable argsort; the scatter with a float64
index_add_ over the same maps (rtol 1e-4, atol 1e-5 max|ref|); the model step with the switch
graphsage.SAGE_TRAIN_FUSED off (the separate gathers and torch's linear + addmm + relu) and with
a float64 CPU restatement of the reference forward (GraphSAGE/GraphSAGE.py:42-57) under
autograd, at the project's gradient tolerance (test_sage_bf16_gpu.close).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def close(a, b, rtol=1e-4, what=""):  # test_sage_bf16_gpu.close
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if b.size else 1.0
    err = float(np.nanmax(np.abs(a - b))) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-5 * scale, err_msg=what)


def close_sum(a, b, what=""):
    """The scatter against float64: rtol 1e-4, atol 1e-5 max|ref| (no floor at 1)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * scale, err_msg=what)


# ------------------------------------------------------------------ the transposed maps
def _np_transpose(cidx, idx, n_prev):
    tgt = np.concatenate([cidx.reshape(-1), idx.reshape(-1)])
    slot = np.argsort(tgt, kind="stable").astype(np.int32)
    ptr = np.zeros(n_prev + 1, np.int64)
    np.cumsum(np.bincount(tgt, minlength=n_prev), out=ptr[1:])
    return ptr, slot


def _maps(rng, M, k, n_prev, repeats=False, hole=False):
    hi = max(1, n_prev // 2) if hole else n_prev  # hole: the upper half is never referenced
    idx = rng.integers(0, hi, (M, k))
    cidx = rng.integers(0, max(1, hi // 3), M) if repeats else rng.permutation(max(hi, M))[:M] % hi
    return cidx.astype(np.int64), idx.astype(np.int64)


def _check_transpose(dev, cidx, idx_t, n_prev):
    from graphneuralnetwork_amd import ops
    tr = ops.sage_maps_transpose(torch.from_numpy(cidx).to(dev), idx_t, n_prev)
    ptr, slot = _np_transpose(cidx, idx_t.cpu().numpy(), n_prev)
    assert (tr.M, tr.k) == tuple(idx_t.shape)
    assert tr.ptr.dtype == torch.int64 and tr.slot.dtype == torch.int32
    assert np.array_equal(tr.ptr.cpu().numpy(), ptr)
    assert np.array_equal(tr.slot.cpu().numpy(), slot)


@pytest.mark.parametrize("M,k,n_prev", [(1, 1, 1), (7, 3, 5), (300, 25, 64), (1000, 10, 4096)])
@pytest.mark.parametrize("repeats", [False, True])
def test_transpose_is_bit_exact(dev, M, k, n_prev, repeats):
    rng = np.random.default_rng(M + 7 * k)
    cidx, idx = _maps(rng, M, k, n_prev, repeats=repeats)
    _check_transpose(dev, cidx, torch.from_numpy(idx).to(dev), n_prev)


def test_transpose_unreferenced_targets_one_segment_and_strided_maps(dev):
    rng = np.random.default_rng(5)
    cidx, idx = _maps(rng, 200, 10, 512, repeats=True, hole=True)
    assert idx.max() < 256  # targets 256.. have no slot
    _check_transpose(dev, cidx, torch.from_numpy(idx).to(dev), 512)
    # n_prev = 1: every slot in one segment
    z = np.zeros((333, 4), np.int64)
    _check_transpose(dev, z[:, 0].copy(), torch.from_numpy(z).to(dev), 1)
    # a strided [M, k] view of a wider buffer (the sampler's maps are pieces of one buffer)
    wide = torch.from_numpy(rng.integers(0, 512, (200, 16))).to(dev)
    view = wide[:, 3:13]
    assert view.stride(0) == 16 and not view.is_contiguous()
    _check_transpose(dev, cidx, view, 512)


def test_transpose_of_no_rows_and_bad_indices(dev):
    from graphneuralnetwork_amd import ops
    e1 = torch.empty(0, dtype=torch.int64, device=dev)
    tr = ops.sage_maps_transpose(e1, torch.empty((0, 5), dtype=torch.int64, device=dev), 9)
    assert tr.M == 0 and tr.k == 5 and tr.slot.numel() == 0
    assert tr.ptr.shape == (10,) and int(tr.ptr.abs().sum()) == 0
    cidx = torch.tensor([0, 1, 2], device=dev)
    idx = torch.tensor([[0, 1], [2, 3], [1, 0]], device=dev)
    for bad in (4, -1):  # == n_prev, and the reference's padding value
        b = idx.clone()
        b[1, 1] = bad
        with pytest.raises(IndexError):
            ops.sage_maps_transpose(cidx, b, 4)
        c = cidx.clone()
        c[2] = bad
        with pytest.raises(IndexError):
            ops.sage_maps_transpose(c, idx, 4)
    # unchecked: the flawed slot lies past ptr[n_prev], the scatter never reads it
    b = idx.clone()
    b[1, 1] = 4
    tr = ops.sage_maps_transpose(cidx, b, 4, check=False)
    assert int(tr.ptr[-1]) == 8
    g = torch.ones((3, 8), device=dev)
    dx = ops.sage_scatter_concat(g, tr, 4)
    want = np.zeros((4, 4))
    for t in cidx.tolist():
        want[t] += 1.0
    for t in b.flatten().tolist():
        if t < 4:
            want[t] += 0.5
    close_sum(dx.cpu().numpy(), want, "flawed slot skipped")


# ------------------------------------------------------------------ the scatter
def _ref_scatter(dbuf, cidx, idx, n_prev):
    """float64 index_add_ on the same maps."""
    M, k = idx.shape
    F = dbuf.shape[1] // 2
    d = torch.from_numpy(np.asarray(dbuf, np.float64))
    out = torch.zeros((n_prev, F), dtype=torch.float64)
    out.index_add_(0, torch.from_numpy(cidx), d[:, :F])
    out.index_add_(0, torch.from_numpy(idx.reshape(-1)),
                   (d[:, F:] / k).repeat_interleave(k, dim=0))
    return out.numpy()


def _run_scatter(dev, dbuf_t, cidx, idx, n_prev, prefill=True):
    from graphneuralnetwork_amd import ops
    tr = ops.sage_maps_transpose(torch.from_numpy(cidx).to(dev), torch.from_numpy(idx).to(dev),
                                 n_prev)
    out = None
    if prefill:  # unreferenced rows must be WRITTEN as zeros, not left as they were
        out = torch.full((n_prev, dbuf_t.shape[1] // 2), float("nan"), device=dev)
    dx = ops.sage_scatter_concat(dbuf_t, tr, n_prev, out=out)
    assert out is None or dx is out
    return dx, tr


@pytest.mark.parametrize("F", [128, 64, 8])
@pytest.mark.parametrize("k", [1, 10, 25])
@pytest.mark.parametrize("padded", [False, True])
def test_scatter_vs_float64(dev, F, k, padded):
    rng = np.random.default_rng(F + k)
    M, n_prev = 1003, 700
    cidx, idx = _maps(rng, M, k, n_prev, repeats=True, hole=True)
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    dt = torch.from_numpy(d).to(dev)
    if padded:  # a column-padded view: row stride 2F + 8
        wide = torch.full((M, 2 * F + 8), float("nan"), device=dev)
        wide[:, :2 * F] = dt
        dt = wide[:, :2 * F]
        assert dt.stride(0) == 2 * F + 8
    dx, _ = _run_scatter(dev, dt, cidx, idx, n_prev)
    assert dx.shape == (n_prev, F) and dx.dtype == torch.float32
    got = dx.cpu().numpy()
    assert not np.isnan(got).any()
    assert (got[n_prev // 2:] == 0).all()  # nobody references the upper half: written as zeros
    close_sum(got, _ref_scatter(d, cidx, idx, n_prev), f"scatter F={F} k={k}")


def _hub_case(rng, F=128):
    M, k, n_prev = 4096, 25, 3  # one target referenced by every slot: far beyond one chunk
    cidx = np.ones(M, np.int64)
    idx = np.ones((M, k), np.int64)
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    return d, cidx, idx, n_prev


def test_scatter_one_target_takes_every_slot(dev):
    d, cidx, idx, n_prev = _hub_case(np.random.default_rng(11))
    dx, tr = _run_scatter(dev, torch.from_numpy(d).to(dev), cidx, idx, n_prev)
    assert tr.ptr.tolist() == [0, 0, 4096 * 26, 4096 * 26]
    got = dx.cpu().numpy()
    assert (got[0] == 0).all() and (got[2] == 0).all()
    close_sum(got, _ref_scatter(d, cidx, idx, n_prev), "hub")


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
    dx, tr = _run_scatter(dev, torch.from_numpy(d).to(dev), cidx, idx, 2)
    assert int(tr.ptr[1]) == slots
    close_sum(dx.cpu().numpy(), _ref_scatter(d, cidx, idx, 2), f"{slots} slots")


def test_scatter_is_deterministic(dev):
    rng = np.random.default_rng(12)
    d, cidx, idx, n_prev = _hub_case(rng)
    # a mixed case: a few hubs past the chunk length among many short lists
    M2, k2, n2 = 3000, 10, 2000
    c2, i2 = _maps(rng, M2, k2, n2)
    i2[rng.random((M2, k2)) < 0.3] = 7
    i2[rng.random((M2, k2)) < 0.05] = 1999
    d2 = rng.standard_normal((M2, 128)).astype(np.float32)
    for dd, cc, ii, nn in ((d, cidx, idx, n_prev), (d2, c2, i2, n2)):
        t = torch.from_numpy(dd).to(dev)
        a, _ = _run_scatter(dev, t, cc, ii, nn)
        b, _ = _run_scatter(dev, t, cc, ii, nn)
        assert torch.equal(a, b)
        close_sum(a.cpu().numpy(), _ref_scatter(dd, cc, ii, nn), "deterministic case")


def test_scatter_nonfinite_reach_their_targets_only(dev):
    rng = np.random.default_rng(13)
    M, k, F, n_prev = 500, 10, 64, 300
    cidx, idx = _maps(rng, M, k, n_prev)
    d = rng.standard_normal((M, 2 * F)).astype(np.float32)
    d[17, 5] = np.nan          # centre half of row 17, column 5 -> target cidx[17]
    d[401, F + 9] = np.inf     # neighbour half of row 401, column 9 -> targets idx[401, :]
    dx, _ = _run_scatter(dev, torch.from_numpy(d).to(dev), cidx, idx, n_prev)
    got = dx.cpu().numpy()
    nan_at = np.zeros((n_prev, F), bool)
    nan_at[cidx[17], 5] = True
    inf_at = np.zeros((n_prev, F), bool)
    inf_at[idx[401], 9] = True
    inf_at &= ~nan_at
    assert np.array_equal(np.isnan(got), nan_at)
    assert np.array_equal(np.isposinf(got), inf_at)
    assert not np.isneginf(got).any()
    ref = _ref_scatter(d, cidx, idx, n_prev)
    fin = ~(nan_at | inf_at)
    close_sum(got[fin], ref[fin], "finite rest")


def test_scatter_declines_an_unsupported_width(dev):
    from graphneuralnetwork_amd import ops
    rng = np.random.default_rng(14)
    cidx, idx = _maps(rng, 50, 3, 40)
    tr = ops.sage_maps_transpose(torch.from_numpy(cidx).to(dev), torch.from_numpy(idx).to(dev), 40)
    assert ops.sage_scatter_concat(torch.zeros((50, 72), device=dev), tr, 40) is None  # F = 36
    assert ops.sage_scatter_concat(torch.zeros((50, 1024), device=dev), tr, 40) is None  # F = 512
    e = ops.sage_maps_transpose(torch.empty(0, dtype=torch.int64, device=dev),
                                torch.empty((0, 3), dtype=torch.int64, device=dev), 40)
    z = ops.sage_scatter_concat(torch.zeros((0, 16), device=dev), e, 40)  # M = 0: no launch
    assert z.shape == (40, 8) and int((z != 0).sum()) == 0


def test_scatter_past_4_gib_of_gradient_rows(dev):
    """dBuf of 4,200,000 x 256 fp32 (4.3 GB): the byte offset of its last rows passes 2^32."""
    from graphneuralnetwork_amd import ops
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory (found {free >> 30} GiB)")
    M, F, k, n_prev = 4_200_000, 128, 1, 16
    g = torch.Generator(device=dev).manual_seed(3)
    dbuf = torch.empty((M, 2 * F), device=dev)
    for r0 in range(0, M, 1 << 20):  # filled in pieces: no second 4 GB temporary
        dbuf[r0:r0 + (1 << 20)].normal_(generator=g)
    assert dbuf.numel() * 4 > 2 ** 32
    cidx = torch.arange(M, device=dev) % 14          # targets 0..13
    idx = (torch.arange(M, device=dev) % 14).view(M, 1)
    cidx[-8:] = 15                                   # the last 8 rows land alone on target 15
    idx[-8:] = 15
    cidx[:1000] = 14                                 # target 14: the first 1000 rows
    idx[:1000] = 14
    tr = ops.sage_maps_transpose(cidx, idx, n_prev, check=False)
    dx = ops.sage_scatter_concat(dbuf, tr, n_prev)
    assert dx.shape == (n_prev, F)
    want15 = (dbuf[-8:, :F].double().sum(0) + dbuf[-8:, F:].double().sum(0)).cpu().numpy()
    want14 = (dbuf[:1000, :F].double().sum(0) + dbuf[:1000, F:].double().sum(0)).cpu().numpy()
    close_sum(dx[15].cpu().numpy(), want15, "target 15 (rows past 2^32 bytes)")
    close_sum(dx[14].cpu().numpy(), want14, "target 14")


# ------------------------------------------------------------------ the model step
@functools.lru_cache(maxsize=None)
def _graph():
    from graphneuralnetwork_amd.sampler import symmetric_adjacency
    rng = np.random.default_rng(21)
    n = 2000
    s, d = rng.integers(0, n, 20000), rng.integers(0, n, 20000)
    adj = symmetric_adjacency(s, d, n, device=torch.device("cuda:0"))
    deg = (adj.rowptr[1:] - adj.rowptr[:-1]).cpu().numpy()
    return n, adj, torch.from_numpy(np.flatnonzero(deg > 0)[:40])


def _batch(unsup):
    from graphneuralnetwork_amd.sampler import sample_batch, sample_unsupervised_batch
    n, adj, seeds = _graph()
    if unsup:
        return sample_unsupervised_batch(adj, seeds.to(adj.device), (5, 3), window=2, K=2, seed=3)
    return sample_batch(adj, seeds.to(adj.device), (5, 3), seed=3)


def _ref_tower(P, table, b):
    """GraphSAGE.forward, one branch (GraphSAGE/GraphSAGE.py:42-57, MEAN), float64 on the CPU."""
    cf = table[b.frontier.cpu()]
    nf = table[b.frontier_nbrs.cpu()]
    feats = None
    L = len(b.center_maps) + 1
    for i in range(L):
        comb = torch.cat([cf, nf.mean(dim=1)], dim=1)
        feats = torch.relu(comb @ P[f"sage_blocks.sage_layer{i}.weight.weight"].t())
        if i != L - 1:
            cf = feats[b.center_maps[i].cpu()]
            nf = feats[b.neigh_maps[i].cpu()]
    return feats


def _loss(unsup, emb, second, labels):
    if unsup:
        return torch.nn.functional.binary_cross_entropy_with_logits(
            second.squeeze(1), labels.to(second.dtype))
    return torch.nn.functional.cross_entropy(second, labels)


def _ref_step(net, table_np, batch, unsup, labels):
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in net.named_parameters()}
    table = torch.from_numpy(table_np).double().requires_grad_()
    if unsup:
        emb = _ref_tower(P, table, batch.center)
        ctx = _ref_tower(P, table, batch.context).reshape(*labels.shape, -1)
        second = torch.bmm(emb.unsqueeze(1), ctx.permute(0, 2, 1))
    else:
        emb = _ref_tower(P, table, batch)
        second = emb @ P["dense.weight"].t() + P["dense.bias"]
    _loss(unsup, emb, second, labels.cpu()).backward()
    out = {"emb": emb.detach().numpy(), "second": second.detach().numpy(),
           "table": table.grad.numpy()}
    out.update({k: v.grad.numpy() for k, v in P.items()})
    return out


def _gpu_step(net, table, batch, unsup, labels):
    net.zero_grad()
    if table.grad is not None:
        table.grad = None
    with torch.enable_grad():
        args = batch.forward_args(table)
        if not unsup:
            args = (*args, None, None, None, None, None)
        emb, second = net(*args)
        _loss(unsup, emb, second, labels).backward()
    out = {"emb": emb.detach().cpu().numpy(), "second": second.detach().cpu().numpy()}
    if table.requires_grad:
        out["table"] = table.grad.cpu().numpy().copy()
    out.update({k: p.grad.cpu().numpy().copy() for k, p in net.named_parameters()})
    return out


def test_model_step_when_the_scatter_declines(dev, monkeypatch):
    """A None from sage_scatter_concat inside the layer's backward (a shape it declines, e.g.
    2^31 slots) drops that gradient to the SpMM over the Python-built CSR: same numbers."""
    from graphneuralnetwork_amd import graphsage
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    n, F, H = _graph()[0], 64, 128
    batch = _batch(False)
    rng = np.random.default_rng(32)
    t_np = rng.standard_normal((n, F)).astype(np.float32)
    net = GraphSAGE(2, F, H, agg_func="MEAN", Unsupervised=False, class_size=7).to(dev).train()
    labels = torch.from_numpy(rng.integers(0, 7, 40)).to(dev)
    runs = []
    for decline in (False, True):
        asked = []
        if decline:
            monkeypatch.setattr(graphsage, "sage_scatter_concat",
                                lambda *a, **k: asked.append(1))  # returns None
        t = torch.from_numpy(t_np).to(dev).requires_grad_()
        runs.append(_gpu_step(net, t, batch, False, labels))
        assert len(asked) == (2 if decline else 0)
    for name in runs[0]:
        close(runs[1][name], runs[0][name], what=f"{name}: scatter declined vs taken")
    assert np.abs(runs[0]["table"]).max() > 0


@pytest.mark.parametrize("unsup", [False, True], ids=["supervised", "unsupervised"])
@pytest.mark.parametrize("F,H", [(64, 128), (36, 24)])
def test_model_step(dev, monkeypatch, unsup, F, H):
    from graphneuralnetwork_amd import graphsage
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    n = _graph()[0]
    batch = _batch(unsup)
    rng = np.random.default_rng(31)
    t_np = rng.standard_normal((n, F)).astype(np.float32)
    t_np = torch.from_numpy(t_np).bfloat16().float().numpy()  # bf16-representable values
    torch.manual_seed(0)
    net = GraphSAGE(2, F, H, agg_func="MEAN", Unsupervised=unsup,
                    class_size=None if unsup else 7).to(dev).train()
    labels = batch.labels if unsup else torch.from_numpy(rng.integers(0, 7, 40)).to(dev)
    calls = []
    real = graphsage.sage_scatter_concat

    def counted(dbuf, tr, n_prev):
        r = real(dbuf, tr, n_prev)
        calls.append(r is not None)
        return r

    monkeypatch.setattr(graphsage, "sage_scatter_concat", counted)
    covered = (F, H) == (64, 128)
    towers = 2 if unsup else 1
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(graphsage, "SAGE_TRAIN_FUSED", fused)
        for kind in ("fp32_grad", "fp32", "bf16"):
            t = torch.from_numpy(t_np).to(dev)
            t = t.bfloat16() if kind == "bf16" else t.requires_grad_(kind == "fp32_grad")
            del calls[:]
            runs[fused, kind] = _gpu_step(net, t, batch, unsup, labels)
            # layer 1 always scatters (its table is layer 0's output); layer 0 only for a
            # table that asks for its gradient
            want = towers * (2 if kind == "fp32_grad" else 1) if fused and covered else 0
            assert calls == [True] * want, (fused, kind, calls)
    ref = _ref_step(net, t_np, batch, unsup, labels)
    names = ["emb", "second"] + [k for k, _ in net.named_parameters()]
    for kind in ("fp32_grad", "fp32", "bf16"):
        for name in names + (["table"] if kind == "fp32_grad" else []):
            on, off = runs[True, kind][name], runs[False, kind][name]
            close(on, off, what=f"{kind} {name}: switch on vs off")
            close(on, ref[name], what=f"{kind} {name}: switch on vs float64")
            if kind == "bf16":
                close(on, runs[True, "fp32"][name], what=f"{name}: bf16 table vs fp32 table")
    assert np.abs(ref["table"]).max() > 0
    for name, _ in net.named_parameters():
        assert np.abs(ref[name]).max() > 0, name
