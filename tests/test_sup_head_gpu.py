"""The supervised head on the device (csrc/sup_head.hip, ops.sup_head_count / sup_head_forward /
sup_head_backward, loss.supervised_loss / accuracy): the masked mean cross entropy of the
reference's loops, the count of correct predictions and the gradient with respect to the whole
logits, against torch's float64 cross entropy and its autograd on the CPU.

Values: the project's fp32 rule (``_close`` of test_unsup_sampler_gpu: rtol 1e-4, atol
2e-5 max|ref|). Counts, zeros, multiplicities, determinism and the switch-off path: exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
GIB = 1 << 30
UP = 3.0  # the upstream gradient of the loss: the scaling is exercised


@pytest.fixture(autouse=True)
def _every_size_on_the_device(monkeypatch):
    """The dispatcher's row thresholds (measured speed, not coverage) off: these tests are about
    the kernels at the smallest shapes at which they can go wrong."""
    from graphneuralnetwork_amd import loss as L
    monkeypatch.setattr(L, "SUPERVISED_HEAD_MIN_ROWS", 0)
    monkeypatch.setattr(L, "SUPERVISED_HEAD_MIN_ROWS_INDEXED", 0)


def _close(got, ref, what):  # test_unsup_sampler_gpu._close
    a, b = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: max|err| {err:.3e} max|ref| {scale:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=2e-5 * scale, err_msg=what)


def _sel(t, index):
    return t if index is None else t[index]


def _ref(z, labels, index, up=UP):
    """torch in float64 on the CPU: (loss, n_correct, d(up loss)/dz)."""
    zd = z.detach().double().cpu().requires_grad_()
    lab = labels.cpu()
    idx = None if index is None else index.cpu()
    loss = F.cross_entropy(_sel(zd, idx), _sel(lab, idx))
    (up * loss).backward()
    correct = (torch.argmax(_sel(z.detach().cpu(), idx), 1) == _sel(lab, idx)).sum()
    return loss.detach(), correct, zd.grad


def _fused(z, labels, index, up=UP, **kw):
    """loss.supervised_loss and its autograd: (loss, n_correct, d(up loss)/dz)."""
    from graphneuralnetwork_amd import loss as L
    zz = z.detach().requires_grad_()  # shares z's storage and strides
    loss, correct = L.supervised_loss(zz, labels, index, count_correct=True, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert correct.dim() == 0 and correct.dtype == torch.int64 and correct.is_cuda
    (dz,) = torch.autograd.grad(loss, zz, torch.tensor(up, device=z.device))
    assert dz.shape == z.shape and dz.dtype == torch.float32
    return loss.detach(), correct, dz


def _logits(dev, N, C, layout, gen):
    if layout == "contiguous":
        return torch.randn(N, C, device=dev, generator=gen) * 2
    wide = torch.randn(N, C + 3, device=dev, generator=gen) * 2
    z = wide[:, 1:1 + C]  # rows 4 bytes off a 16-byte boundary, pitch C + 3
    assert z.data_ptr() % 16 == 4 and (N == 1 or z.stride(0) == C + 3)
    return z


def _dup_index(N, gen, dev):
    """About N / 3 entries with duplicates and negative entries (N >= 1)."""
    n = max(2, N // 3)
    idx = torch.randint(-N, N, (n,), device=dev, generator=gen)
    idx[0] = idx[-1]
    return idx


@pytest.mark.parametrize("layout", ["contiguous", "pitched"])
@pytest.mark.parametrize("N", [1, 5, 257, 4099])
@pytest.mark.parametrize("C", [2, 3, 7, 8, 33, 64])
def test_parity(dev, C, N, layout):
    gen = torch.Generator(device=dev).manual_seed(100 * C + N)
    z = _logits(dev, N, C, layout, gen)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen)
    for index in (None, _dup_index(N, gen, dev)):
        loss, correct, dz = _fused(z, labels, index)
        rl, rc, rdz = _ref(z, labels, index)
        what = f"C={C} N={N} {layout} index={'none' if index is None else 'dup'}"
        _close(loss, rl, "loss " + what)
        assert int(correct) == int(rc), what
        _close(dz, rdz, "dz " + what)
        assert dz.is_contiguous()


@pytest.fixture(scope="module")
def case257(dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    N, C = 257, 7
    z = torch.randn(N, C, device=dev, generator=gen) * 2
    labels = torch.randint(0, C, (N,), device=dev, generator=gen)
    return N, C, z, labels, gen


def _selections(N, dev, gen):
    unique = torch.randperm(N, device=dev, generator=gen)[:60]
    dup = unique.clone()
    dup[1] = dup[2] = dup[0]      # one node three times
    dup[11] = dup[10]             # another twice
    neg = unique.clone()
    neg[::3] -= N                 # entries in [-N, 0) wrap
    mask = torch.rand(N, device=dev, generator=gen) < 0.3
    return {"none": None, "unique": unique, "dup": dup, "negative": neg, "mask": mask}


@pytest.mark.parametrize("kind", ["none", "unique", "dup", "negative", "mask"])
def test_selections(dev, case257, kind):
    from graphneuralnetwork_amd import ops
    N, C, z, labels, _ = case257
    index = _selections(N, dev, torch.Generator(device=dev).manual_seed(6))[kind]
    loss, correct, dz = _fused(z, labels, index)
    rl, rc, rdz = _ref(z, labels, index)
    _close(loss, rl, f"loss {kind}")
    assert int(correct) == int(rc)
    _close(dz, rdz, f"dz {kind}")
    if index is None:
        return
    # the multiplicity, exactly; rows that are not selected, exactly zero
    count, status = ops.sup_head_count(index, N)
    want = (index.to(torch.int32) if index.dtype == torch.bool
            else torch.bincount(index % N, minlength=N).to(torch.int32))
    assert count.dtype == torch.int32 and torch.equal(count, want) and int(status) == 0
    if kind == "dup":
        assert sorted(count[count > 1].tolist()) == [2, 3]
    assert torch.equal(dz[count == 0], torch.zeros_like(dz[count == 0]))
    assert bool((dz[count > 0] != 0).any(1).all())
    if kind == "mask":  # a mask is the same selection as its index
        l2, c2, dz2 = _fused(z, labels, torch.nonzero(index).view(-1))
        assert torch.equal(l2, loss) and torch.equal(c2, correct) and torch.equal(dz2, dz)


def test_empty_selection(dev, case257):
    N, C, z, labels, _ = case257
    for index in (torch.zeros(0, dtype=torch.int64, device=dev),
                  torch.zeros(N, dtype=torch.bool, device=dev)):
        loss, correct, dz = _fused(z, labels, index)
        zt = z.detach().clone().requires_grad_()
        lt = F.cross_entropy(zt[index], labels[index])
        (UP * lt).backward()
        assert torch.isnan(loss) and torch.isnan(lt) and int(correct) == 0
        assert torch.equal(dz, zt.grad) and not bool(dz.any())


def test_ignore_index(dev, case257):
    N, C, z, labels, _ = case257
    gen = torch.Generator(device=dev).manual_seed(8)
    index = _selections(N, dev, gen)["dup"]
    some = labels.clone()
    some[index[:20]] = -100  # the tripled node among them
    for idx in (index, None):
        loss, correct, dz = _fused(z, some, idx)
        rl, rc, rdz = _ref(z, some, idx)
        _close(loss, rl, "loss with ignored rows")
        assert int(correct) == int(rc)  # an ignored row is never correct
        _close(dz, rdz, "dz with ignored rows")
        assert not bool(dz[some == -100].any())
    none = labels.clone()
    none[index] = -100
    loss, correct, dz = _fused(z, none, index)
    zt = z.detach().clone().requires_grad_()
    lt = F.cross_entropy(zt[index], none[index])
    (UP * lt).backward()
    assert torch.isnan(loss) and torch.isnan(lt) and int(correct) == 0
    assert torch.equal(dz, zt.grad) and not bool(dz.any())


def test_argmax_rules(dev):
    """Ties go to the first maximum and a NaN counts as the maximum, as torch.argmax on the
    device; n_correct with labels on, before and after the winner."""
    from graphneuralnetwork_amd import loss as L
    inf, nan = float("inf"), float("nan")
    rows = torch.tensor([[1., 5., 5., 2., 5., 0., -1.],      # a tie: 1
                         [0., nan, 3., nan, 9., 1., 2.],     # NaN: 1
                         [0., 1., inf, 3., inf, 2., 1.],     # +inf twice: 2
                         [-inf, -inf, -inf, -inf, -inf, -inf, -inf],  # all equal: 0
                         [-inf, 2., 2., 1., 0., 0., 0.],
                         [3., 3., 3., 3., 3., 3., 3.]], device=dev)
    am = torch.argmax(rows, 1)
    assert am.tolist()[:4] == [1, 1, 2, 0]
    for shift in (0, 1, -1):
        labels = (am + shift) % 7
        for index in (None, torch.tensor([5, 0, 0, 1, 2, 3, 4, -5], device=dev)):
            _, correct = L.supervised_loss(rows, labels, index, count_correct=True)
            want = (torch.argmax(_sel(rows, index), 1) == _sel(labels, index)).sum()
            assert torch.equal(correct, want), (shift, index)
            assert L.accuracy(rows, labels, index) == float(want) / len(_sel(labels, index))


@pytest.mark.parametrize("pattern", ["plus_inf", "minus_inf_finite", "all_minus_inf", "nan"])
def test_non_finite_logits(dev, pattern):
    inf, nan = float("inf"), float("nan")
    special = {"plus_inf": [0.5, inf, -1.0], "minus_inf_finite": [-inf, 0.0, 0.0],
               "all_minus_inf": [-inf, -inf, -inf], "nan": [0.25, nan, 1.0]}[pattern]
    gen = torch.Generator(device=dev).manual_seed(9)
    z = torch.randn(6, 3, device=dev, generator=gen)
    z[2] = torch.tensor(special, device=dev)
    labels = torch.tensor([0, 2, 1, 1, 0, 2], device=dev)
    for index in (None, torch.tensor([2, 4, 2, 0], device=dev)):
        loss, correct, dz = _fused(z, labels, index)
        zt = z.detach().clone().requires_grad_()
        lt = F.cross_entropy(_sel(zt, index), _sel(labels, index))
        (UP * lt).backward()
        cls = lambda t: torch.stack((torch.isnan(t), torch.isinf(t)))  # noqa: E731
        assert torch.equal(cls(loss), cls(lt.detach())), pattern
        assert torch.equal(cls(dz), cls(zt.grad)), pattern
        assert torch.equal(correct, (torch.argmax(_sel(z, index), 1) == _sel(labels, index)).sum())
        assert bool(torch.isfinite(loss)) == (pattern == "minus_inf_finite")
        rl, _, rdz = _ref(z, labels, index)
        fin = torch.isfinite(dz).cpu()
        _close(dz.cpu()[fin], rdz[fin], f"finite dz, {pattern}")
        if pattern == "minus_inf_finite":
            _close(loss, rl, f"loss, {pattern}")


@pytest.mark.parametrize("bad", ["index_high", "index_low", "label_high", "label_negative"])
def test_status(dev, bad):
    """A bad index entry or label is never used as an address: NaN loss and an all-NaN gradient
    with check=False, an exception with check=True, and nothing written outside the logits'
    and the gradient's own elements."""
    from graphneuralnetwork_amd import loss as L
    from graphneuralnetwork_amd import ops
    N, C, G = 50, 7, 4096
    gen = torch.Generator(device=dev).manual_seed(10)
    zbuf = torch.full((G + N * C + G,), 7.0, device=dev)
    dbuf = torch.full((G + N * C + G,), 9.0, device=dev)
    z = zbuf[G:G + N * C].view(N, C)
    z.normal_(generator=gen)
    z0 = z.clone()
    labels = torch.randint(0, C, (N,), device=dev, generator=gen)
    index = torch.tensor([3, 7, 7, 49, -50, 20], device=dev)
    if bad == "index_high":
        index[2] = N
    elif bad == "index_low":
        index[4] = -N - 1
    elif bad == "label_high":
        labels[7] = C
    else:
        labels[20] = -1
    err = IndexError if bad.startswith("index") else ValueError
    bit = 1 if bad.startswith("index") else 2
    loss, correct, dz = _fused(z, labels, index)
    assert torch.isnan(loss) and bool(torch.isnan(dz).all())
    with pytest.raises(err):
        L.supervised_loss(z, labels, index, check=True)
    # the ops, with the gradient inside a guarded buffer
    count, status = ops.sup_head_count(index, N)
    lo, _, inv_valid, status = ops.sup_head_forward(z, labels, index, status=status)
    out = dbuf[G:G + N * C].view(N, C)
    got = ops.sup_head_backward(z, labels, count, torch.ones(1, device=dev), inv_valid, status,
                                out=out)
    assert got is out and int(status) == bit
    assert torch.isnan(lo) and bool(torch.isnan(out).all())
    assert torch.equal(z, z0)
    for buf, fill in ((zbuf, 7.0), (dbuf, 9.0)):
        assert bool((buf[:G] == fill).all()) and bool((buf[G + N * C:] == fill).all())
    if not bad.startswith("index"):  # no index: the bad label is met in the row pass
        loss, _, dz = _fused(z, labels, None)
        assert torch.isnan(loss) and bool(torch.isnan(dz).all())
        with pytest.raises(ValueError):
            L.supervised_loss(z, labels, None, check=True)


def test_deterministic(dev):
    gen = torch.Generator(device=dev).manual_seed(12)
    N, C = 4099, 7
    z = torch.randn(N, C, device=dev, generator=gen)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen)
    index = torch.randint(0, N, (3000,), device=dev, generator=gen)
    assert index.unique().numel() < index.numel()
    first, again = _fused(z, labels, index), _fused(z, labels, index)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["none", "dup", "mask"])
def test_no_host_read(dev, case257, kind):
    """The loss, the count, the upstream gradient and the status word stay on the device: forward
    and backward under torch's synchronisation check, then the same numbers as without it."""
    N, C, z, labels, _ = case257
    index = _selections(N, dev, torch.Generator(device=dev).manual_seed(6))[kind]
    want = _fused(z, labels, index)  # warm: the library is loaded, the pool holds the buffers
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        from graphneuralnetwork_amd import loss as L
        zz = z.detach().requires_grad_()
        loss, correct = L.supervised_loss(zz, labels, index, count_correct=True)
        (dz,) = torch.autograd.grad(loss * up, zz)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(loss.detach(), want[0]) and torch.equal(correct, want[1])
    assert torch.equal(dz, want[2])  # the factor reached the kernel as a device scalar


def _need(dev, nbytes, what):
    """No skip: a device without the memory fails the test with the figure."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < nbytes + (GIB >> 1):
        pytest.fail(f"{what} needs {nbytes / GIB:.2f} GiB of free device memory "
                    f"(+ 0.5 GiB of slack), found {free / GIB:.2f} GiB")


def test_wide_pitch(dev):
    """Logits [2^16 + 8, 7] at a pitch of 2^15 + 8 elements: the last rows start past 2^31
    elements (and 2^33 bytes) of the buffer, so a 32-bit r ldz reads another row."""
    N, C, pitch = (1 << 16) + 8, 7, (1 << 15) + 8
    assert (N - 8) * pitch > 1 << 31
    _need(dev, N * pitch * 4, "the pitched logits")
    gen = torch.Generator(device=dev).manual_seed(13)
    big = torch.empty(N * pitch, dtype=torch.float32, device=dev)
    try:
        z = big.view(N, pitch)[:, :C]
        z.copy_(torch.randn(N, C, device=dev, generator=gen) * 2)
        labels = torch.randint(0, C, (N,), device=dev, generator=gen)
        index = torch.cat([torch.arange(0, N, 3, device=dev),
                           torch.arange(N - 8, N, device=dev)])
        loss, correct, dz = _fused(z, labels, index)
        rl, rc, rdz = _ref(z, labels, index)
        _close(loss, rl, "loss, pitched past 2^31")
        assert int(correct) == int(rc)
        rows = torch.cat([torch.arange(8), torch.arange(N - 8, N)])
        _close(dz[rows.to(dev)], rdz[rows], "dz first / last 8 rows")
        _close(dz, rdz, "dz, pitched past 2^31")
    finally:
        del big
        torch.cuda.empty_cache()


def test_wide_rows(dev):
    """N C = 2^31 + 512 at C = 64: the logits' and the gradient's last rows lie past 2^31
    elements. The loss against float64 sums taken in pieces on the device, the first / last 8
    rows of the gradient against float64. Peak: z 8 GiB + dz 8 GiB + 0.5 GiB of pieces."""
    from graphneuralnetwork_amd import loss as L
    C = 64
    N = (1 << 25) + 8
    assert (N - 8) * C >= 1 << 31
    _need(dev, 2 * N * C * 4 + GIB, "the logits and their gradient")
    gen = torch.Generator(device=dev).manual_seed(14)
    z = torch.empty((N, C), dtype=torch.float32, device=dev)
    step = 1 << 20
    total = torch.zeros((), dtype=torch.float64, device=dev)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen)
    want_correct = 0
    for r0 in range(0, N, step):
        zc = z[r0:r0 + step]
        zc.normal_(0.0, 2.0, generator=gen)
        total += F.cross_entropy(zc.double(), labels[r0:r0 + step], reduction="sum")
        want_correct += int((torch.argmax(zc, 1) == labels[r0:r0 + step]).sum())
    z.requires_grad_()
    loss, correct = L.supervised_loss(z, labels, count_correct=True)
    _close(loss, total / N, "loss, N C past 2^31")
    assert int(correct) == want_correct
    (dz,) = torch.autograd.grad(loss, z, torch.tensor(UP, device=dev))
    rows = torch.cat([torch.arange(8), torch.arange(N - 8, N)]).to(dev)
    zd = z.detach()[rows].double()
    ref = (torch.softmax(zd, 1) - F.one_hot(labels[rows], C)) * (UP / N)
    _close(dz[rows], ref, "dz first / last 8 rows, N C past 2^31")
    # no row in between was skipped or written twice: every row of p - onehot sums to zero
    worst = 0.0
    for r0 in range(0, N, step):
        piece = dz[r0:r0 + step]
        worst = max(worst, float(piece.double().sum(1).abs().max()))
        assert bool((piece.abs().amax(1) > 0).all())
    assert worst < 1e-6 * UP / N * C
    del z, dz
    torch.cuda.empty_cache()


def test_ops_wrappers(dev):
    from graphneuralnetwork_amd import ops
    z = torch.randn(20, 7, device=dev)
    y = torch.randint(0, 7, (20,), device=dev)
    idx = torch.tensor([1, 2, 2], device=dev)
    r = ops.sup_head_forward(z, y, idx)
    assert r is not None and len(r) == 4
    only = ops.sup_head_forward(z, y, idx, want_correct=False)
    assert only[1] is None and torch.equal(only[0], r[0])
    with pytest.raises(ValueError):
        ops.sup_head_forward(z[0], y)                          # logits not [N, C]
    with pytest.raises(ValueError):
        ops.sup_head_forward(z, y[:5])                         # labels of another length
    with pytest.raises(TypeError):
        ops.sup_head_forward(z, y, idx.to(torch.int32))
    with pytest.raises(ValueError):
        ops.sup_head_forward(z, y, idx.view(1, 3))
    with pytest.raises(TypeError):
        ops.sup_head_count(idx.float(), 20)
    with pytest.raises(ValueError):
        ops.sup_head_count(torch.zeros(19, dtype=torch.bool, device=dev), 20)
    count, status = ops.sup_head_count(idx, 20)
    with pytest.raises(ValueError):
        ops.sup_head_forward(z, y, idx, count)                 # the selection given twice
    with pytest.raises(ValueError):
        ops.sup_head_backward(z, y, count[:5], torch.ones(1, device=dev), r[2], r[3])
    with pytest.raises(TypeError):
        ops.sup_head_backward(z, y, count, torch.ones(1, device=dev).double(), r[2], r[3])
    wide = torch.randn(20, 130, device=dev)
    assert ops.sup_head_forward(wide[:, :1], y) is None        # C = 1
    assert ops.sup_head_forward(wide[:, :65], y) is None       # C = 65
    assert ops.sup_head_forward(wide[:, :14:2], y) is None     # stride 2 along C
    assert ops.sup_head_forward(z, y.float()) is None          # float labels
    assert ops.sup_head_forward(z, torch.rand(20, 7, device=dev)) is None  # probabilities
    assert ops.sup_head_forward(z.double(), y) is None
    assert ops.sup_head_backward(wide[:, :65], y, None, torch.ones(1, device=dev), r[2],
                                 r[3]) is None
    assert ops.sup_head_forward(wide[:, :64], y) is not None   # C = 64, pitch 130


@pytest.mark.parametrize("kind", ["none", "dup", "mask"])
def test_switch_off_is_torchs(dev, case257, kind, monkeypatch):
    from graphneuralnetwork_amd import loss as L
    N, C, z, labels, _ = case257
    index = _selections(N, dev, torch.Generator(device=dev).manual_seed(6))[kind]
    monkeypatch.setattr(L, "SUPERVISED_HEAD_FUSED", False)
    loss, correct, dz = _fused(z, labels, index)
    zt = z.detach().clone().requires_grad_()
    lt = F.cross_entropy(_sel(zt, index), _sel(labels, index))
    (dzt,) = torch.autograd.grad(lt, zt, torch.tensor(UP, device=dev))
    assert torch.equal(loss, lt.detach()) and torch.equal(dz, dzt)
    assert torch.equal(correct, (torch.argmax(_sel(z, index), 1) == _sel(labels, index)).sum())
    monkeypatch.setattr(L, "SUPERVISED_HEAD_FUSED", True)
    on = _fused(z, labels, index)
    _close(on[0], loss, "on vs off loss")
    _close(on[2], dz, "on vs off dz")


@pytest.mark.parametrize("kind", ["none", "dup"])
def test_below_the_row_threshold_is_torchs(dev, case257, kind, monkeypatch):
    """Fewer rows than the measured thresholds: torch's expression, bit for bit, and no call of
    the device head."""
    from graphneuralnetwork_amd import loss as L
    monkeypatch.undo()  # the module's thresholds as they ship
    assert 257 < L.SUPERVISED_HEAD_MIN_ROWS <= L.SUPERVISED_HEAD_MIN_ROWS_INDEXED
    N, C, z, labels, _ = case257
    index = _selections(N, dev, torch.Generator(device=dev).manual_seed(6))[kind]

    def never(*a, **k):
        raise AssertionError("the device head ran below its row threshold")

    monkeypatch.setattr(L, "sup_head_forward", never)
    loss, correct, dz = _fused(z, labels, index)
    zt = z.detach().clone().requires_grad_()
    lt = F.cross_entropy(_sel(zt, index), _sel(labels, index))
    (dzt,) = torch.autograd.grad(lt, zt, torch.tensor(UP, device=dev))
    assert torch.equal(loss, lt.detach()) and torch.equal(dz, dzt)
    assert torch.equal(correct, (torch.argmax(_sel(z, index), 1) == _sel(labels, index)).sum())
    assert L.accuracy(z, labels, index) == _ref_accuracy(_sel(z, index), _sel(labels, index))


def _ref_accuracy(y_hat, y):  # GCN/train_eval.py:9-17
    if len(y_hat.shape) > 1 and y_hat.shape[1] > 1:
        y_hat = torch.argmax(y_hat, axis=1)
    cmp = y_hat.to(dtype=y.dtype) == y
    cmp = cmp.to(dtype=y.dtype)
    return float(cmp.sum()) / len(cmp)


def _small_graph(n=300):
    rng = np.random.default_rng(15)
    s, d = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    return n, np.concatenate([s, d, np.arange(n)]), np.concatenate([d, s, np.arange(n)])


def _model_steps(net, forward, labels, index, dev):
    """One training step with supervised_loss and one with torch's loss on the same logits'
    graph: (loss, grads) each."""
    from graphneuralnetwork_amd import loss as L
    out = {}
    for fused in (True, False):
        net.zero_grad(set_to_none=True)
        logits = forward()
        if fused:
            loss = L.supervised_loss(logits, labels, index)
        else:
            loss = F.cross_entropy(_sel(logits, index), _sel(labels, index))
        loss.backward()
        out[fused] = (loss.detach(), {k: p.grad.clone() for k, p in net.named_parameters()
                                      if p.grad is not None},
                      logits.detach())
    _close(out[True][0], out[False][0], "model loss")
    assert out[False][1] and any(float(g.abs().max()) > 0 for g in out[False][1].values())
    for k, g in out[False][1].items():
        _close(out[True][1][k], g, f"model grad {k}")
    logits = out[True][2]
    assert L.accuracy(logits, labels, index) == _ref_accuracy(_sel(logits, index),
                                                              _sel(labels, index))


def test_gcn_model_step(dev):
    from graphneuralnetwork_amd.gcn import GCN_Model
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    n, s, d = _small_graph()
    g = gcn_adjacency(torch.from_numpy(s), torch.from_numpy(d), n, device=dev)
    torch.manual_seed(16)
    net = GCN_Model(16, 16, 7, 2, 0.0).to(dev).train()
    x = torch.randn(n, 16, device=dev)
    labels = torch.randint(0, 7, (n,), device=dev)
    _model_steps(net, lambda: net(x, g), labels, torch.arange(0, n, 3, device=dev), dev)


def test_gat_model_step(dev):
    from graphneuralnetwork_amd.gat import GAT
    from graphneuralnetwork_amd.graph import CsrGraph
    n, s, d = _small_graph()
    key = np.unique(s * n + d)
    r, c = key // n, key % n
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    g = CsrGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev),
                 torch.ones(c.size, device=dev), n, n, symmetric=True)
    torch.manual_seed(17)
    net = GAT(16, 8, 7, 0.0, 0.2, 2).to(dev).train()
    x = 0.5 * torch.randn(n, 16, device=dev)
    labels = torch.randint(0, 7, (n,), device=dev)
    _model_steps(net, lambda: net(x, g), labels, torch.arange(0, n, 3, device=dev), dev)


def test_graphsage_model_step(dev):
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    from graphneuralnetwork_amd.sampler import sample_batch, symmetric_adjacency
    n, s, d = _small_graph()
    adj = symmetric_adjacency(s[:1500], d[:1500], n, device=dev)
    deg = adj.rowptr[1:] - adj.rowptr[:-1]
    seeds = torch.nonzero(deg > 0).view(-1)[:64]
    batch = sample_batch(adj, seeds, (5, 3), seed=3)
    torch.manual_seed(18)
    net = GraphSAGE(2, 16, 16, agg_func="MEAN", Unsupervised=False, class_size=7).to(dev).train()
    table = torch.randn(n, 16, device=dev)
    labels = torch.randint(0, 7, (seeds.numel(),), device=dev)
    args = (*batch.forward_args(table), None, None, None, None, None)
    _model_steps(net, lambda: net(*args)[1], labels, None, dev)


def test_no_grad_allocates_no_logits_sized_tensor(dev):
    """The val_loss of the loops: under no_grad neither an [N, C] nor an [n, C] tensor."""
    from graphneuralnetwork_amd import loss as L
    N, C = 4099, 7
    z = torch.randn(N, C, device=dev, requires_grad=True)
    labels = torch.randint(0, C, (N,), device=dev)
    index = torch.arange(0, N, 2, device=dev)
    for idx in (None, index):
        with torch.no_grad():
            L.supervised_loss(z, labels, idx, count_correct=True)  # warm: the library, the pool
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        with torch.no_grad():
            loss, correct = L.supervised_loss(z, labels, idx, count_correct=True)
        torch.cuda.synchronize(dev)
        after = torch.cuda.memory_allocated(dev)
        peak = torch.cuda.max_memory_allocated(dev)
        n = N if idx is None else idx.numel()
        assert not loss.requires_grad and loss.grad_fn is None
        assert after - before <= 2 * 512, (before, after)       # the two 0-dim results
        assert peak - before < n * C * 4, (before, peak)        # no [n, C] temporary either
