"""The operand contract of the GraphSAGE adjoint's Python wrappers, the same for every form: the
four scatters (ops.sage_scatter_concat / _concat_maxpool / sage_scatter_agg / _agg_maxpool) and
the two transposed-map builders (ops.sage_maps_transpose / _nbr).

Pinned per form: the exception type of each malformed operand, None for each operand the kernels
decline, ``out=`` returned as given, zeros for M = 0, and the result against a float64 numpy
scatter (rtol 1e-4, atol 1e-5 max|ref|: test_sage_train_gpu.close_sum) or, for the builders,
numpy's stable argsort bit for bit. Every malformed operand is rejected before a launch.
"""
import numpy as np
import pytest
import torch
from test_sage_train_gpu import close_sum

pytestmark = pytest.mark.gpu

N_PREV, M, K, F = 7, 5, 3, 8
SCATTERS = {  # name: (the concat layout with a centre half, the MAXPOOL select)
    "sage_scatter_concat": (True, False),
    "sage_scatter_concat_maxpool": (True, True),
    "sage_scatter_agg": (False, False),
    "sage_scatter_agg_maxpool": (False, True),
}
BUILDERS = ("sage_maps_transpose", "sage_maps_transpose_nbr")
scatters = pytest.mark.parametrize("name", list(SCATTERS))
builders = pytest.mark.parametrize("name", BUILDERS)


def _build(dev, name, cidx, idx, n_prev=N_PREV, **kw):
    """Either builder on numpy (or tensor) maps; the centre map goes to the concat form only."""
    from graphneuralnetwork_amd import ops
    t = [x if torch.is_tensor(x) else torch.from_numpy(x).to(dev) for x in (cidx, idx)]
    if name == "sage_maps_transpose":
        return ops.sage_maps_transpose(t[0], t[1], n_prev, **kw)
    return ops.sage_maps_transpose_nbr(t[1], n_prev, **kw)


class Case:
    """Valid operands of one scatter form at [M, k] over n_prev rows and width F."""

    def __init__(self, dev, name, M=M, k=K, F=F, n_prev=N_PREV):
        self.name, (self.centre, self.mask) = name, SCATTERS[name]
        rng = np.random.default_rng(1000 * M + 10 * k + F)
        self.cidx = rng.integers(0, n_prev, M).astype(np.int64)
        self.idx = rng.integers(0, n_prev, (M, k)).astype(np.int64)
        self.width = 2 * F if self.centre else F
        self.d = rng.standard_normal((M, self.width)).astype(np.float32)
        self.a = rng.integers(0, max(k, 1), (M, F)).astype(np.uint8)
        self.n_prev, self.F, self.k, self.M = n_prev, F, k, M
        self.dbuf = torch.from_numpy(self.d).to(dev)
        self.arg = torch.from_numpy(self.a).to(dev)
        self.tr = _build(dev, BUILDERS[0] if self.centre else BUILDERS[1], self.cidx, self.idx,
                         n_prev)

    def run(self, dbuf=None, arg=None, tr=None, n_prev=None, out=None):
        from graphneuralnetwork_amd import ops
        dbuf = self.dbuf if dbuf is None else dbuf
        tr = self.tr if tr is None else tr
        n_prev = self.n_prev if n_prev is None else n_prev
        if self.mask:
            return getattr(ops, self.name)(dbuf, self.arg if arg is None else arg, tr, n_prev,
                                           out=out)
        return getattr(ops, self.name)(dbuf, tr, n_prev, out=out)

    def ref(self):
        """The float64 scatter: centre rows whole, a neighbour entry scaled by 1 / k (MEAN) or
        the elements it won (MAXPOOL)."""
        d, Fw = self.d.astype(np.float64), self.F
        out = np.zeros((self.n_prev, Fw))
        if self.centre:
            np.add.at(out, self.cidx, d[:, :Fw])
            d = d[:, Fw:]
        if self.mask:
            rows = np.take_along_axis(self.idx, self.a.astype(np.int64), axis=1)  # [M, F]
            np.add.at(out, (rows, np.broadcast_to(np.arange(Fw), rows.shape)), d)
        else:
            np.add.at(out, self.idx.reshape(-1), np.repeat(d / self.k, self.k, axis=0))
        return out


# ------------------------------------------------------------------ (a) malformed operands
@scatters
def test_scatter_malformed_operands_raise_the_same_types(dev, name):
    from graphneuralnetwork_amd import ops
    c = Case(dev, name)
    other = Case(dev, "sage_scatter_agg" if c.centre else "sage_scatter_concat")
    with pytest.raises(TypeError):
        c.run(dbuf=c.dbuf.double())
    if c.mask:
        with pytest.raises(TypeError):
            c.run(arg=c.arg.long())
    with pytest.raises(ValueError):  # maps of the other kind
        c.run(tr=other.tr)
    with pytest.raises(ValueError):  # the same arrays, the other kind declared
        c.run(tr=ops.SageMapsT(c.tr.ptr, c.tr.slot, M, K, not c.centre))
    with pytest.raises(ValueError):
        c.run(n_prev=N_PREV + 1)
    with pytest.raises(ValueError):  # a non-contiguous out=
        c.run(out=torch.zeros((N_PREV, 2 * F), device=dev)[:, :F])
    flat = torch.zeros(N_PREV * F + 1, device=dev)
    with pytest.raises(ValueError):  # a contiguous out= 4 bytes off a 16-B boundary
        c.run(out=flat[1:].view(N_PREV, F))
    with pytest.raises(ValueError):  # a slot array of the wrong length
        c.run(tr=ops.SageMapsT(c.tr.ptr, c.tr.slot[:-1], M, K, c.centre))


@builders
def test_builder_malformed_operands_raise_the_same_types(dev, name):
    cidx = torch.zeros(M, dtype=torch.int64, device=dev)
    idx = torch.zeros((M, K), dtype=torch.int64, device=dev)
    with pytest.raises(TypeError):
        _build(dev, name, cidx, idx.int())
    with pytest.raises(ValueError):
        _build(dev, name, cidx, idx.reshape(-1))
    with pytest.raises(ValueError):
        _build(dev, name, cidx, idx, n_prev=-1)
    bad = idx.clone()
    bad[2, 1] = N_PREV
    with pytest.raises(IndexError):
        _build(dev, name, cidx, bad)
    if name == "sage_maps_transpose":
        with pytest.raises(TypeError):
            _build(dev, name, cidx.int(), idx)
        with pytest.raises(ValueError):
            _build(dev, name, cidx[:-1], idx)


# ------------------------------------------------------------------ (b) declined operands
@scatters
def test_scatter_declined_operands_return_none(dev, name):
    for width in (36, 512):
        c = Case(dev, name, F=width)
        assert c.run() is None, f"F = {width}"
    c = Case(dev, name)
    flat = torch.zeros(M * c.width + 1, device=dev)
    shifted = flat[1:].view(M, c.width)  # the rows start one element off a 16-B boundary
    assert shifted.data_ptr() % 16 == 4
    assert c.run(dbuf=shifted) is None
    assert Case(dev, name, k=0).run() is None
    assert c.run() is not None
    if c.mask:  # the uint8 winner holds a column below 255
        wide = Case(dev, name, M=1, k=256)
        assert (wide.tr.M, wide.tr.k) == (1, 256)
        assert wide.run() is None
        assert Case(dev, name, M=1, k=255).run() is not None


@builders
def test_builder_declines_a_table_past_int32(dev, name):
    cidx = torch.zeros(M, dtype=torch.int64, device=dev)
    idx = torch.zeros((M, K), dtype=torch.int64, device=dev)
    assert _build(dev, name, cidx, idx, n_prev=2 ** 31 - 1, check=False) is None


# ------------------------------------------------------------------ (c), (d), (e)
@scatters
def test_scatter_out_is_returned_and_matches_float64(dev, name):
    c = Case(dev, name)
    want = c.ref()
    got = c.run()
    assert got.shape == (N_PREV, F) and got.dtype == torch.float32
    close_sum(got.cpu().numpy(), want, name)
    out = torch.full((N_PREV, F), float("nan"), device=dev)
    assert c.run(out=out) is out
    assert torch.equal(out, got)  # every row stored, the sums in the same order


@scatters
def test_scatter_of_one_row_with_any_row_stride(dev, name):
    """M = 1: the row strides of dbuf and arg are never used, whatever they are."""
    c = Case(dev, name, M=1)
    d2 = torch.zeros((2, c.width + 1), device=dev)
    d2[:1, :c.width] = c.dbuf
    a2 = torch.zeros((2, F + 1), dtype=torch.uint8, device=dev)
    a2[:1, :F] = c.arg
    dbuf, arg = d2[:1, :c.width], a2[:1, :F]
    assert dbuf.stride(0) == c.width + 1 and arg.stride(0) % 4 == 1
    got = c.run(dbuf=dbuf, arg=arg)
    assert got is not None
    close_sum(got.cpu().numpy(), c.ref(), name + " M=1")


@scatters
def test_scatter_of_no_rows_is_zeros(dev, name):
    c = Case(dev, name, M=0)
    assert (c.tr.M, c.tr.k, c.tr.slot.numel()) == (0, K, 0)
    z = c.run()
    assert z.shape == (N_PREV, F) and z.dtype == torch.float32 and int((z != 0).sum()) == 0
    out = torch.full((N_PREV, F), float("nan"), device=dev)
    assert c.run(out=out) is out and int((out != 0).sum()) == 0


def _np_transpose(name, cidx, idx, n_prev):
    tgt = idx.reshape(-1)
    if name == "sage_maps_transpose":
        tgt = np.concatenate([cidx.reshape(-1), tgt])
    ptr = np.zeros(n_prev + 1, np.int64)
    np.cumsum(np.bincount(tgt, minlength=n_prev), out=ptr[1:])
    return ptr, np.argsort(tgt, kind="stable").astype(np.int32)


@builders
@pytest.mark.parametrize("rows,k", [(M, K), (1, K), (0, K), (M, 0)])
def test_builder_matches_numpy(dev, name, rows, k):
    rng = np.random.default_rng(10 * rows + k)
    centre = name == "sage_maps_transpose"
    cidx = rng.integers(0, N_PREV, rows).astype(np.int64)
    wide = torch.from_numpy(rng.integers(0, N_PREV, (rows + 1, 2 * k + 1))).to(dev)
    view = wide[:rows, :2 * k:2]  # [rows, k], neither stride a contiguous one
    assert tuple(view.shape) == (rows, k) and (k == 0 or view.stride() == (2 * k + 1, 2))
    tr = _build(dev, name, cidx, view)
    ptr, slot = _np_transpose(name, cidx, view.cpu().numpy(), N_PREV)
    assert (tr.M, tr.k, tr.centre) == (rows, k, centre)
    assert tr.ptr.dtype == torch.int64 and tr.slot.dtype == torch.int32
    assert np.array_equal(tr.ptr.cpu().numpy(), ptr)
    assert np.array_equal(tr.slot.cpu().numpy(), slot)
