"""The feature transform's bf16 store epilogue (gnn_gcn_transform_bf16out / _rows_bf16out).

The MFMA sequence is the fp32 entry's, so the stored bf16 is the round-to-nearest-even of
exactly the fp32 value that entry stores: compared bit for bit (int16 views) with torch's
float32 -> bfloat16 conversion of the fp32 result. Inputs are scaled so that no result is
subnormal (subnormal rounding is not pinned).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64), (64, 128), (128, 128), (128, 64), (256, 256)]


@pytest.fixture(params=["split-bf16", "fp32-mfma"])
def precision(request, dev):
    from graphneuralnetwork_amd import ops
    prev = ops.set_transform_precision(request.param)
    yield request.param
    ops.set_transform_precision(prev)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(n, k, fout, dev):
    # |x w^T| ~ 1: far from the subnormal range; exact zeros are not subnormal either
    return torch.randn(n, k, device=dev), torch.randn(fout, k, device=dev) / k ** 0.5


@pytest.mark.parametrize("n", [1, 15, 17, 1000])
@pytest.mark.parametrize("k,fout", SHAPES)
def test_bf16_store_is_the_rounded_fp32_result(dev, precision, k, fout, n):
    from graphneuralnetwork_amd.ops import gcn_transform
    x, w = _inputs(n, k, fout, dev)
    if n > 2:  # a NaN row, and rows whose results are +inf / -inf in every column
        x[0, k // 2] = float("nan")
        x[1] = 0
        x[1, 0] = float("inf")
        w[:, 0] = w[:, 0].abs() + 0.5
        x[2] = -x[1]
    ref = gcn_transform(x, w)
    y = gcn_transform(x, w, out_dtype=torch.bfloat16)
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    want = ref.to(torch.bfloat16)
    ok = ~torch.isnan(want)
    assert torch.equal(_bits(y)[ok], _bits(want)[ok])
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    if n > 2:
        assert bool(torch.isnan(y[0]).all())
        if precision == "fp32-mfma" or k < 128:  # the split-bf16 products turn an inf into NaN
            assert bool((y[1] == float("inf")).all()) and bool((y[2] == float("-inf")).all())
    # a bf16 `out` decides the dtype
    out = torch.empty(n, fout, device=dev, dtype=torch.bfloat16)
    assert gcn_transform(x, w, out=out) is out
    assert torch.equal(_bits(out), _bits(y))


@pytest.mark.parametrize("k,fout", SHAPES)
def test_scattered_rows(dev, precision, k, fout):
    from graphneuralnetwork_amd.ops import gcn_transform
    n = 1000
    x, w = _inputs(n, k, fout, dev)
    ref = gcn_transform(x, w, out_dtype=torch.bfloat16)
    perm = torch.randperm(n, device=dev)
    y = gcn_transform(x, w, out_rows=perm, out_dtype=torch.bfloat16)
    want = torch.empty_like(ref)
    want[perm] = ref
    assert torch.equal(_bits(y), _bits(want))
    big = torch.full((2 * n + 3, fout), 7.0, device=dev, dtype=torch.bfloat16)
    ids = torch.randperm(2 * n + 3, device=dev)[:n]
    gcn_transform(x, w, out=big, out_rows=ids)
    assert torch.equal(_bits(big[ids]), _bits(ref))
    rest = torch.ones(2 * n + 3, dtype=torch.bool, device=dev)
    rest[ids] = False
    assert bool((big[rest] == 7.0).all())  # rows not named keep the sentinel


def test_bad_row_id_and_unsupported_forms(dev):
    from graphneuralnetwork_amd.ops import gcn_transform
    x = torch.randn(3, 64, device=dev)
    w = torch.randn(128, 64, device=dev)
    bad = torch.tensor([0, 3, 1], device=dev)
    with pytest.raises(IndexError):
        gcn_transform(x, w, out_rows=bad, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        gcn_transform(x, w, relu=True, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        gcn_transform(x, w, out_dtype=torch.float16)
    assert gcn_transform(x, torch.randn(7, 64, device=dev), out_dtype=torch.bfloat16) is None
