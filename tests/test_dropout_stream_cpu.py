"""Independence of the hashed dropout streams (no GPU): the element mask of (seed, row, column)
(csrc/common.hpp dropout_hash, through the oracle's C restatement) and the attention mask of
(seed, CSR edge, head) (csrc/gat.hip hash3, restated in numpy below). The masked training-step
tests take these masks as given; this pins that they behave as independent Bernoulli(1 - p)
draws: keep rate, correlation between neighbours (adjacent rows / columns, the diagonal, lags
2..1024), seed against seed + 1, and chi-square of the per-row and per-column keep counts, each
as a z-score with |z| < 5 (about 500 statistics: a true random stream exceeds 5 with
probability 3e-4 over all of them; the present hashes give at most |z| = 3.76 here, and gave
at most 2.44 in the numpy restatement run when the bound was set)."""
import numpy as np
import pytest

from oracle import c_oracle

SEEDS = [0, 77, 0x1234_5678_9ABC_DEF, 2 ** 61 + 5]  # two above 2^32
PS = [0.1, 0.5, 0.6]
LAGS = [2 ** i for i in range(1, 11)]  # 2 .. 1024
Z_MAX = 5.0


def _q(p):
    """The kept fraction the kernels realise: u = (hash >> 8) / 2^24 >= float32(p)."""
    return 1.0 - np.ceil(float(np.float32(p)) * 16777216.0) / 16777216.0


def _corr_z(a, b, q):
    """z-score of the co-occurrence of two 0/1 arrays of independent Bernoulli(q) draws."""
    n = a.size
    both = np.count_nonzero(a & b)
    return (both - n * q * q) / np.sqrt(n * q * q * (1.0 - q * q))


def _stream_zs(keep, other, q):
    """{name: z} for a [R, C] boolean keep block and the block of the next seed."""
    R, C = keep.shape
    zs = {"rate": (np.count_nonzero(keep) - keep.size * q) / np.sqrt(keep.size * q * (1 - q)),
          "rows+1": _corr_z(keep[1:], keep[:-1], q),
          "cols+1": _corr_z(keep[:, 1:], keep[:, :-1], q),
          "diag": _corr_z(keep[1:, 1:], keep[:-1, :-1], q),
          "seed+1": _corr_z(keep, other, q)}
    for lag in LAGS:
        if lag < R:
            zs[f"rows+{lag}"] = _corr_z(keep[lag:], keep[:-lag], q)
        if lag < C:
            zs[f"cols+{lag}"] = _corr_z(keep[:, lag:], keep[:, :-lag], q)
    for name, cnt, trials in (("chi2 rows", keep.sum(1), C), ("chi2 cols", keep.sum(0), R)):
        chi2 = float((((cnt - trials * q) ** 2) / (trials * q * (1 - q))).sum())
        zs[name] = (chi2 - cnt.size) / np.sqrt(2.0 * cnt.size)
    return zs


def _check(zs, tag):
    worst = max(zs, key=lambda k: abs(zs[k]))
    print(f"{tag}: {len(zs)} statistics, worst {worst} z = {zs[worst]:+.2f}")
    bad = {k: round(float(v), 2) for k, v in zs.items() if not abs(v) < Z_MAX}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", PS)
def test_element_dropout_stream_is_independent(p, seed):
    rows, cols = np.arange(65536)[:, None], np.arange(128)[None, :]
    keep = c_oracle.dropout_keep(seed, rows, cols, p)
    other = c_oracle.dropout_keep(seed + 1, rows, cols, p)
    _check(_stream_zs(keep, other, _q(p)), f"element p={p} seed={seed:#x}")


def _hash3(seed: int, edge: np.ndarray, head: np.ndarray) -> np.ndarray:
    """csrc/gat.hip hash3 in numpy uint32 arithmetic."""
    M = np.uint64(0xFFFFFFFF)
    e = edge.astype(np.uint64)
    h = np.uint64(seed & 0xFFFFFFFF) ^ ((np.uint64(seed >> 32) * np.uint64(0x27d4eb2f)) & M)
    h = h ^ ((e & M) * np.uint64(0x9e3779b9) & M)
    h = h ^ (((e >> np.uint64(32)) * np.uint64(0x85ebca6b)) & M)
    h = h ^ ((head.astype(np.uint64) * np.uint64(0xc2b2ae35)) & M)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & M
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & M
    h = h ^ (h >> np.uint64(16))
    return h


def _edge_keep(seed, n_edges, heads, p):
    h = _hash3(seed, np.arange(n_edges)[:, None], np.arange(heads)[None, :])
    return (h >> np.uint64(8)).astype(np.float64) / 16777216.0 >= float(np.float32(p))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", PS)
def test_attention_dropout_stream_is_independent(p, seed):
    """(edge, head) over 2^20 edges x 8 heads; rows are edges, columns heads."""
    keep = _edge_keep(seed, 1 << 20, 8, p)
    other = _edge_keep(seed + 1, 1 << 20, 8, p)
    _check(_stream_zs(keep, other, _q(p)), f"attention p={p} seed={seed:#x}")
