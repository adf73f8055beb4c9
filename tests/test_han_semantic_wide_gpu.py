"""64-bit addressing of the semantic-attention kernels (csrc/han_semantic.hip) on the smallest
z past 2^31 elements: M = 2, D = 64, N = 2^24 + 64 (8 GiB + 32 KiB), in the manner of
tests/test_wide_addressing_gpu.py.

z [N, 2, 64] and g [N, 64] are zero-filled; only 13 probe nodes carry data (random, so every
probe row differs): nodes 0, 1, N - 2, N - 1 and t - 1, t, t + 1 for t = 2^22, 2^23, 2^24 --
the nodes whose z rows lie around byte offset 2^31 (t = 2^22), byte offset 2^32 (2^23) and
element 2^31 (2^24) of z and dz, and around byte offsets 2^31 (2^23) and 2^32 (2^24) of g and
out. A wrapped offset reads zeros or another probe and stores into a row nobody asked for.

The float64 restatement uses the known zeros: a zero row scores s0 = w2 . tanh(b1), so
w[m] = (sum over the probes + (N - 13) s0) / N; out is zero off the probes; off the probes
dz[n, m] = q0[m] W1 with q0[m] = c[m] w2 (1 - tanh(b1)^2), one constant row per metapath (of
size 1 / N, so it is compared at its own scale); dW1 has terms from the probe rows alone.
dz is pre-filled with NaN and the rows that changed are counted.
Peak device memory: z 8 + dz 8 + g 4 + out 4 GiB + 2 GiB of masks. No skip: too little free
memory fails with the figure."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GIB = 1 << 30
N, M, D, S = (1 << 24) + 64, 2, 64, 128
PROBES = np.array(sorted({0, 1, N - 2, N - 1} | {t + k for t in (1 << 22, 1 << 23, 1 << 24)
                                                 for k in (-1, 0, 1)}), np.int64)


def close(a, b, rtol=1e-4):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-5 * float(np.abs(b).max()))


def test_probe_rows_pass_every_threshold():
    rows = (PROBES[:, None] * M + np.arange(M)).ravel()          # of the [N M, D] view
    for thr_bytes in (1 << 31, 1 << 32, 4 << 31):                 # 2^31 elements = 2^33 bytes
        r = thr_bytes // (4 * D)
        assert {r - 1, r, r + 1} <= set(rows.tolist()) and r + 1 < N * M
    for thr_bytes in (1 << 31, 1 << 32):                          # g and out: [N, D]
        n = thr_bytes // (4 * D)
        assert {n - 1, n, n + 1} <= set(PROBES.tolist()) and n + 1 < N
    assert N * M * D > 1 << 31


def test_forward_and_backward_past_2_31_elements(dev):
    from graphneuralnetwork_amd import ops
    free, _ = torch.cuda.mem_get_info(dev)
    need = 27 * GIB
    if free < need:
        pytest.fail(f"needs {need / GIB:.0f} GiB of free device memory, found {free / GIB:.2f}")
    rng = np.random.default_rng(5)
    P = len(PROBES)
    zp = rng.standard_normal((P, M, D)).astype(np.float32)
    zp[:, 1] += 0.5
    gp = rng.standard_normal((P, D)).astype(np.float32)
    w1 = (rng.standard_normal((S, D)) / 8).astype(np.float32)
    b1 = (0.3 * rng.standard_normal(S)).astype(np.float32)
    w2 = (rng.standard_normal(S) / 4).astype(np.float32)
    idx = torch.from_numpy(PROBES).to(dev)
    z = torch.zeros((N, M, D), device=dev)
    g = torch.zeros((N, D), device=dev)
    z[idx] = torch.from_numpy(zp).to(dev)
    g[idx] = torch.from_numpy(gp).to(dev)
    tw1, tb1, tw2 = (torch.from_numpy(t).to(dev) for t in (w1, b1, w2))

    # float64 restatement
    W1, B1, W2, Z, G = (t.astype(np.float64) for t in (w1, b1, w2, zp, gp))
    t0 = np.tanh(B1)
    tp = np.tanh(Z @ W1.T + B1)                                   # [P, M, S]
    w = ((tp @ W2).sum(0) + (N - P) * (t0 @ W2)) / N
    e = np.exp(w - w.max())
    beta = e / e.sum()
    out_p = (beta[None, :, None] * Z).sum(1)
    dbeta = np.einsum("pd,pmd->m", G, Z)
    c = beta * (dbeta - (beta * dbeta).sum()) / N
    q = c[None, :, None] * W2 * (1 - tp * tp)                     # [P, M, S]
    dz_p = beta[None, :, None] * G[:, None, :] + q @ W1
    dz_0 = (c[:, None] * W2 * (1 - t0 * t0)) @ W1                 # [M, D]
    dW1 = np.einsum("pms,pmd->sd", q, Z)

    out, got_beta = ops.han_semantic_forward(z, tw1, tb1, tw2)
    assert np.abs(got_beta.cpu().numpy() - beta).max() <= 1e-5
    close(out[idx].cpu().numpy(), out_p)
    assert int((out != 0).any(1).sum()) == P, "a row of out off the probes is not zero"
    del out

    dz = torch.full((N, M, D), float("nan"), device=dev)
    _, dw1, db1, dw2 = ops.han_semantic_backward(g, z, tw1, tb1, tw2, got_beta, dz_out=dz)
    changed = int((~torch.isnan(dz)).all(2).sum())
    assert changed == N * M, f"{N * M - changed} rows of dz were never written"
    close(dz[idx].cpu().numpy(), dz_p)
    off = np.setdiff1d(np.arange(2, 40), PROBES)[0]               # a node off the probes
    const = dz[int(off)].clone()                                  # [M, D]
    close(const.cpu().numpy(), dz_0)
    same = int((dz == const).all(2).sum())
    assert same == (N - P) * M, "rows off the probes differ from the constant row"
    scale = np.abs(dW1).max()
    assert np.abs(dw1.cpu().numpy() - dW1).max() <= 1e-4 * scale
    assert torch.isfinite(db1).all() and torch.isfinite(dw2).all()
