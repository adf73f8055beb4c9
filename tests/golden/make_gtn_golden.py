"""Generate tests/golden/gtn.npz by running the REFERENCE GTN model.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gtn_golden.py

A fresh subprocess puts the reference's GTN directory on sys.path, builds a small seeded
heterogeneous graph (60 papers, 50 authors, 6 subjects; relations PA, AP, PS, SP and I as the
reference's dense [N, N, T] tensor), runs the reference's ``GTN_Model(5, 2, 12, 8, 3, L, True)``
for L = 1, 2, 3 in fp32 with explicit conv weights (the reference never initialises them) and
stores the inputs, every parameter, ``y``, ``Ws`` and the gradient of every parameter after
``F.cross_entropy(y, labels).backward()``. Every paper has an author and a subject and every
author and subject has a paper, so no off-diagonal column of any H is empty and the reference's
gradients are finite (asserted). Nothing from the reference is copied: only data is written.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
N_PAPER, N_AUTHOR, N_SUBJECT = 60, 50, 6
LAYERS = (1, 2, 3)


def graph(rng):
    """(pa, ps): paper-author and paper-subject pairs. Author 0 is a hub with 40 papers; every
    paper has at least one author and exactly one subject; every author and subject is used."""
    pairs = {(int(p), 0) for p in rng.choice(N_PAPER, size=40, replace=False)}
    for a in range(1, N_AUTHOR):                      # every author has a paper
        pairs.add((int(rng.integers(N_PAPER)), a))
    for p in range(N_PAPER):                          # every paper has an author, some two more
        for a in rng.integers(1, N_AUTHOR, size=int(rng.integers(1, 4))):
            pairs.add((p, int(a)))
    pa = np.array(sorted(pairs), np.int64)
    subj = rng.integers(0, N_SUBJECT, size=N_PAPER)
    subj[:N_SUBJECT] = np.arange(N_SUBJECT)           # every subject has a paper
    ps = np.stack([np.arange(N_PAPER), subj], 1).astype(np.int64)
    return pa, ps


def part_gtn():
    sys.path.insert(0, str(REF / "GTN"))
    import torch
    import torch.nn.functional as F
    from models.GTN import GTN_Model                  # reference GTN/models/GTN.py
    rng = np.random.default_rng(23)
    pa, ps = graph(rng)
    n = N_PAPER + N_AUTHOR + N_SUBJECT
    a0, s0 = N_PAPER, N_PAPER + N_AUTHOR
    rels = [(pa[:, 0], pa[:, 1] + a0), (pa[:, 1] + a0, pa[:, 0]),
            (ps[:, 0], ps[:, 1] + s0), (ps[:, 1] + s0, ps[:, 0]),
            (np.arange(n), np.arange(n))]
    A = np.zeros((n, n, len(rels)), np.uint8)
    out = {"n": np.array(n, np.int64), "names": np.array(["PA", "AP", "PS", "SP", "I"])}
    for t, (row, col) in enumerate(rels):
        A[row, col, t] = 1
        out[f"rel{t}_row"], out[f"rel{t}_col"] = row.astype(np.int32), col.astype(np.int32)
    out["A"] = A
    X = rng.standard_normal((n, 12)).astype(np.float32)
    target = rng.choice(N_PAPER, size=30, replace=False).astype(np.int64)
    labels = rng.integers(0, 3, size=target.size).astype(np.int64)
    out.update(X=X, target_x=target, labels=labels)
    At, Xt = torch.from_numpy(A.astype(np.float32)), torch.from_numpy(X)
    for L in LAYERS:
        torch.manual_seed(100 + L)
        model = GTN_Model(5, 2, 12, 8, 3, L, True)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("conv1.weight") or name.endswith("conv2.weight"):
                    p.copy_(torch.from_numpy(
                        rng.standard_normal(tuple(p.shape)).astype(np.float32)))
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        y, Ws = model(At, Xt, torch.from_numpy(target))
        F.cross_entropy(y, torch.from_numpy(labels)).backward()
        out[f"L{L}_keys"] = np.array(list(state))
        for k, v in state.items():
            out[f"L{L}_param_{k}"] = v.numpy()
        out[f"L{L}_y"] = y.detach().numpy()
        for i, W in enumerate(Ws):
            for j, w in enumerate(W):
                out[f"L{L}_W_{i}_{j}"] = w.numpy()
        for name, p in model.named_parameters():
            if p.requires_grad and p.grad is not None:   # `bias` is never used by forward
                g = p.grad.numpy()
                assert np.isfinite(g).all(), (L, name)
                out[f"L{L}_grad_{name}"] = g
        print(f"L={L}: y {tuple(y.shape)} max|y| {float(y.detach().abs().max()):.4f}, "
              f"{sum(1 for _ in model.parameters())} parameters")
    np.savez_compressed(HERE / "gtn.npz", **out)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    if len(sys.argv) > 1 and sys.argv[1] == "--part":
        part_gtn()
        sys.exit(0)
    if not REF.exists():
        sys.exit("the reference is not mounted at /root/reference: fixtures cannot be regenerated")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
    subprocess.run([sys.executable, __file__, "--part"], check=True, env=env,
                   cwd=tempfile.gettempdir())
