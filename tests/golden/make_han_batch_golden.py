"""Generate tests/golden/han_batch.npz by running the REFERENCE HAN loader's collect_f.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_han_batch_golden.py

A fresh subprocess puts the reference's HAN directory on sys.path, rebuilds the reference's
``HeteroGraph`` from the relations stored in metapath.npz, creates seeded features and labels
and runs the reference's own ``collect_f`` (HAN/utils/data_utils.py:92-101) over six batches,
one of them the first batch of the reference's shuffled ``DataLoader``. Per batch it stores the
ids, each dense slice as uint8 and the features and labels returned; for the 65-id batch also
the eval logits of the reference's ``HANModel`` with seeded parameters. Nothing from the
reference is copied: only data is written.
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
MODEL = (2, 16, 8, 3, [2], 0.6)                      # HANModel's constructor arguments


def _q(rng, shape, scale=64, lim=48):
    """Dyadic random values k/scale, k in [-lim, lim]."""
    return (rng.integers(-lim, lim + 1, size=shape) / scale).astype(np.float32)


def part_han_batch():
    sys.path.insert(0, str(REF / "HAN"))
    import scipy.sparse as sp
    import torch
    from torch.utils.data import DataLoader
    from models import HANModel                        # reference HAN/models/__init__.py
    from utils.data_utils import HeteroGraph, collect_f  # reference HAN/utils/data_utils.py
    gd = np.load(HERE / "metapath.npz")
    keys = [str(k) for k in gd["keys"]]
    hg = HeteroGraph({k: sp.csr_matrix((gd[f"{k}_val"].astype(np.float64),
                                        (gd[f"{k}_row"], gd[f"{k}_col"])),
                                       shape=tuple(int(v) for v in gd[f"{k}_shape"]))
                      for k in keys})
    rng = np.random.default_rng(23)
    n = int(gd[f"{keys[0]}_shape"][0])
    features = _q(rng, (n, 16), 32, 32)
    labels = rng.integers(0, 3, size=n)
    batchify = collect_f(hg, features, labels)
    for k, adj in zip(keys, batchify.HGs_adj):         # the loader's graphs are metapath.npz's
        assert np.array_equal(adj.numpy().astype(np.uint8), gd[f"{k}_adj"])
    torch.manual_seed(0)
    loader = DataLoader(np.arange(n), batch_size=32, shuffle=True, collate_fn=batchify)
    first = next(iter(loader))
    perm = rng.permutation(n)
    batches = {
        "one": [int(perm[0])],
        "loader": None,                                # what the DataLoader drew, read back below
        "b64": [int(v) for v in rng.permutation(n)[:64]],
        "b65": [int(v) for v in rng.permutation(n)[:65]],
        "all": [int(v) for v in perm],
        "repeat": [5, 17, 5, 200, 17, 17, 0, 299, 5, 121, 200, 64],
    }
    out = {"keys": np.array(keys), "batches": np.array(list(batches)), "features": features,
           "labels": labels.astype(np.int64), "model": np.array(MODEL[:4] + (MODEL[4][0],))}
    for name, ids in batches.items():
        if ids is None:
            adjs, feat, lab = first
            # the ids the sampler drew: the same generator state draws the same permutation
            torch.manual_seed(0)
            ids = [int(v) for v in next(iter(DataLoader(np.arange(n), batch_size=32, shuffle=True,
                                                        collate_fn=lambda d: list(d))))]
            assert torch.equal(feat, batchify.features[ids])
        else:
            # numpy integers: what a DataLoader over an index array hands its collate_fn
            adjs, feat, lab = batchify([np.int64(v) for v in ids])
        out[f"{name}_idx"] = np.asarray(ids, np.int64)
        for k, a in zip(keys, adjs):
            a = a.numpy()
            assert set(np.unique(a)) <= {0.0, 1.0} and a.shape == (len(ids), len(ids))
            out[f"{name}_{k}"] = a.astype(np.uint8)
        out[f"{name}_features"] = feat.numpy().astype(np.float32)
        out[f"{name}_labels"] = lab.numpy().astype(np.int64)
        print(name, len(ids), [int(out[f"{name}_{k}"].sum()) for k in keys],
              [int((out[f"{name}_{k}"].sum(1) == 0).sum()) for k in keys])
    net = HANModel(*MODEL)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.from_numpy(_q(rng, tuple(p.shape), 64, 40)))
    net.eval()
    adjs, feat, _ = batchify([np.int64(v) for v in batches["b65"]])
    with torch.no_grad():
        logits = net([a.float() for a in adjs], feat)
    out["b65_logits"] = logits.numpy().astype(np.float32)
    for k, v in net.state_dict().items():
        out[f"sd_{k}"] = v.numpy()
    np.savez_compressed(HERE / "han_batch.npz", **out)
    print("han_batch", logits.shape, (HERE / "han_batch.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    if len(sys.argv) > 1 and sys.argv[1] == "--part":
        part_han_batch()
        sys.exit(0)
    if not REF.exists():
        sys.exit("the reference is not mounted at /root/reference: fixtures cannot be regenerated")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
    subprocess.run([sys.executable, __file__, "--part"], check=True, env=env,
                   cwd=tempfile.gettempdir())
