"""Generate tests/golden/metapath.npz by running the REFERENCE HAN loader's HeteroGraph.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metapath_golden.py

A fresh subprocess puts the reference's HAN directory on sys.path, builds two small seeded
scipy relations in the reference's own format (the PvsA / PvsL matrices of ACM.mat are scipy
sparse float64), runs the reference's ``HeteroGraph`` over them (HAN/utils/data_utils.py:74-89)
and stores, per relation, the COO triplets and the dense uint8 metapath adjacency it returns.
Nothing from the reference is copied: only data is written.
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


def relations(rng):
    """{'p_vs_a': 300 x 80 with a hub column, empty rows and duplicates-free valued entries,
    'p_vs_l': 300 x 40}: (row, col, val, shape) each."""
    out = {}
    n, k = 300, 80
    deg = rng.integers(1, 5, size=n)
    deg[rng.choice(n, size=25, replace=False)] = 0          # papers without an author
    deg[[0, n - 1]] = 0                                      # the first and the last row empty
    w = 1.0 / np.arange(1, k + 1) ** 1.1                     # skewed author popularity
    w /= w.sum()
    row = np.repeat(np.arange(n), deg)
    col = rng.choice(k, size=row.size, p=w)
    hub = rng.choice(np.nonzero(deg)[0], size=120, replace=False)  # author 7 wrote 120 papers
    row, col = np.concatenate([row, hub]), np.concatenate([col, np.full(hub.size, 7)])
    key = np.unique(row * k + col)                           # one stored entry per (i, j)
    row, col = key // k, key % k
    out["p_vs_a"] = (row, col, rng.integers(1, 4, size=row.size).astype(np.float64), (n, k))
    n, k = 300, 40
    row = np.repeat(np.arange(n), rng.integers(1, 3, size=n))
    col = rng.integers(0, k, size=row.size)
    key = np.unique(row * k + col)
    row, col = key // k, key % k
    out["p_vs_l"] = (row, col, np.ones(row.size, np.float64), (n, k))
    return out


def part_metapath():
    sys.path.insert(0, str(REF / "HAN"))
    import scipy.sparse as sp
    from utils.data_utils import HeteroGraph           # reference HAN/utils/data_utils.py
    rels = relations(np.random.default_rng(17))
    hg = HeteroGraph({key: sp.csr_matrix((val, (row, col)), shape=shape)
                      for key, (row, col, val, shape) in rels.items()})
    assert len(hg) == len(rels)
    out = {"keys": np.array(list(rels))}
    for key, dense in zip(rels, hg):                   # the reference's own __iter__
        row, col, val, shape = rels[key]
        assert set(np.unique(dense)) <= {0.0, 1.0}
        out[f"{key}_row"] = row.astype(np.int32)
        out[f"{key}_col"] = col.astype(np.int32)
        out[f"{key}_val"] = val.astype(np.float32)
        out[f"{key}_shape"] = np.array(shape, np.int64)
        out[f"{key}_adj"] = np.asarray(dense).astype(np.uint8)
        print(key, shape, "nnz", row.size, "edges", int(out[f"{key}_adj"].sum()))
    np.savez_compressed(HERE / "metapath.npz", **out)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    if len(sys.argv) > 1 and sys.argv[1] == "--part":
        part_metapath()
        sys.exit(0)
    if not REF.exists():
        sys.exit("the reference is not mounted at /root/reference: fixtures cannot be regenerated")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
    subprocess.run([sys.executable, __file__, "--part"], check=True, env=env,
                   cwd=tempfile.gettempdir())
