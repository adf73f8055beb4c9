#!/usr/bin/env python3
"""Regenerate tests/golden/unsup_pairs.npz from the reference implementation.

Run in the build container only (needs /root/reference, read-only):

    python tests/golden/make_golden_unsup.py

The reference's own get_context_nodes / get_negative_nodes (GraphSAGE/data_utils.py:50-70) run
under a seeded global ``random`` on a small synthetic graph given as a citation-pair stream
(the adjacency sets are built the way read_pubmed_data builds them). Stored per configuration:
the nodes, window, K, the contexts and negatives the reference returned, and the next
``random.random()`` after each call (the generator's position). Nothing from the reference is
copied: only data is written.
"""
import random
import sys
from collections import defaultdict
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent / "unsup_pairs.npz"

N_NODES = 48  # a universe small enough that candidates are rejected; node 47 is isolated
# (window, K, seed): windows on both sides of the degrees, need = window * K from 1 to 25
CONFIGS = [(5, 5, 11), (1, 1, 12), (5, 1, 13), (1, 5, 14)]


def pair_stream():
    """Degrees 1..9 over nodes 0..46: below, equal to and above both windows (1 and 5)."""
    pairs = []
    for v in range(N_NODES - 2):          # a path over 0..46: ends of degree 1, inside 2
        pairs.append((v, v + 1))
    for u in range(13, 20):               # node 3: 2 + 7 = 9 neighbours
        pairs.append((3, u))
    for u in range(30, 35):               # node 40: 2 + 5 = 7 neighbours
        pairs.append((u, 40))
    for h, us in ((10, (21, 25, 36)), (28, (5, 6, 7))):  # exactly 5 neighbours
        for u in us:
            pairs.append((h, u))
    for t in range(0, len(pairs), 3):     # repeats in the other orientation, as a cites file has
        pairs.append(pairs[t][::-1])
    return np.asarray(pairs, dtype=np.int64)


def main():
    if not REF.is_dir():
        sys.exit("the reference is not mounted at /root/reference: fixtures cannot be regenerated")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF / "GraphSAGE"))
    import data_utils as du  # reference GraphSAGE/data_utils.py

    pairs = pair_stream()
    adj = defaultdict(set)
    for a, b in pairs.tolist():
        adj[a].add(b)
        adj[b].add(a)
    deg = np.array([len(adj[v]) if v in adj else 0 for v in range(N_NODES)])
    assert deg[N_NODES - 1] == 0 and (deg[:-1] > 0).all()
    for w in (1, 5):
        assert (deg[:-1] < w).any() or w == 1
        assert (deg[:-1] == w).any() and (deg[:-1] > w).any()
    out = {"pairs": pairs, "n_nodes": np.int64(N_NODES), "deg": deg}
    universe = list(range(N_NODES))
    for c, (window, K, seed) in enumerate(CONFIGS):
        nodes = list(range(N_NODES - 1)) + [3, 0]  # every connected node, two of them twice
        random.seed(seed)
        contexts = du.get_context_nodes(nodes, adj, window)
        after_ctx = random.random()
        negatives = du.get_negative_nodes(contexts, universe, K)
        after_neg = random.random()
        out[f"case{c}_meta"] = np.asarray([window, K, seed], dtype=np.int64)
        out[f"case{c}_nodes"] = np.asarray(nodes, dtype=np.int64)
        out[f"case{c}_contexts"] = np.asarray(contexts, dtype=np.int64)
        out[f"case{c}_negatives"] = np.asarray(negatives, dtype=np.int64)
        out[f"case{c}_next"] = np.asarray([after_ctx, after_neg], dtype=np.float64)
    # the isolated node: random.choices over an empty list raises IndexError after one draw
    random.seed(15)
    try:
        du.get_context_nodes([0, N_NODES - 1, 1], adj, 5)
        raised = 0
    except IndexError:
        raised = 1
    out["iso_raises"] = np.int64(raised)
    out["iso_next"] = np.float64(random.random())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
