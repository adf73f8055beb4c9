"""Metapath graphs on the device (hetero.metapath_graph over csrc/relation_product.hip) against
(a) the reference's own line, scipy ``B * B.T`` then ``> 0`` on the host CPU, and (b) the torch
restatement ``hetero.relation_product_torch`` on the same device tensors, in one process.

    python tools/metapath_ab.py --out profiles/metapath_ab.json

Relations: n papers x k authors, ``--per-row`` (3) authors per paper drawn with
``numpy.random.default_rng(seed).choice(k, p ~ 1 / (rank + 1) ** 0.5)`` (a Zipf-like author
popularity, exponent 0.5), duplicates kept; sizes 3,025 x 6,000 (ACM-like), 100K x 40K and
1M x 400K. Every timed call is wall clock around the call and a device synchronise (the count
call reads nnz back, so the host is part of the work); blocks of calls, the sides alternated,
median and min-max of the block means. Peak memory is torch.cuda.max_memory_allocated above
what is allocated before the call (the inputs).

``--trace``: only 2 + 5 builds at 1M x 400K, for the per-kernel times of a profiler run

    rocprofv3 --kernel-trace --stats -d bench_out/metapath_trace -o run --output-format csv -- \
        python3 tools/metapath_ab.py --trace --out bench_out/unused.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"acm_like": (3025, 6000), "100K": (100_000, 40_000), "1M": (1_000_000, 400_000)}
EXPONENT = 0.5


def relation(n, k, per_row, seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, k + 1) ** EXPONENT
    p /= p.sum()
    row = np.repeat(np.arange(n, dtype=np.int64), per_row)
    col = rng.choice(k, size=row.size, p=p).astype(np.int64)
    return row, col


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "blocks": len(ms)}


def timed_blocks(sides, seconds, block, sync):
    """{name: [ms per call, one per block]}: blocks of ``block`` calls per side, alternating,
    until every side has ``seconds`` of timed work (at least 3 blocks each)."""
    times = {k: [] for k in sides}
    total = {k: 0.0 for k in sides}
    for fn in sides.values():
        fn()
    sync()
    while min(total.values()) < seconds or min(len(v) for v in times.values()) < 3:
        for k, fn in sides.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            sync()
            t = time.perf_counter() - t0
            total[k] += t
            times[k].append(t * 1e3 / block)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per side, at least")
    ap.add_argument("--per-row", type=int, default=3)
    ap.add_argument("--shapes", default="acm_like,100K,1M")
    ap.add_argument("--no-model", action="store_true", help="skip the HANLayer forward")
    ap.add_argument("--trace", action="store_true", help="7 builds at 1M x 400K (for a profiler)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/metapath_ab.py needs a ROCm device")
    from graphneuralnetwork_amd import _lib, han, hetero
    from graphneuralnetwork_amd.graph import CsrGraph, from_coo
    dev = torch.device("cuda:0")

    def sync():
        torch.cuda.synchronize(dev)

    def device_relation(n, k, seed):
        row, col = relation(n, k, args.per_row, seed)
        b = from_coo(torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev),
                     torch.ones(row.size, device=dev), n, k, check=False)
        return row, col, b

    if args.trace:
        n, k = SHAPES["1M"]
        _, _, b = device_relation(n, k, 0)
        bt = b.transpose()
        for _ in range(7):
            hetero.relation_product(b, bt)
        sync()
        return

    try:
        import scipy.sparse as sp
        host_line = "scipy: C = B * B.T; C > 0 (csr float64, no .toarray())"
    except ImportError:
        sp = None
        host_line = "torch.sparse.mm(B, B.T) on CPU tensors (scipy is not importable)"
    s_max, m_max = hetero.class_limits()
    res.update({"device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "generator": f"numpy default_rng(seed).choice(k, p ~ 1/(rank+1)^{EXPONENT}), "
                             f"{args.per_row} entries per row, duplicates kept, seed 0",
                "host_line": host_line, "class_limits": {"short_max": s_max, "mid_max": m_max},
                "timing": "wall clock around blocks of calls and a device synchronise, sides "
                          f"alternated, >= {args.seconds} s and >= 3 blocks per side; median "
                          "and min-max over block means"})
    shapes = {}
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        row, col, b = device_relation(n, k, 0)
        bt = b.transpose()
        sync()
        g = hetero.relation_product(b, bt)
        deg_k = torch.bincount(b.col.to(torch.int64), minlength=k)
        ub = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(
            0, torch.from_numpy(row).to(dev), deg_k[b.col.to(torch.int64)])
        r = {"n": n, "k": k, "nnz_B": int(b.nnz), "max_column_degree": int(deg_k.max()),
             "nnz_C": int(g.nnz), "partial_products_sum_ub": int(ub.sum()),
             "max_ub": int(ub.max()),
             "rows_by_class": {"short": int((ub <= s_max).sum()),
                               "mid": int(((ub > s_max) & (ub <= m_max)).sum()),
                               "heavy": int((ub > m_max).sum())},
             "workspace_bytes": int(_lib.load().gnn_relation_product_workspace_bytes(
                 n, k, n, b.nnz, bt.nnz))}
        del g, ub, deg_k
        block = 20 if n <= 3025 else 4 if n <= 100_000 else 1
        # (b) the kernels against the torch restatement, same device tensors
        t = timed_blocks({"kernels": lambda: hetero.relation_product(b, bt),
                          "torch_restatement": lambda: hetero.relation_product_torch(b, bt)},
                         args.seconds, block, sync)
        r["product_device"] = {k_: summary(v) for k_, v in t.items()}
        r["product_device"]["torch_over_kernels"] = (
            r["product_device"]["torch_restatement"]["median_ms"]
            / r["product_device"]["kernels"]["median_ms"])
        peak = {}
        for side, fn in (("kernels", hetero.relation_product),
                         ("torch_restatement", hetero.relation_product_torch)):
            sync()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            out = fn(b, bt)
            sync()
            peak[side] = torch.cuda.max_memory_allocated(dev) - base
            peak[side + "_result_bytes"] = int(out.rowptr.numel() * 8 + out.col.numel() * 8)
            del out
        r["peak_bytes_above_inputs"] = peak
        a_, b_ = hetero.relation_product(b, bt), hetero.relation_product_torch(b, bt)
        r["kernels_equal_torch"] = bool(torch.equal(a_.rowptr, b_.rowptr)
                                        and torch.equal(a_.col, b_.col))
        del a_, b_
        # (a) metapath_graph (transpose + count + fill) against the reference's host line
        if sp is not None:
            B = sp.csr_matrix((np.ones(row.size), (row, col)), shape=(n, k))

            def host():
                C = B * B.T
                return C > 0
        else:
            Bt = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])),
                                         torch.ones(row.size), (n, k)).coalesce()

            def host():
                return torch.sparse.mm(Bt, Bt.t()) > 0
        def device():  # a fresh CsrGraph each call: the transpose is built, not read from b's cache
            return hetero.metapath_graph(CsrGraph(b.rowptr, b.col, b.val, n, k))

        t = timed_blocks({"device_metapath_graph": device,
                          "host_reference_line": host},
                         args.seconds, 1 if n > 3025 else 5, sync)
        r["metapath_vs_host"] = {k_: summary(v) for k_, v in t.items()}
        r["metapath_vs_host"]["host_over_device"] = (
            r["metapath_vs_host"]["host_reference_line"]["median_ms"]
            / r["metapath_vs_host"]["device_metapath_graph"]["median_ms"])
        if sp is not None:
            r["host_nnz_C"] = int(host().nnz)
        shapes[name] = r
        res["shapes"] = shapes
        print(json.dumps({name: r}), flush=True)
        write()
        del b, bt
        torch.cuda.empty_cache()

    if args.no_model or "1M" not in shapes:
        return
    # a HANLayer inference forward over three metapath graphs built this way (seeds 0, 1, 2)
    n, k = SHAPES["1M"]
    gs = []
    for seed in range(3):
        _, _, b = device_relation(n, k, seed)
        gs.append(hetero.metapath_graph(b))
        del b
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(n, 64, device=dev, generator=gen)
    torch.manual_seed(0)
    layer = han.HANLayer(3, 64, 8, 8, 0.6).to(dev).eval()

    def infer():
        with torch.no_grad():
            return layer(gs, X)

    for _ in range(2):
        infer()
    t = timed_blocks({"forward": infer}, args.seconds, 2, sync)
    res["hanlayer_inference_1M"] = {"what": "HANLayer(3, 64, 8, 8, 0.6).eval() forward over three "
                                            "device-built metapath graphs (seeds 0, 1, 2)",
                                    "edges_per_graph": [int(g.nnz) for g in gs],
                                    **summary(t["forward"])}
    print(json.dumps({"hanlayer_inference_1M": res["hanlayer_inference_1M"]}), flush=True)
    write()


if __name__ == "__main__":
    main()
