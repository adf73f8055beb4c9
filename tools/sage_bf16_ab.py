"""fp32 vs bf16 feature table on the GraphSAGE gathers, measured in one process.

    python tools/sage_bf16_ab.py [--small] [--out profiles/bf16_sage_ab_cfg4.json]

Builds the cfg4 workload as bench.py does (R-MAT 10M nodes / 100M edges, symmetric adjacency
relabelled by degree, a 10M x 128 table, 8192 seeds, fanout [25, 10]; --small: 1M / 10M for a
quick look), samples one batch, then times on the fp32 table and on ``table.bfloat16()`` with
device events, alternating the two in blocks until each side has at least --seconds of timed
work:

  * the layer-0 gather-mean (``sage_gather_aggregate`` over the frontier's [M, 10] map),
  * the concat form (``sage_gather_concat``: centre rows + mean in one launch),
  * the MEAN / MAX / MAXPOOL 2-layer inference forwards (``GraphSAGE.forward`` in eval mode).

Per side: median and min-max of the block means, and for the two gathers the achieved
fraction of the HBM roofline on the compulsory bytes (distinct table rows once + the index
map + the output). bf16 counts as an improvement only where the two block ranges do not
overlap (``ranges_overlap``). Parity: bf16 against the fp32 kernel on ``table.bfloat16()
.float()``.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak, the roofline bench.py uses


def summary(ms, nbytes=None):
    m = statistics.median(ms)
    out = {"median_ms": m, "min_ms": min(ms), "max_ms": max(ms), "blocks": len(ms)}
    if nbytes is not None:
        out["compulsory_bytes"] = nbytes
        out["hbm_fraction"] = nbytes / (m * 1e-3) / HBM_BYTES_PER_S
    return out


def compare(t, nbytes=None):
    """{fp32, bf16} block means -> both summaries, the ratio and whether the ranges overlap."""
    out = {k: summary(v, nbytes[k] if nbytes else None) for k, v in t.items()}
    out["bf16_over_fp32_time"] = out["bf16"]["median_ms"] / out["fp32"]["median_ms"]
    out["ranges_overlap"] = not (out["bf16"]["max_ms"] < out["fp32"]["min_ms"]
                                 or out["fp32"]["max_ms"] < out["bf16"]["min_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1M nodes / 10M edges (not cfg4)")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side, at least")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from graphneuralnetwork_amd import _lib
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    from graphneuralnetwork_amd.ops import sage_gather_aggregate, sage_gather_concat
    from graphneuralnetwork_amd.rmat import rmat_edges
    from graphneuralnetwork_amd.sampler import degree_ordered, sample_batch, symmetric_adjacency
    from spmm_bf16_ab import alternate
    dev = torch.device("cuda:0")
    n, e = (1_000_000, 10_000_000) if args.small else (10_000_000, 100_000_000)
    F = H = args.feat
    s, d = rmat_edges(n, e, 0)
    adj = symmetric_adjacency(s, d, n, device=dev)
    del s, d
    adj, _, _ = degree_ordered(adj)
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(n, F, device=dev, generator=gen)
    table16 = table.bfloat16()
    deg = adj.rowptr[1:] - adj.rowptr[:-1]
    cand = torch.nonzero(deg > 0).view(-1)
    seeds = cand[torch.randperm(cand.numel(), device=dev, generator=gen)[:8192]]
    batch = sample_batch(adj, seeds, (25, 10), seed=0)
    idx, sid = batch.frontier_nbrs, batch.frontier
    M, k = idx.shape
    iters = 20
    res = {"workload": "cfg4" if not args.small else "small", "nodes": n, "edges": e, "feat": F,
           "seeds": int(seeds.numel()), "fanout": [25, 10], "frontier": M, "k_layer0": k,
           "table_bytes": {"fp32": n * F * 4, "bf16": n * F * 2},
           "device": torch.cuda.get_device_name(dev),
           "library_stamp": _lib.load().gnn_build_stamp().decode(),
           "timing": f"device events around blocks of {iters} calls, sides alternated, "
                     f">= {args.seconds} s per side; median and min-max over block means",
           "bytes_model": "distinct gathered rows * e*F + M*k*8 (+ M*8 centre ids) + output "
                          "(M*4F, or M*8F for the concat form), e = element size of the table"}
    distinct = int(torch.unique(idx).numel())
    distinct_c = int(torch.unique(torch.cat([idx.reshape(-1), sid])).numel())
    res["distinct_rows_gathered"] = distinct

    out = torch.empty((M, F), device=dev)
    buf = torch.empty((M, 2 * F), device=dev)
    t = alternate(torch, {
        "fp32": lambda: sage_gather_aggregate(table, idx, "MEAN", check=False, out=out),
        "bf16": lambda: sage_gather_aggregate(table16, idx, "MEAN", check=False, out=out)},
        args.seconds, iters)
    res["layer0_gather_mean"] = compare(
        t, {k_: distinct * es * F + M * k * 8 + M * 4 * F for k_, es in (("fp32", 4), ("bf16", 2))})
    print(json.dumps({"layer0_gather_mean": res["layer0_gather_mean"]}), flush=True)
    t = alternate(torch, {
        "fp32": lambda: sage_gather_concat(table, sid, idx, "MEAN", check=False, out=buf),
        "bf16": lambda: sage_gather_concat(table16, sid, idx, "MEAN", check=False, out=buf)},
        args.seconds, iters)
    res["layer0_concat_mean"] = compare(
        t, {k_: distinct_c * es * F + M * (k + 1) * 8 + M * 8 * F
            for k_, es in (("fp32", 4), ("bf16", 2))})
    print(json.dumps({"layer0_concat_mean": res["layer0_concat_mean"]}), flush=True)

    # parity: the bf16 kernels against the fp32 kernels on the same (rounded) values
    t16f = table16.float()
    y16 = sage_gather_aggregate(table16, idx, "MEAN", check=False)
    y32 = sage_gather_aggregate(t16f, idx, "MEAN", check=False)
    res["parity_vs_fp32_kernel_on_rounded_table"] = {
        "mean_max_abs_diff": float((y16 - y32).abs().max()),
        "mean_max_abs": float(y32.abs().max()),
        "argmax_equal": bool(torch.equal(sage_gather_aggregate(table16, idx, "MAX", check=False),
                                         sage_gather_aggregate(t16f, idx, "MAX", check=False))),
        "maxpool_equal": bool(torch.equal(
            sage_gather_aggregate(table16, idx, "MAXPOOL", check=False),
            sage_gather_aggregate(t16f, idx, "MAXPOOL", check=False))),
        "concat_self_equal": bool(torch.equal(
            sage_gather_concat(table16, sid, idx, "MEAN", check=False)[:, :F], t16f[sid]))}
    del t16f, y16, y32

    for agg in ("MEAN", "MAX", "MAXPOOL"):
        torch.manual_seed(0)
        net = GraphSAGE(2, F, H, False, agg_func=agg, Unsupervised=False,
                        class_size=3).to(dev).eval()

        def fwd(tab):
            fargs = batch.forward_args(tab)

            def fn():
                with torch.no_grad():
                    net(*fargs, None, None, None, None, None)
            return fn
        t = alternate(torch, {"fp32": fwd(table), "bf16": fwd(table16)}, args.seconds, iters)
        res[f"forward_{agg}"] = compare(t)
        print(json.dumps({f"forward_{agg}": res[f"forward_{agg}"]}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
