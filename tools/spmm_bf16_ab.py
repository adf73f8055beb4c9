"""fp32 vs bf16 feature rows on the GCN aggregation, measured in one process.

    python tools/spmm_bf16_ab.py --build-layout          (CPU side: the 8-B-per-lane variant)
    python tools/spmm_bf16_ab.py [--ns] [--layout] [--out profiles/bf16_spmm_ab_cfg2.json]

Builds the cfg2 graph as bench.py does (R-MAT 1M nodes / 10M edges, the normalised
adjacency; --ns: the north star, 10M / 100M), warms both dtypes, then times ``spmm_forward``
on fp32 X and on ``X.bfloat16()`` with device events, alternating the two in blocks until each
side has at least --seconds of timed work. Both the natural-order graph (the default policy:
fp32 takes the staged XCD form, bf16 the hub-staged form) and the column-degree-ordered graph
A P^T (what Graph_conv_layer and bench.py run: hub rows read in place; the default policy,
and for bf16 the XCD-direct and the hub-staged route each by name) are timed. Per
dtype: median and spread of the block means, edges/s, and the achieved fraction of the HBM
roofline on the compulsory bytes nnz * 8 + N * (8 + e * F) + N * 4 F (e = element size).
Parity: the bf16 result against the fp32 kernel run on ``X.bfloat16().float()``, full size.
Also times ``Graph_conv_layer(F, F)`` inference under both settings of ops.SUPPORT_DTYPE.
--layout adds the bf16 kernels built with GNN_SPMM_BF16_VW=4 (8-B loads, 4 bf16 per lane)
from lib/variants/ to the alternation: the lane-layout A/B.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak, the roofline bench.py uses
LAYOUT_TAG, LAYOUT_DEFS = "bf16vw4", ["GNN_SPMM_BF16_VW=4"]


def summary(ms, nnz, nbytes):
    m = statistics.median(ms)
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), m, max(ms)]
    return {"median_ms": m, "min_ms": min(ms), "max_ms": max(ms), "iqr_ms": q[2] - q[0],
            "blocks": len(ms), "edges_per_s": nnz / (m * 1e-3),
            "compulsory_bytes": nbytes, "hbm_fraction": nbytes / (m * 1e-3) / HBM_BYTES_PER_S}


def alternate(torch, sides, seconds, iters, libs=None):
    """sides: {name: fn}. Blocks of ``iters`` calls per side, alternating, until every side
    has >= ``seconds`` of timed work. ``libs``: {name: variant library} selected (outside the
    timed region) for that side's blocks. Returns {name: [ms per call, one per block]}."""
    from graphneuralnetwork_amd import _lib
    libs = libs or {}
    times = {k: [] for k in sides}
    total = {k: 0.0 for k in sides}
    for k, fn in sides.items():  # warm every side (plans, allocator, code objects)
        _lib.use_variant(libs.get(k))
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    while min(total.values()) < seconds * 1e3:
        for k, fn in sides.items():
            if libs:
                _lib.use_variant(libs.get(k))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            t = a.elapsed_time(b)
            total[k] += t
            times[k].append(t / iters)
    _lib.use_variant(None)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", action="store_true", help="the north star (10M nodes / 100M edges)")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side, at least")
    ap.add_argument("--layout", action="store_true", help="also time the 8-B-per-lane bf16 build")
    ap.add_argument("--build-layout", action="store_true", help="build that variant and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.build_layout:
        from graphneuralnetwork_amd.build import build_variant
        print(build_variant(LAYOUT_TAG, LAYOUT_DEFS, only=["spmm_bf16.hip"]))
        return
    import torch
    from graphneuralnetwork_amd import _lib, ops
    from graphneuralnetwork_amd.gcn import Graph_conv_layer
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    from graphneuralnetwork_amd.rmat import rmat_edges
    dev = torch.device("cuda:0")
    n, e = (10_000_000, 100_000_000) if args.ns else (1_000_000, 10_000_000)
    F = args.feat
    s, d = rmat_edges(n, e, 0)
    g = gcn_adjacency(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), n, device=dev)
    del s, d
    torch.manual_seed(0)
    X = torch.randn(n, F, device=dev)
    Xb = X.bfloat16()
    Y = torch.empty(n, F, device=dev)
    iters = 5 if args.ns else 20
    res = {"workload": "north star" if args.ns else "cfg2", "nodes": n, "nnz": g.nnz, "feat": F,
           "device": torch.cuda.get_device_name(dev), "library_stamp": _lib.load().gnn_build_stamp().decode(),
           "timing": f"device events around blocks of {iters} calls, sides alternated, "
                     f">= {args.seconds} s per side; spread over block means",
           "bytes_model": "nnz*8 + N*(8 + e*F) + N*4*F, e = element size of X"}

    def nbytes(esize):
        return g.nnz * 8 + n * (8 + esize * F) + n * 4 * F

    layout_lib = ROOT / "graphneuralnetwork_amd" / "lib" / "variants" / f"libgnn_{LAYOUT_TAG}.so"
    if args.layout and not layout_lib.exists():
        raise SystemExit(f"{layout_lib} missing: run --build-layout first")
    order = ops.column_order(g, F, 2) or ops.column_order(g, F)
    graphs = {"natural": (g, X, Xb)}
    if order is not None:
        Xo = order.permute_rows(X)
        graphs["column_ordered"] = (order.graph, Xo, Xo.bfloat16())
    for gname, (gr, x32, x16) in graphs.items():
        def run(x, **kw):
            return lambda: ops.spmm_forward(gr, x, out=Y, **kw)
        sides = {"fp32": run(x32), "bf16": run(x16)}
        if gname == "column_ordered":  # the two bf16 routes over in-place hub rows, by name
            sides["bf16_xcd_direct"] = run(x16, xcd=True)
            sides["bf16_hub_in_place"] = run(x16, xcd=False)
            sides["fp32_hub_in_place"] = run(x32, xcd=False)
        libs = None
        if args.layout:
            sides["bf16_8B_lanes"] = run(x16)
            libs = {"bf16_8B_lanes": layout_lib}
            if gname == "column_ordered":
                sides["bf16_8B_lanes_xcd_direct"] = run(x16, xcd=True)
                libs["bf16_8B_lanes_xcd_direct"] = layout_lib
        t = alternate(torch, sides, args.seconds, iters, libs)
        out = {k: summary(v, g.nnz, nbytes(4 if k.startswith("fp32") else 2))
               for k, v in t.items()}
        out["bf16_over_fp32_time"] = out["bf16"]["median_ms"] / out["fp32"]["median_ms"]
        # parity at full size: bf16 rows vs the fp32 kernel on the same (rounded) values
        y16 = ops.spmm_forward(gr, x16).clone()
        y32 = ops.spmm_forward(gr, x16.float())
        diff = (y16 - y32).abs()
        out["parity_vs_fp32_kernel_on_rounded_x"] = {
            "max_abs_diff": float(diff.max()), "max_abs_y": float(y32.abs().max()),
            "max_abs_diff_over_max_abs_y": float(diff.max() / y32.abs().max()),
            "max_rel_diff_where_abs_y_ge_1e-3_max": float(
                (diff / y32.abs())[y32.abs() >= 1e-3 * y32.abs().max()].max())}
        if args.layout:
            _lib.use_variant(layout_lib)
            out["bf16_8B_lanes"]["equal_to_default_layout_within_1e-5"] = bool(
                torch.allclose(ops.spmm_forward(gr, x16), y16, rtol=1e-5,
                               atol=1e-5 * float(y16.abs().max())))
            _lib.use_variant(None)
        del y16, y32, diff
        res[gname] = out
        print(json.dumps({gname: out}), flush=True)
    # the drop-in layer at inference: transform + aggregation, fp32 vs bf16 support
    layer = Graph_conv_layer(F, F).to(dev).eval()

    def layer_run(dtype):
        def fn():
            with torch.no_grad(), ops.support_dtype(dtype):
                layer(X, g)
        return fn
    t = alternate(torch, {"fp32": layer_run(torch.float32), "bf16": layer_run(torch.bfloat16)},
                  args.seconds / 2, iters)
    res["graph_conv_layer_inference"] = {
        k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
            "blocks": len(v)} for k, v in t.items()}
    res["graph_conv_layer_inference"]["what"] = (
        f"Graph_conv_layer({F}, {F}) forward under no_grad: MFMA transform (scattered rows "
        "where the column order applies) + SpMM with the bias epilogue; SUPPORT_DTYPE fp32 vs bf16")
    print(json.dumps({"graph_conv_layer_inference": res["graph_conv_layer_inference"]}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
