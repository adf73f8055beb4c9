"""Interleaved A/B of whole-library builds (lib/variants/libgnn_<tag>.so, built by
build.build_variant) on the default SpMM path (ops.spmm_forward) at one workload.

    python tools/lib_ab.py --build --variants base,ntcold      (CPU side)
    python tools/lib_ab.py --variants base,ntcold [--workload cfg2|ns] [--feat 128]
    python tools/lib_ab.py --op sage --dtype bf16 --workload ns --variants base,sbu4,sbu16
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# tag -> -D flags. Variant libraries export only the C-ABI (build.EXPORT_MAP), so each
# one launches its own kernels; before round 2 they did not (the kernels' weak template
# symbols bound to the main library), and every round-1 library A/B compared the main
# build with itself.
# Non-temporal loads for the cold (non-hub) gathers, so they leave the hub rows in L2:
# no change (cfg2 1.134 vs 1.136 ms, ns 14.37 vs 14.37 ms, profiles/r02q_nt_*.log).
# Prefetching the next 64-edge (col, val) chunk during the current one: no change (cfg2
# 1.133 vs 1.134 ms, ns 14.21 vs 14.23 ms, profiles/r02o_pf_*.log), not kept.
# Short rows (2..16 edges) in their own launch, 64/LPS rows per wave (LPS lanes x 4 16-B
# chunks, 2 edges in flight per lane): slower at every threshold (cfg2 1.136 ms off, 1.144
# at <= 4, 1.168 at <= 16, 1.211 at <= 64; ns 14.35 off vs 14.41), profiles/r02p_short_*.log;
# not kept: the one-wave-per-row mid path already overlaps those rows' latency.
# GCN transform grid (tools/transform_ab.py --variants, profiles/r02m_transform_ab.log):
# 512 workgroups 0.300 ms at 1M x 128 x 128, 256: 0.333, 768: 0.316, 1024: 0.30x.
# Retired with their code (DESIGN.md section 6 keeps the rows, git history the arms):
# small rows in their own launch (split*, sp*u8); occupancy caps by dynamic LDS (wg6 .. wg2);
# edge (col, val) moved to the edge slots by v_readlane + select instead of ds_bpermute:
# slower (cfg2 0.946 vs 0.870 ms, ns 11.87 vs 11.79 ms, profiles/r05u_readlane_*.log);
# the schedule of a packed task, cfg2 --ordered --bias,
# profiles/r07_lib_ab_*.log: bias in registers -2.3 .. -3.1 %, with the lean bookkeeping
# -3.0 .. -3.3 % (both kept, now the only form); the ring +5 .. +9 % (slower), 2 % less slow
# with the next chunk prefetched (parent, parent2, breg, lean, ring, ringpf).
VARIANTS = {
    "base": [],
    "tu2": ["GNN_SPMM_TASK_U=2"],
    "tu8": ["GNN_SPMM_TASK_U=8"],
    "tu16": ["GNN_SPMM_TASK_U=16"],
    "tf256": ["GNN_TF_GRID=256"],
    "tf768": ["GNN_TF_GRID=768"],
    "tf1024": ["GNN_TF_GRID=1024"],
    "u2": ["GNN_SPMM_U=2"],
    "u8": ["GNN_SPMM_U=8"],
    "small2": ["GNN_SPMM_SMALL_UNROLL=2"],
    "small8": ["GNN_SPMM_SMALL_UNROLL=8"],
    "small16": ["GNN_SPMM_SMALL_UNROLL=16"],
    "s16u8": ["GNN_SPMM_SMALL_UNROLL=16", "GNN_SPMM_U=8"],
    "s16u2": ["GNN_SPMM_SMALL_UNROLL=16", "GNN_SPMM_U=2"],
    "small32": ["GNN_SPMM_SMALL_UNROLL=32"],
    "small4": ["GNN_SPMM_SMALL_UNROLL=4"],
    "s2": ["GNN_SPMM_SMALL_UNROLL=2"],
    "s4u8": ["GNN_SPMM_SMALL_UNROLL=4", "GNN_SPMM_U=8"],
    "s2u8": ["GNN_SPMM_SMALL_UNROLL=2", "GNN_SPMM_U=8"],
    "s4u6": ["GNN_SPMM_SMALL_UNROLL=4", "GNN_SPMM_U=6"],
    "s4u12": ["GNN_SPMM_SMALL_UNROLL=4", "GNN_SPMM_U=12"],
    "s4u16": ["GNN_SPMM_SMALL_UNROLL=4", "GNN_SPMM_U=16"],
    "su2": ["GNN_SAGE_U=2"],
    "su8": ["GNN_SAGE_U=8"],
    "su16": ["GNN_SAGE_U=16"],
    "su4": ["GNN_SAGE_U=4"],
    # the same knob of the bf16-table instance (sage_bf16.hip; --op sage --dtype bf16)
    "sbu4": ["GNN_SAGE_BF16_U=4"],
    "sbu8": ["GNN_SAGE_BF16_U=8"],
    "sbu16": ["GNN_SAGE_BF16_U=16"],
    # edges per batch in spmm_items_kernel (pass 1 of the XCD-direct form; the A/B runs in
    # tools/spmm_items_ab.py --variants, which also flips ops.SPMM_ITEMS_KERNEL); the default is
    # 16 at F = 128 and 8 at F = 256
    "iu8": ["GNN_SPMM_ITEMS_U=8"],
    "iu16": ["GNN_SPMM_ITEMS_U=16"],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--only", default="spmm.hip,sage.hip,sage_bf16.hip",
                    help="--build: csrc files compiled with the variant's defines (the rest "
                         "link from the main build)")
    ap.add_argument("--seg-lens", default="", help="also time the default build at these seg_len")
    ap.add_argument("--ordered", action="store_true",
                    help="time the column-ordered graph A P^T, as bench.py does")
    ap.add_argument("--op", default="spmm", choices=["spmm", "sage"],
                    help="sage: the fused gather-mean over [M=62,401, k=10] uniform-degree-weighted "
                         "samples of the workload's graph (the cfg4 layer-0 shape)")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                    help="element type of the gathered table X")
    ap.add_argument("--bias", action="store_true",
                    help="add a bias row, as the GCN layer (and bench.py) does")
    ap.add_argument("--replay", action="store_true",
                    help="also bench.spmm_replay per variant (needs --ordered): the step with "
                         "every gather served by an L2-resident table, the schedule's own cost")
    ap.add_argument("--equal", action="store_true",
                    help="compare every variant's full output with the first variant's "
                         "(torch.equal), print one line each and fail if any differs")
    args = ap.parse_args()
    names = args.variants.split(",")  # "tag" or "tag@seg_len"
    if args.build:
        from graphneuralnetwork_amd.build import build_variant
        for n in {n.split("@")[0] for n in names}:
            print(build_variant(n, VARIANTS[n], only=[f for f in args.only.split(",") if f]))
        return
    import torch
    from graphneuralnetwork_amd import _lib
    from graphneuralnetwork_amd.ops import spmm_forward
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    from graphneuralnetwork_amd.rmat import rmat_edges
    dev = torch.device("cuda:0")
    n, e = (1_000_000, 10_000_000) if args.workload == "cfg2" else (10_000_000, 100_000_000)
    s, d = rmat_edges(n, e, 0)
    g = gcn_adjacency(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), n, device=dev)
    F = args.feat
    if args.ordered:
        from graphneuralnetwork_amd.ops import column_order
        o = column_order(g, F)
        g = g if o is None else o.graph
    X = torch.randn(n, F, device=dev)
    if args.dtype == "bf16":
        X = X.bfloat16()
    Y = torch.empty(n, F, device=dev)
    nbytes = g.nnz * (8 + 4 * F) + n * (8 + 4 * F)
    if args.op == "sage":
        from graphneuralnetwork_amd.ops import sage_gather_aggregate
        from graphneuralnetwork_amd.sampler import sample_neighbors
        deg = g.rowptr[1:] - g.rowptr[:-1]
        cand = torch.nonzero(deg > 0).view(-1)
        nodes = cand[torch.randperm(cand.numel(), device=dev)[:62401]]
        idx = sample_neighbors(g, nodes, 10, 0)
        Y = torch.empty(idx.shape[0], F, device=dev)
        nbytes = idx.numel() * (X.element_size() * F + 8) + idx.shape[0] * 4 * F

        def spmm_forward(g_, X_, out=None, seg_len=None):  # noqa: F811 -- same harness
            return sage_gather_aggregate(X_, idx, "MEAN", check=False, out=out)
    if args.bias and args.op == "spmm":
        import functools
        spmm_forward = functools.partial(spmm_forward, bias=torch.randn(F, device=dev))
    ref = spmm_forward(g, X, out=torch.empty_like(Y)).clone()
    libs = {v: ROOT / "graphneuralnetwork_amd" / "lib" / "variants" /
            f"libgnn_{v.split('@')[0]}.so" for v in names}
    seg = {v: int(v.split("@")[1]) for v in names if "@" in v}
    seg.update({f"seg{sl}": int(sl) for sl in args.seg_lens.split(",") if sl})
    names = names + [k for k in seg if k not in names]
    if args.equal:
        outs = {}
        for v in names:
            _lib.use_variant(libs[v] if v in libs and libs[v].exists() else None)
            Yv = torch.full_like(Y, float("nan"))
            spmm_forward(g, X, out=Yv, seg_len=seg.get(v))
            torch.cuda.synchronize()
            outs[v] = Yv
        same = {v: bool(torch.equal(outs[v], outs[names[0]])) for v in names}
        for v in names:
            print(json.dumps({"variant": v, "workload": args.workload, "feat": F,
                              "ordered": args.ordered, "bias": args.bias,
                              "library": libs[v].name if v in libs and libs[v].exists()
                              else "default build",
                              "rows": int(Y.shape[0]), "finite": bool(outs[v].isfinite().all()),
                              f"torch_equal_to_{names[0]}": same[v]}), flush=True)
        del outs
        if not all(same.values()):
            sys.exit(1)
    if args.replay and args.op == "spmm":
        import bench
        fwd = spmm_forward
        kw = fwd.keywords if hasattr(fwd, "keywords") else {}
        for v in names:
            _lib.use_variant(libs[v] if v in libs and libs[v].exists() else None)
            rp = bench.spmm_replay(g, X, kw.get("bias"), Y)
            print(json.dumps({"variant": v, "workload": args.workload, "replay": rp and {
                k: rp[k] for k in ("as_built_ms", "hub_gathers_in_L2_ms", "all_gathers_in_L2_ms")}}),
                flush=True)
    times = {v: [] for v in names}
    for r in range(args.rounds):
        for v in names:
            _lib.use_variant(libs[v] if v in libs and libs[v].exists() else None)
            sl = seg.get(v)
            spmm_forward(g, X, out=Y, seg_len=sl)
            torch.cuda.synchronize()
            if r == 0 and sl is None:
                assert torch.equal(Y, ref), v
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20 if args.op == "sage" else 5):
                spmm_forward(g, X, out=Y, seg_len=sl)
            b.record()
            torch.cuda.synchronize()
            times[v].append(a.elapsed_time(b) / (20 if args.op == "sage" else 5))
    for v, t in times.items():
        m = statistics.median(t)
        print(json.dumps({"variant": v, "op": args.op, "dtype": args.dtype,
                          "workload": args.workload, "feat": F, "median_ms": m,
                          "min_ms": min(t), "max_ms": max(t),
                          "algo_GBps": nbytes / m / 1e6}), flush=True)


if __name__ == "__main__":
    main()
