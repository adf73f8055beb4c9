"""HAN mini-batches on the device (hetero.induced_subgraphs over csrc/induced_subgraph.hip)
against (a) the torch restatement ``hetero.induced_subgraph_torch`` on the same device tensors and,
for structure only, the two chained ``relation_product`` calls S.A then .S^T the operation replaces;
(b) a HANModel training step per batch with the slice's share of it, and at the ACM-like size the
reference's own dense line ``A[idx][:, idx]`` plus ``from_dense``; all in one process.

    python tools/han_batch_ab.py --out profiles/han_batch_ab.json
    python tools/han_batch_ab.py --shapes 100K,1M --batches all --no-model \
        --out profiles/han_batch_ab_all.json      # the whole graph permuted: heavy rows

Graphs: three metapath graphs per size, built as tools/metapath_ab.py builds them (n papers x k
authors, 3 authors a paper, seeds 0, 1, 2): 3,025 x 6,000 (ACM-like), 100K x 40K and 1M x 400K.
A batch is a prefix of ``numpy.random.default_rng(7).permutation(n)``. Every timed call is wall
clock around the call and a device synchronise (the slice reads the totals and the status back,
so the host is part of the work); blocks of calls, the sides alternated, median and min-max of the
block means. Peak memory is torch.cuda.max_memory_allocated above what is allocated before the
call (the inputs).

``--trace``: only 2 + 10 slices at 1M x 400K and b = 8,192, for the per-kernel times of a profiler

    rocprofv3 --kernel-trace --stats -d bench_out/han_batch_trace -o run --output-format csv -- \
        python3 tools/han_batch_ab.py --trace --out bench_out/unused.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from metapath_ab import SHAPES, relation, summary, timed_blocks  # noqa: E402

BATCHES = "32,1024,8192,65536"
STEP_BATCH = 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per side, at least")
    ap.add_argument("--per-row", type=int, default=3)
    ap.add_argument("--shapes", default="acm_like,100K,1M")
    ap.add_argument("--batches", default=BATCHES, help="batch sizes; 'all' is a permutation of "
                                                       "every node")
    ap.add_argument("--no-model", action="store_true", help="skip the training steps")
    ap.add_argument("--trace", action="store_true", help="12 slices at 1M, b = 8,192 (profiler)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/han_batch_ab.py needs a ROCm device")
    from graphneuralnetwork_amd import _lib, graph, han, hetero
    from graphneuralnetwork_amd.graph import CsrGraph, from_coo, from_dense
    dev = torch.device("cuda:0")

    def sync():
        torch.cuda.synchronize(dev)

    def metapath_graphs(n, k):
        gs = []
        for seed in range(3):
            row, col = relation(n, k, args.per_row, seed)
            b = from_coo(torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev),
                         torch.ones(row.size, device=dev), n, k, check=False)
            gs.append(hetero.metapath_graph(b))
            del b
        sync()
        return gs

    def batch(n, b):
        return torch.from_numpy(np.random.default_rng(7).permutation(n)[:b].copy()).to(dev)

    def block_for(fn):
        fn()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return max(1, min(50, int(0.05 / max(time.perf_counter() - t0, 1e-6))))

    def peak_of(fn):
        sync()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        sync()
        peak = torch.cuda.max_memory_allocated(dev) - base
        return peak, out

    if args.trace:
        n, k = SHAPES["1M"]
        gs = metapath_graphs(n, k)
        idx = batch(n, STEP_BATCH)
        for _ in range(12):
            hetero.induced_subgraphs(gs, idx)
        sync()
        return

    s_max, m_max, lds_bits = hetero.subgraph_class_limits()
    res.update({"device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "graphs": "three metapath graphs per size (tools/metapath_ab.py's relations, "
                          f"{args.per_row} entries per row, seeds 0, 1, 2)",
                "batch": "prefix of numpy default_rng(7).permutation(n)",
                "class_limits": {"short_max": s_max, "mid_max": m_max, "lds_bits": lds_bits},
                "timing": "wall clock around blocks of calls and a device synchronise, sides "
                          f"alternated, >= {args.seconds} s and >= 3 blocks per side; median "
                          "and min-max over block means"})
    shapes = {}
    kept = {}
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        gs = metapath_graphs(n, k)
        r = {"n": n, "k": k, "nnz": [int(g.nnz) for g in gs], "batches": {}}
        for b in sorted({n if b == "all" else min(int(b), n) for b in args.batches.split(",")}):
            idx = batch(n, b)

            def kernels():
                return hetero.induced_subgraphs(gs, idx)

            def restated():
                return [hetero.induced_subgraph_torch(g, idx) for g in gs]

            S = from_coo(torch.arange(b, device=dev), idx, torch.ones(b, device=dev), b, n,
                         check=False)
            St = S.transpose()

            def two_products():   # structure only; S and S^T given
                return [hetero.relation_product(hetero.relation_product(S, g), St) for g in gs]

            got, want, old = kernels(), restated(), two_products()
            equal = all(torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col)
                        and torch.equal(x.val, y.val) for x, y in zip(got, want))
            equal_old = all(torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col)
                            for x, y in zip(got, old))
            deg = torch.cat([g.rowptr[1:] - g.rowptr[:-1] for g in got])
            e = {"b": b, "nnz_C": [int(g.nnz) for g in got],
                 "selected_rows_entries": [int((g.rowptr[idx + 1] - g.rowptr[idx]).sum())
                                           for g in gs],
                 "rows_by_class": {"short": int(((deg > 0) & (deg <= s_max)).sum()),
                                   "mid": int(((deg > s_max) & (deg <= m_max)).sum()),
                                   "heavy": int((deg > m_max).sum()),
                                   "edgeless": int((deg == 0).sum())},
                 "kernels_equal_torch": bool(equal), "kernels_equal_two_products": bool(equal_old),
                 "workspace_bytes": int(_lib.load().gnn_induced_subgraph_workspace_bytes(n, b))}
            del got, want, old, deg
            sides = {"kernels": kernels, "torch_restatement": restated,
                     "two_relation_products": two_products}
            t = timed_blocks(sides, args.seconds, block_for(restated), sync)
            e["slice_3_graphs"] = {k_: summary(v) for k_, v in t.items()}
            for other in ("torch_restatement", "two_relation_products"):
                e["slice_3_graphs"][other + "_over_kernels"] = (
                    e["slice_3_graphs"][other]["median_ms"]
                    / e["slice_3_graphs"]["kernels"]["median_ms"])
            peak = {}
            for side, fn in sides.items():
                peak[side], out = peak_of(fn)
                if side == "kernels":
                    peak["result_bytes"] = int(sum(g.rowptr.numel() * 8 + g.col.numel() * 8
                                                   for g in out))
                del out
            e["peak_bytes_above_inputs"] = peak
            r["batches"][str(b)] = e
            print(json.dumps({name: {str(b): e}}), flush=True)
            del S, St
        shapes[name] = r
        res["shapes"] = shapes
        write()
        if name in ("acm_like", "1M") and not args.no_model:
            kept[name] = gs
        else:
            del gs
        torch.cuda.empty_cache()

    if args.no_model:
        return

    # (b) a training step per batch: slice, forward, loss, backward
    def step_parts(gs, n, b, slicer):
        gen = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(n, 64, device=dev, generator=gen)
        y = torch.randint(0, 7, (n,), device=dev, generator=gen)
        torch.manual_seed(0)
        net = han.HANModel(3, 64, 8, 7, [8], 0.6).to(dev).train()
        perm = np.random.default_rng(7).permutation(n)
        batches = [torch.from_numpy(perm[i * b:(i + 1) * b].copy()).to(dev)
                   for i in range(max(1, min(8, n // b)))]
        state = {"i": 0, "slice_s": 0.0, "steps": 0}

        def step():
            idx = batches[state["i"] % len(batches)]
            state["i"] += 1
            sync()
            t0 = time.perf_counter()
            adjs = slicer(gs, idx)
            sync()
            state["slice_s"] += time.perf_counter() - t0
            state["steps"] += 1
            net.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(net(adjs, X[idx]), y[idx])
            loss.backward()
            return loss

        return step, state

    def where_the_rest_goes(step):
        """ms per step inside the per-graph builders the training path runs on a fresh batch
        graph, each timed inclusively between two synchronises (so the step itself is slower
        than the timed one), attributed to the outermost builder."""
        acc, depth = {}, [0]

        def wrap(owner, attr, label):
            fn = getattr(owner, attr)

            def timed(*a, **kw):
                if depth[0]:
                    return fn(*a, **kw)
                depth[0] += 1
                sync()
                t0 = time.perf_counter()
                try:
                    return fn(*a, **kw)
                finally:
                    sync()
                    acc[label] = acc.get(label, 0.0) + time.perf_counter() - t0
                    depth[0] -= 1
            setattr(owner, attr, timed)
            return owner, attr, fn

        saved = [wrap(graph, "_build_plan", "row_split_plans"),
                 wrap(CsrGraph, "task_plan", "task_plans"),
                 wrap(graph, "_build_hub_plan", "hub_plans"),
                 wrap(graph, "_build_xcd_hub_plan", "xcd_hub_plans"),
                 wrap(graph, "degree_order", "degree_order"),
                 wrap(CsrGraph, "transpose_eid", "transpose_with_edge_ids"),
                 wrap(CsrGraph, "transpose", "transpose")]
        try:
            steps = 4
            sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            sync()
            total = (time.perf_counter() - t0) * 1e3 / steps
        finally:
            for owner, attr, fn in saved:
                setattr(owner, attr, fn)
        out = {k_: v * 1e3 / steps for k_, v in acc.items()}
        out["instrumented_step_ms"] = total
        return out

    steps = {}
    if "1M" in kept:
        n = SHAPES["1M"][0]
        step, state = step_parts(kept["1M"], n, STEP_BATCH, hetero.induced_subgraphs)
        for _ in range(2):
            step()
        state.update(slice_s=0.0, steps=0)
        t = timed_blocks({"step": step}, args.seconds, 2, sync)
        s = {"what": "HANModel(3, 64, 8, 7, [8], 0.6).train(): induced_subgraphs, forward, "
                     f"cross-entropy and backward per batch of {STEP_BATCH} on the three 1M graphs",
             **summary(t["step"]), "slice_ms_mean": state["slice_s"] * 1e3 / state["steps"]}
        s["slice_share"] = s["slice_ms_mean"] / s["median_ms"]
        s["rest_of_the_step_ms"] = where_the_rest_goes(step)
        steps["1M_b8192"] = s
        print(json.dumps({"1M_b8192": s}), flush=True)
        del kept["1M"]
        torch.cuda.empty_cache()
    if "acm_like" in kept:
        gs = kept["acm_like"]
        n, b = SHAPES["acm_like"][0], 1024
        dense = []
        for g in gs:
            d = torch.zeros(n, n, device=dev)
            d[torch.repeat_interleave(torch.arange(n, device=dev), g.rowptr[1:] - g.rowptr[:-1]),
              g.col.to(torch.int64)] = 1
            dense.append(d)
        idx = batch(n, b)

        def csr_path():
            return hetero.induced_subgraphs(gs, idx)

        def dense_line():   # the reference's line on the device, then what HANModel makes of it
            return [from_dense(a[idx][:, idx], "positive") for a in dense]

        x, y = csr_path(), dense_line()
        same = all(torch.equal(p.rowptr, q.rowptr) and torch.equal(p.col, q.col)
                   for p, q in zip(x, y))
        t = timed_blocks({"induced_subgraphs": csr_path, "dense_slice_plus_from_dense": dense_line},
                         args.seconds, block_for(dense_line), sync)
        a = {"b": b, "equal": bool(same), **{k_: summary(v) for k_, v in t.items()}}
        a["dense_over_csr"] = (a["dense_slice_plus_from_dense"]["median_ms"]
                               / a["induced_subgraphs"]["median_ms"])
        for label, slicer, graphs in (("csr", hetero.induced_subgraphs, gs),
                                      ("dense", lambda ds, i: [d[i][:, i] for d in ds], dense)):
            step, state = step_parts(graphs, n, b, slicer)
            for _ in range(2):
                step()
            state.update(slice_s=0.0, steps=0)
            t = timed_blocks({"step": step}, args.seconds, 2, sync)
            a[f"step_{label}"] = {**summary(t["step"]),
                                  "slice_ms_mean": state["slice_s"] * 1e3 / state["steps"]}
        steps["acm_like_b1024"] = a
        print(json.dumps({"acm_like_b1024": a}), flush=True)
    res["training_step"] = steps
    write()


if __name__ == "__main__":
    main()
