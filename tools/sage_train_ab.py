"""The GraphSAGE training step on the cfg4 dataset with and without the training layer
(graphsage._SageTrainLayerFn), measured in one process.

    python tools/sage_train_ab.py [--small] --out profiles/sage_train_ab_cfg4.json

Builds the cfg4 workload as bench.py does (R-MAT 10M nodes / 100M edges, symmetric adjacency
relabelled by degree, a 10M x 128 table; --small: 1M / 10M for a quick look), samples one batch
of 8192 seeds with fanouts [25, 10] and times, with device events around blocks of calls, every
side at least --seconds of timed work, median and min-max of the block means:

  * the training step -- forward, loss, backward; the weights require grad, the table does not
    -- (a) supervised with cross-entropy, (b) unsupervised with window 5, K 5 and
    binary_cross_entropy_with_logits, each with graphsage.SAGE_TRAIN_FUSED off (the separate
    gathers, torch's linear + addmm + relu and a CSR rebuilt in Python per backward gather) and
    on, over an fp32 and a bf16 table, the four sides alternated;
  * the two new launches alone at the second tower's layer-1 shape (its 245,760 seeds, k = 25,
    over the ~1M-row frontier): ``sage_maps_transpose`` and ``sage_scatter_concat``, the
    scatter's gathered bytes M (k + 1) F 4 over its time as a share of the 8 TB/s roofline,
    and beside them what they replace: the two ``_scatter_rows`` calls and the sum of their
    results (autograd's accumulation of the two gradients of one table).

--agg MAXPOOL: the same protocol for the max-pool layer (graphsage._SageMaxPoolTrainLayerFn,
switch graphsage.SAGE_TRAIN_FUSED_MAXPOOL; off: the row gather, the argmax and value launches of
_GatherMaxPoolAgg and its index_put_ backward). The two new ops alone, at the same layer-1 shape
over a random fp32 table: ``sage_gather_concat_arg`` against the three launches it replaces, and
``sage_scatter_concat_maxpool`` against the backward it replaces (the index_put_ of the aggregate
half with its zero table, row-id and column tensors, the centre rows' ``_scatter_rows``, and
their sum), plus the bytes each side keeps for the backward (uint8 against int64 winners).

--gcn: the gcn-mode layers (GraphSAGE(.., gcn=True): relu(W . agg), the sampler's maps of width
fanout + 1; graphsage._SageGcnTrainLayerFn / _fused_gcn_layer, switch graphsage.SAGE_GCN_FUSED)
by the same protocol, MEAN and MAXPOOL in one process (--agg is not read): the supervised and
the unsupervised training step, and the inference forward on a PENDING batch (sample_batch(...,
sync=False): with the switch off the forward reads the frontier size back, with it on it does
not), each over an fp32 and a bf16 table with the switch off and on, the four sides alternated.
Per aggregator it also counts the layer-0 outputs whose ReLU passes on one side only (the two
sides' GEMMs round differently) and compares the new adjoint alone with the path it replaces at
the second tower's layer-1 shape.

    python tools/sage_train_ab.py --gcn --out profiles/sage_gcn_ab_cfg4.json

Each comparison also records that both sides compute the same numbers at this size: the largest
difference of every weight gradient (one step per side) and of the scatter's output, over the
largest magnitude of the previous path's.
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
WINDOW, K = 5, 5


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "blocks": len(ms)}


def compare(t):
    """{side: summary} plus, per table dtype, off / on and whether the block ranges are apart."""
    out = {k: summary(v) for k, v in t.items()}
    for dt in ("fp32", "bf16"):
        off, on = out[f"{dt}_off"], out[f"{dt}_on"]
        out[f"{dt}_off_over_on"] = off["median_ms"] / on["median_ms"]
        out[f"{dt}_on_faster_outside_block_ranges"] = on["max_ms"] < off["min_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1M nodes / 10M edges (not cfg4)")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side, at least")
    ap.add_argument("--agg", choices=("MEAN", "MAXPOOL"), default="MEAN")
    ap.add_argument("--gcn", action="store_true",
                    help="the gcn-mode layers (graphsage.SAGE_GCN_FUSED), MEAN and MAXPOOL")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    n, e = (1_000_000, 10_000_000) if args.small else (10_000_000, 100_000_000)
    res = {}
    switch = "SAGE_TRAIN_FUSED" if args.agg == "MEAN" else "SAGE_TRAIN_FUSED_MAXPOOL"

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    import torch.nn.functional as Fn
    from graphneuralnetwork_amd import _lib, graphsage, ops
    from graphneuralnetwork_amd import sampler as S
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    from graphneuralnetwork_amd.rmat import rmat_edges
    from spmm_bf16_ab import alternate
    dev = torch.device("cuda:0")
    F = H = args.feat
    fanouts = (25, 10)
    s, d = rmat_edges(n, e, 0)
    adj = S.symmetric_adjacency(s, d, n, device=dev)
    del s, d
    adj, _, _ = S.degree_ordered(adj)
    deg = adj.rowptr[1:] - adj.rowptr[:-1]
    n_conn = int((deg > 0).sum())
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(n, F, device=dev, generator=gen)
    table16 = table.bfloat16()
    print("dataset built", flush=True)
    B = args.seeds
    seeds = torch.randperm(n_conn, device=dev, generator=gen)[:B]
    ctx_b = S.sample_contexts(adj, seeds, WINDOW, seed=0)
    neg_b = S.sample_negatives(ctx_b, n_conn, K, seed=0)  # among the nodes with neighbours
    if args.gcn:
        return gcn_ab(args, res, write, adj, seeds, ctx_b, neg_b, table, table16, gen)
    pu = S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, contexts=ctx_b,
                                     negatives=neg_b)
    ps = S.sample_batch(adj, seeds, fanouts, seed=1)
    if args.agg != "MEAN":
        res.update({"agg": args.agg, "switch": f"graphsage.{switch}"})
    res.update({"workload": "cfg4" if not args.small else "small", "nodes": n, "edges": e,
                "feat": F, "hidden": H, "seeds": B, "window": WINDOW, "K": K,
                "fanout": list(fanouts), "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "centre_tower_layers": list(pu.center.layer_sizes),
                "second_tower_layers": list(pu.context.layer_sizes),
                "timing": f"device events around blocks of calls, sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})

    torch.manual_seed(0)
    net_u = GraphSAGE(2, F, H, False, agg_func=args.agg, Unsupervised=True).to(dev).train()
    net_s = GraphSAGE(2, F, H, False, agg_func=args.agg, Unsupervised=False,
                      class_size=3).to(dev).train()
    y_s = torch.randint(0, 3, (B,), device=dev, generator=gen)
    y_u = pu.labels.to(torch.float32)

    def step_s(tab, fused):
        a = ps.forward_args(tab)

        def fn():
            setattr(graphsage, switch, fused)
            net_s.zero_grad(set_to_none=True)
            _, logits = net_s(*a, None, None, None, None, None)
            Fn.cross_entropy(logits, y_s).backward()
        return fn

    def step_u(tab, fused):
        a = pu.forward_args(tab)

        def fn():
            setattr(graphsage, switch, fused)
            net_u.zero_grad(set_to_none=True)
            _, score = net_u(*a)
            Fn.binary_cross_entropy_with_logits(score.squeeze(1), y_u).backward()
        return fn

    for name, step, iters in (("supervised_step", step_s, 4), ("unsupervised_step", step_u, 1)):
        t = alternate(torch, {"fp32_off": step(table, False), "fp32_on": step(table, True),
                              "bf16_off": step(table16, False), "bf16_on": step(table16, True)},
                      args.seconds, iters)
        res[name] = compare(t)
        # the same numbers? one step per side on the fp32 table, every weight gradient
        net = net_s if step is step_s else net_u
        grads = {}
        for fused in (False, True):
            step(table, fused)()
            grads[fused] = {k_: p.grad.clone() for k_, p in net.named_parameters()}
        res[name]["grad_max_abs_diff_over_max_abs"] = {
            k_: float((grads[True][k_] - g).abs().max() / g.abs().max())
            for k_, g in grads[False].items()}
        if args.agg == "MAXPOOL" and step is step_s:
            # the two sides run layer 0's GEMM on different kernels, and a maximum is not
            # continuous: how many layer-1 winners land on another row because of that
            with torch.no_grad():
                W0 = net_s.sage_blocks.sage_layer0.weight.weight
                buf, _ = ops.sage_gather_concat_arg(table, ps.frontier, ps.frontier_nbrs,
                                                    check=False)
                h_on = ops.gcn_transform(buf, W0, relu=True)
                h_off = torch.relu(torch.addmm(Fn.linear(buf[:, :F], W0[:, :F]), buf[:, F:],
                                               W0[:, F:].t()))
                nm = ps.neigh_maps[-1]
                r_on = nm.gather(1, ops.sage_gather_aggregate(h_on, nm, "MAX", check=False))
                r_off = nm.gather(1, ops.sage_gather_aggregate(h_off, nm, "MAX", check=False))
                top = ops.sage_gather_aggregate(h_off, nm, "MAXPOOL", check=False)
                res[name]["layer1_winners"] = {
                    "entries": r_on.numel(),
                    "on_another_row_with_a_positive_maximum":
                        int(((r_on != r_off) & (top > 0)).sum()),
                    "layer0_output_max_abs_diff": float((h_on - h_off).abs().max()),
                    "layer0_output_max_abs": float(h_off.abs().max())}
                del buf, h_on, h_off, r_on, r_off, top
        print(json.dumps({name: res[name]}), flush=True)
        write()
    setattr(graphsage, switch, True)

    # ---- the two new launches alone, at the second tower's layer-1 shape
    tower = pu.context
    cidx, idx = tower.center_maps[-1], tower.neigh_maps[-1]
    n_prev = int(tower.layers[1].numel())
    M, k = idx.shape
    dbuf = torch.randn(M, 2 * F, device=dev, generator=gen)
    tr = ops.sage_maps_transpose(cidx, idx, n_prev)
    lens = tr.ptr[1:] - tr.ptr[:-1]
    gathered = M * (k + 1) * F * 4
    if args.agg == "MAXPOOL":
        h = torch.randn(n_prev, F, device=dev, generator=gen)  # layer 0's output stands in

        def fwd_parent():
            c = ops.gather_rows(h, cidx, check=False)
            a = ops.sage_gather_aggregate(h, idx, "MAX", check=False)
            return c, a, ops.sage_gather_aggregate(h, idx, "MAXPOOL", check=False)

        def bwd_parent():  # _GatherMaxPoolAgg.backward + _GatherRows.backward + their sum
            rows = idx.gather(1, arg64)
            cols = torch.arange(F, device=dev).expand_as(rows)
            out = torch.zeros((n_prev, F), device=dev)
            out.index_put_((rows, cols), dbuf[:, F:], accumulate=True)
            return out + graphsage._scatter_rows(dbuf[:, :F], cidx.reshape(-1, 1), n_prev, 1.0)
        buf, arg = ops.sage_gather_concat_arg(h, cidx, idx, check=False)
        c_, arg64, v_ = fwd_parent()
        fwd_same = bool(torch.equal(buf[:, :F], c_) and torch.equal(buf[:, F:], v_)
                        and torch.equal(arg.to(torch.int64), arg64))
        old, new = bwd_parent(), ops.sage_scatter_concat_maxpool(dbuf, arg, tr, n_prev)
        agree = float((new - old).abs().max() / old.abs().max())
        again = ops.sage_scatter_concat_maxpool(dbuf, arg, tr, n_prev)
        rerun = {"sage_scatter_concat_maxpool": bool(torch.equal(new, again)),
                 "parent_index_put": bool(torch.equal(old, bwd_parent()))}
        del old, new, again, c_, v_, buf
        t = alternate(torch, {
            "sage_gather_concat_arg": lambda: ops.sage_gather_concat_arg(h, cidx, idx, check=False),
            "parent_gather_argmax_maxpool": fwd_parent,
            "sage_scatter_concat_maxpool":
                lambda: ops.sage_scatter_concat_maxpool(dbuf, arg, tr, n_prev),
            "parent_index_put_backward": bwd_parent}, args.seconds, 4)
        kern = {k_: summary(v) for k_, v in t.items()}
        sc = kern["sage_scatter_concat_maxpool"]
        sc["bytes_gathered"] = gathered + M * (k + 1) * F  # the gradient rows and their winners
        sc["hbm_fraction"] = sc["bytes_gathered"] / (sc["median_ms"] * 1e-3) / HBM_BYTES_PER_S
        res["second_tower_layer1"] = {
            "M": M, "k": k, "n_prev": n_prev, "slots": M * (k + 1),
            "longest_list": int(lens.max()), "lists_split_into_chunks": int((lens > 256).sum()),
            "forward_bit_identical_to_parent_launches": fwd_same,
            "scatter_vs_parent_max_abs_diff_over_max_abs": agree,
            "bit_identical_on_rerun": rerun,
            "saved_winner_bytes": {"uint8_arg": M * F, "parent_int64_argmax": M * F * 8},
            **kern}
        l0 = int(tower.layers[-1].numel())  # the second tower's layer-0 rows
        res["second_tower_layer0_saved_winner_bytes"] = {
            "M": l0, "uint8_arg": l0 * F, "parent_int64_argmax": l0 * F * 8,
            "note": "from the shape; only a table that requires grad saves it in the parent"}
        print(json.dumps({"second_tower_layer1": res["second_tower_layer1"]}), flush=True)
        write()
        return

    def parent():
        return (graphsage._scatter_rows(dbuf[:, :F], cidx.reshape(-1, 1), n_prev, 1.0)
                + graphsage._scatter_rows(dbuf[:, F:], idx, n_prev, 1.0 / k))
    old, new = parent(), ops.sage_scatter_concat(dbuf, tr, n_prev)
    agree = float((new - old).abs().max() / old.abs().max())
    del old, new
    t = alternate(torch, {
        "sage_maps_transpose": lambda: ops.sage_maps_transpose(cidx, idx, n_prev, check=False),
        "sage_scatter_concat": lambda: ops.sage_scatter_concat(dbuf, tr, n_prev),
        "parent_two_scatter_rows": parent}, args.seconds, 4)
    kern = {k_: summary(v) for k_, v in t.items()}
    sc = kern["sage_scatter_concat"]
    sc["bytes_gathered"] = gathered
    sc["hbm_fraction"] = gathered / (sc["median_ms"] * 1e-3) / HBM_BYTES_PER_S
    res["second_tower_layer1"] = {
        "M": M, "k": k, "n_prev": n_prev, "slots": M * (k + 1),
        "longest_list": int(lens.max()), "median_list": float(lens.float().median()),
        "lists_split_into_chunks": int((lens > 256).sum()),
        "scatter_vs_parent_max_abs_diff_over_max_abs": agree, **kern}
    print(json.dumps({"second_tower_layer1": res["second_tower_layer1"]}), flush=True)
    write()


def gcn_ab(args, res, write, adj, seeds, ctx_b, neg_b, table, table16, gen):
    """--gcn: graphsage.SAGE_GCN_FUSED off / on, both aggregators, on the dataset main() built."""
    import torch
    import torch.nn.functional as Fn
    from graphneuralnetwork_amd import _lib, graphsage, ops
    from graphneuralnetwork_amd import sampler as S
    from graphneuralnetwork_amd.graphsage import GraphSAGE
    from spmm_bf16_ab import alternate
    dev = table.device
    F = H = args.feat
    B, fanouts = args.seeds, (25, 10)
    pu = S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, contexts=ctx_b,
                                     negatives=neg_b, gcn=True)
    ps = S.sample_batch(adj, seeds, fanouts, seed=1, gcn=True)
    # the same batches with their sizes left on the device (the inference forward's input)
    qu = S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, contexts=ctx_b,
                                     negatives=neg_b, gcn=True, sync=False)
    qs = S.sample_batch(adj, seeds, fanouts, seed=1, gcn=True, sync=False)
    res.update({"gcn": True, "switch": "graphsage.SAGE_GCN_FUSED",
                "workload": "cfg4" if not args.small else "small",
                "nodes": adj.n_rows, "edges": 10_000_000 if args.small else 100_000_000, "feat": F, "hidden": H, "seeds": B, "window": WINDOW, "K": K,
                "fanout": list(fanouts), "map_widths": [k + 1 for k in fanouts],
                "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "centre_tower_layers": list(pu.center.layer_sizes),
                "second_tower_layers": list(pu.context.layer_sizes),
                "timing": f"device events around blocks of calls, sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})
    y_s = torch.randint(0, 3, (B,), device=dev, generator=gen)
    y_u = pu.labels.to(torch.float32)
    for agg in ("MEAN", "MAXPOOL"):
        torch.manual_seed(0)
        net_u = GraphSAGE(2, F, H, True, agg_func=agg, Unsupervised=True).to(dev)
        net_s = GraphSAGE(2, F, H, True, agg_func=agg, Unsupervised=False, class_size=3).to(dev)

        def step(net, batch, tab, fused):
            a = batch.forward_args(tab)
            a = a if net.Unsupervised else (*a, None, None, None, None, None)

            def fn():
                graphsage.SAGE_GCN_FUSED = fused
                net.zero_grad(set_to_none=True)
                _, second = net(*a)
                if net.Unsupervised:
                    Fn.binary_cross_entropy_with_logits(second.squeeze(1), y_u).backward()
                else:
                    Fn.cross_entropy(second, y_s).backward()
            return fn

        def infer(net, batch, tab, fused):
            a = batch.forward_args(tab)
            a = a if net.Unsupervised else (*a, None, None, None, None, None)

            def fn():
                graphsage.SAGE_GCN_FUSED = fused
                with torch.no_grad():
                    return net(*a)
            return fn

        out = res[agg] = {}
        for name, make, net, batch, iters in (
                ("supervised_step", step, net_s, ps, 4), ("unsupervised_step", step, net_u, pu, 1),
                ("supervised_pending_inference", infer, net_s, qs, 4),
                ("unsupervised_pending_inference", infer, net_u, qu, 1)):
            net.train(make is step)
            t = alternate(torch, {"fp32_off": make(net, batch, table, False),
                                  "fp32_on": make(net, batch, table, True),
                                  "bf16_off": make(net, batch, table16, False),
                                  "bf16_on": make(net, batch, table16, True)},
                          args.seconds, iters)
            out[name] = compare(t)
            # the same numbers? one call per side on the fp32 table
            if make is step:
                grads = {}
                for fused in (False, True):
                    make(net, batch, table, fused)()
                    grads[fused] = {k_: p.grad.clone() for k_, p in net.named_parameters()}
                out[name]["grad_max_abs_diff_over_max_abs"] = {
                    k_: float((grads[True][k_] - g).abs().max() / g.abs().max())
                    for k_, g in grads[False].items()}
            else:
                off, on = (make(net, batch, table, fused)() for fused in (False, True))
                out[name]["output_max_abs_diff_over_max_abs"] = [
                    float((a_ - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(on, off)]
            print(json.dumps({agg: {name: out[name]}}), flush=True)
            write()
        # what stands behind a gradient difference above rounding: the two sides run layer 0's
        # GEMM on different kernels and a ReLU is not continuous, so an element whose
        # pre-activation is within rounding of zero passes its gradient on one side only
        with torch.no_grad():
            flips = {}
            for name, net, b in (("supervised", net_s, ps), ("unsupervised_centre", net_u, pu.center),
                                 ("unsupervised_second", net_u, pu.context)):
                W0 = net.sage_blocks.sage_layer0.weight.weight
                buf = ops.sage_gather_aggregate(table, b.frontier_nbrs, agg, check=False)
                h_on = ops.gcn_transform(buf, W0, relu=True)
                h_off = torch.relu(Fn.linear(buf, W0))
                flips[name] = {"elements": h_on.numel(),
                               "passing_on_one_side_only": int(((h_on > 0) != (h_off > 0)).sum()),
                               "max_abs_diff": float((h_on - h_off).abs().max()),
                               "max_abs": float(h_off.abs().max())}
                del buf, h_on, h_off
            out["layer0_relu_mask"] = flips
            # the adjoint alone at the second tower's layer-1 shape, against the path it replaces
            tower = pu.context
            idx = tower.neigh_maps[-1]
            n_prev = int(tower.layers[1].numel())
            M, k = idx.shape
            dbuf = torch.randn(M, F, device=dev, generator=gen)
            tr = ops.sage_maps_transpose_nbr(idx, n_prev)
            lens = tr.ptr[1:] - tr.ptr[:-1]
            if agg == "MEAN":
                old = graphsage._scatter_rows(dbuf, idx, n_prev, 1.0 / k)
                new = ops.sage_scatter_agg(dbuf, tr, n_prev)
                again = ops.sage_scatter_agg(dbuf, tr, n_prev)
            else:
                h = torch.randn(n_prev, F, device=dev, generator=gen)  # layer 0's output stands in
                _, arg = ops.sage_gather_aggregate_arg(h, idx, check=False)
                old = graphsage._gcn_maxpool_scatter_torch(dbuf, arg, idx, n_prev)
                new = ops.sage_scatter_agg_maxpool(dbuf, arg, tr, n_prev)
                again = ops.sage_scatter_agg_maxpool(dbuf, arg, tr, n_prev)
            out["second_tower_layer1_scatter"] = {
                "M": M, "k": k, "n_prev": n_prev, "slots": M * k,
                "longest_list": int(lens.max()),
                "lists_split_into_chunks": int((lens > 256).sum()),
                "vs_parent_max_abs_diff_over_max_abs":
                    float((new - old).abs().max() / old.abs().max()),
                "bit_identical_on_rerun": bool(torch.equal(new, again))}
            del old, new, again, dbuf, tr
        print(json.dumps({agg: {k_: out[k_] for k_ in ("layer0_relu_mask",
                                                       "second_tower_layer1_scatter")}}), flush=True)
        write()
    graphsage.SAGE_GCN_FUSED = True


if __name__ == "__main__":
    main()
