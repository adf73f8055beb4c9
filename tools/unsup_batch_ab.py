"""Unsupervised GraphSAGE batches on the cfg4 dataset: what the device contexts / negatives and
the second tower cost, measured in one process.

    python tools/unsup_batch_ab.py [--small] [--merge old.json] --out profiles/unsup_batch_cfg4.json
    python tools/unsup_batch_ab.py --host-reference DIR [--merge old.json] --out ...   (no GPU)

Builds the cfg4 workload as bench.py does (R-MAT 10M nodes / 100M edges, symmetric adjacency
relabelled by degree, a 10M x 128 table; --small: 1M / 10M for a quick look) and times, with
device events around blocks of calls, every side at least --seconds of timed work, median and
min-max of the block means:

  * dataset scale: ``gnn_sample_contexts`` + ``gnn_sample_negatives`` for every node, window 5,
    K 5 (the reference's precomputation before training), with the fraction of the 8 TB/s
    roofline on the bytes written, n * (window + need) * 8. Nodes without neighbours keep
    their row of -1 (the error word is not read here);
  * one batch of 8192 seeds, fanouts [25, 10]: ``sample_unsupervised_batch(sync=False)`` from
    the precomputed rows (negatives over the nodes that have neighbours: with the degree
    order those are the ids below a bound, so a negative is never an isolated node) and drawn
    per batch; the inference forward on an fp32 and a bf16 table; beside them the supervised
    ``sample_batch(sync=False)`` + forward on the same seeds, so the second tower's cost shows.

``--host-reference DIR`` (a checkout of the reference; CPU only): the reference's own
get_context_nodes / get_negative_nodes (DIR/GraphSAGE/data_utils.py) timed over 100,000
random nodes of the same edge list (relabelling aside) and scaled to all nodes -- an
extrapolation, one interpreter thread.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak, the roofline bench.py uses
WINDOW, K = 5, 5


def summary(ms, nbytes=None):
    m = statistics.median(ms)
    out = {"median_ms": m, "min_ms": min(ms), "max_ms": max(ms), "blocks": len(ms)}
    if nbytes is not None:
        out["bytes_written"] = nbytes
        out["hbm_fraction"] = nbytes / (m * 1e-3) / HBM_BYTES_PER_S
    return out


def host_reference(ref_dir, n, e, slice_nodes):
    """The reference's two functions on `slice_nodes` random nodes that have neighbours."""
    import random
    from collections import defaultdict

    import numpy as np
    from graphneuralnetwork_amd.rmat import rmat_edges
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(Path(ref_dir) / "GraphSAGE"))
    import data_utils as du  # the reference's GraphSAGE/data_utils.py
    s, d = rmat_edges(n, e, 0)
    keep = s != d
    s, d = s[keep], d[keep]
    has = np.zeros(n, bool)
    has[s] = True
    has[d] = True
    cand = np.nonzero(has)[0]
    nodes = np.random.default_rng(0).choice(cand, min(slice_nodes, cand.size), replace=False)
    mark = np.zeros(n, bool)
    mark[nodes] = True
    adj = defaultdict(set)
    for a, b in ((s, d), (d, s)):
        m = mark[a]
        for u, v in zip(a[m].tolist(), b[m].tolist()):
            adj[u].add(v)
    nodes = nodes.tolist()
    universe = list(range(n))
    random.seed(0)
    t0 = time.perf_counter()
    ctx = du.get_context_nodes(nodes, adj, WINDOW)
    t1 = time.perf_counter()
    du.get_negative_nodes(ctx, universe, K)
    t2 = time.perf_counter()
    scale = n / len(nodes)
    return {"slice_nodes": len(nodes), "nodes_with_neighbours": int(cand.size),
            "contexts_s": t1 - t0, "negatives_s": t2 - t1,
            "scaled_to_all_nodes_s": (t2 - t0) * scale,
            "note": "the reference's own get_context_nodes / get_negative_nodes in CPython on "
                    "one interpreter thread; the all-nodes figure is slice time x n / slice "
                    "(an extrapolation)",
            "host_cpus": len(os.sched_getaffinity(0)), "python": sys.version.split()[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1M nodes / 10M edges (not cfg4)")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side, at least")
    ap.add_argument("--host-reference", default=None, metavar="DIR")
    ap.add_argument("--host-slice", type=int, default=100_000)
    ap.add_argument("--merge", default=None, help="start from this JSON (the other mode's keys)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    n, e = (1_000_000, 10_000_000) if args.small else (10_000_000, 100_000_000)
    res = json.loads(Path(args.merge).read_text()) if args.merge else {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    if args.host_reference:
        res["host_reference"] = host_reference(args.host_reference, n, e, args.host_slice)
        print(json.dumps(res["host_reference"]), flush=True)
        write()
        return

    import torch
    from graphneuralnetwork_amd import _lib
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
    assert bool((deg[:n_conn] > 0).all())  # degree order: the nodes with neighbours come first
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(n, F, device=dev, generator=gen)
    table16 = table.bfloat16()
    need = WINDOW * K
    res.update({"workload": "cfg4" if not args.small else "small", "nodes": n, "edges": e,
                "feat": F, "window": WINDOW, "K": K, "fanout": list(fanouts),
                "nodes_with_neighbours": n_conn, "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "timing": f"device events around blocks of calls, sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})

    # ---- dataset scale: every node, one call each
    all_nodes = torch.arange(n, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx_all = S._contexts_into(adj, all_nodes, WINDOW, 0, err)
    t = alternate(torch, {
        "contexts": lambda: S._contexts_into(adj, all_nodes, WINDOW, 0, err),
        "negatives": lambda: S._negatives_into(ctx_all, n, K, 0, err)}, args.seconds, 4)
    ds = {"contexts": summary(t["contexts"], n * WINDOW * 8),
          "negatives": summary(t["negatives"], n * need * 8)}
    tot = ds["contexts"]["median_ms"] + ds["negatives"]["median_ms"]
    ds["both_median_ms"] = tot
    ds["both_hbm_fraction"] = n * (WINDOW + need) * 8 / (tot * 1e-3) / HBM_BYTES_PER_S
    ds["error_word"] = int(err.item())  # 1: the nodes without neighbours (rows of -1)
    res["dataset_scale_all_nodes"] = ds
    print(json.dumps({"dataset_scale_all_nodes": ds}), flush=True)
    del ctx_all
    # the dataset the batches below read: the nodes with neighbours, negatives among them
    conn = all_nodes[:n_conn]
    ctx_ds = S.sample_contexts(adj, conn, WINDOW, seed=0)
    neg_ds = S.sample_negatives(ctx_ds, n_conn, K, seed=0)

    # ---- one batch
    B = args.seeds
    seeds = torch.randperm(n_conn, device=dev, generator=gen)[:B]
    ctx_b, neg_b = ctx_ds[seeds].contiguous(), neg_ds[seeds].contiguous()

    def unsup(**kw):
        return S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, sync=False, **kw)
    probe = unsup(contexts=ctx_b, negatives=neg_b)
    second_tower_buffer = int(probe.context.frontier.untyped_storage().nbytes())
    synced = probe.sync()  # raises on any sampler error: the precomputed rows have none
    sizes = {"centre_tower_layers": list(synced.center.layer_sizes),
             "second_tower_layers": list(synced.context.layer_sizes),
             "second_tower_seeds": int(synced.context.seeds.numel()),
             "second_tower_buffer_bytes": second_tower_buffer}
    # drawn per batch over all n ids, as the reference's universe is: a negative may then be a
    # node without neighbours, which the second tower refuses (the reference's collate_fn
    # raises the same IndexError); recorded, since that batch's timing is of its error path
    try:
        unsup().check()
        sizes["drawn_over_all_ids_check"] = "ok"
    except IndexError as ex:
        sizes["drawn_over_all_ids_check"] = f"IndexError: {ex}"
    err_b = torch.zeros(1, dtype=torch.int32, device=dev)

    def drawn_connected():  # this batch's own draws, negatives among the nodes with neighbours
        c = S._contexts_into(adj, seeds, WINDOW, 1, err_b)
        return unsup(contexts=c, negatives=S._negatives_into(c, n_conn, K, 1, err_b))
    drawn_connected().check()
    sizes["drawn_connected_error_word"] = int(err_b.item())
    del probe, synced
    res["batch"] = {"seeds": B, **sizes}
    t = alternate(torch, {
        "unsup_precomputed_rows": lambda: unsup(contexts=ctx_b, negatives=neg_b),
        "unsup_drawn_per_batch_connected_universe": drawn_connected,
        "unsup_drawn_per_batch_all_ids": lambda: unsup(),
        "supervised": lambda: S.sample_batch(adj, seeds, fanouts, seed=1, sync=False)},
        args.seconds, 10)
    res["batch"]["sampling_pending"] = {k: summary(v) for k, v in t.items()}
    print(json.dumps({"sampling_pending": res["batch"]["sampling_pending"]}), flush=True)

    torch.manual_seed(0)
    net_u = GraphSAGE(2, F, H, False, agg_func="MEAN", Unsupervised=True).to(dev).eval()
    net_s = GraphSAGE(2, F, H, False, agg_func="MEAN", Unsupervised=False,
                      class_size=3).to(dev).eval()
    pu = unsup(contexts=ctx_b, negatives=neg_b)
    ps = S.sample_batch(adj, seeds, fanouts, seed=1, sync=False)

    def fwd_u(tab):
        a = pu.forward_args(tab)

        def fn():
            with torch.no_grad():
                net_u(*a)
        return fn

    def fwd_s(tab):
        a = ps.forward_args(tab)

        def fn():
            with torch.no_grad():
                net_s(*a, None, None, None, None, None)
        return fn
    t = alternate(torch, {"unsup_fp32": fwd_u(table), "unsup_bf16": fwd_u(table16),
                          "supervised_fp32": fwd_s(table), "supervised_bf16": fwd_s(table16)},
                  args.seconds, 5)
    res["batch"]["inference_forward_pending"] = {k: summary(v) for k, v in t.items()}
    print(json.dumps({"inference_forward": res["batch"]["inference_forward_pending"]}), flush=True)

    def step_u():
        b = unsup(contexts=ctx_b, negatives=neg_b)
        with torch.no_grad():
            net_u(*b.forward_args(table))

    def step_s():
        b = S.sample_batch(adj, seeds, fanouts, seed=1, sync=False)
        with torch.no_grad():
            net_s(*b.forward_args(table), None, None, None, None, None)
    t = alternate(torch, {"unsup_fp32": step_u, "supervised_fp32": step_s}, args.seconds, 5)
    res["batch"]["sample_plus_forward_pending"] = {k: summary(v) for k, v in t.items()}
    print(json.dumps({"sample_plus_forward": res["batch"]["sample_plus_forward_pending"]}),
          flush=True)
    pu.check()
    ps.check()
    write()


if __name__ == "__main__":
    main()
