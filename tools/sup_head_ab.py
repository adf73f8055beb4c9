"""The head of the supervised training steps (loss.supervised_loss / accuracy over
csrc/sup_head.hip, switch loss.SUPERVISED_HEAD_FUSED) against torch's path as the reference's
loops write it -- ``loss(output[idx_train], labels[idx_train])``,
``accuracy(output[idx_train], labels[idx_train])``, ``backward()`` -- measured in one process.

    python tools/sup_head_ab.py --cfg cfg2 --out profiles/sup_head_ab_cfg2.json

The protocol is tools/unsup_head_ab.py's: device events around blocks of calls, the sides
alternated, every side warmed first and given at least --seconds of timed work, median and
min-max of the block means. Needs a ROCm device: there is nothing to fall back to.

  a. head_alone: forward + backward of the head on random logits of the workload's shape
     (cfg2 / cfg3: N = 1M, C = 7, idx_train = arange(0, N, 10); cfg4: 8,192 rows, 3 classes, no
     index), torch against fused, once with the accuracy read per step on both sides and once
     without it on either; then each new kernel's call alone, with the bytes its arguments imply
     over its time as a share of 8 TB/s (bytes from the shapes, not measured HBM traffic).
  b. model_step: the whole training step with the switch off and on -- cfg2:
     GCN_Model(128, 128, 7, 2, 0.5) on the 1M / 10M RMAT graph; cfg3: GAT(64, 8, 7, 0.6, 0.2, 8)
     on the same graph; cfg4: the supervised GraphSAGE(2, 128, 128, MEAN, class_size=3) step on
     a device-sampled [25, 10] batch of 8,192 seeds of the 10M / 100M graph.
  c. agreement: the largest difference of the loss and of every parameter gradient between the
     sides over the largest magnitude on the off side (dropout off, so both sides see one
     forward).
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
    out = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
           "blocks": len(ms), "max_is_block": ms.index(max(ms))}
    if nbytes is not None:
        out["bytes_from_shapes"] = nbytes
        out["share_of_8TBps_from_shapes"] = nbytes / (out["median_ms"] * 1e-3) / HBM_BYTES_PER_S
    return out


def compare(t, off, on):
    """{side: summary} plus off / on and how the two block ranges lie."""
    out = {k: summary(v) for k, v in t.items()}
    a, b = out[off], out[on]
    out["off_over_on"] = a["median_ms"] / b["median_ms"]
    out["on_faster_outside_block_ranges"] = b["max_ms"] < a["min_ms"]
    out["ranges_overlap"] = not (b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"])
    return out


def ref_accuracy(y_hat, y):
    """GCN/train_eval.py:9-17, as the loops call it: one host read."""
    import torch
    if len(y_hat.shape) > 1 and y_hat.shape[1] > 1:
        y_hat = torch.argmax(y_hat, axis=1)
    cmp = y_hat.to(dtype=y.dtype) == y
    cmp = cmp.to(dtype=y.dtype)
    return float(cmp.sum()) / len(cmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", choices=("cfg2", "cfg3", "cfg4"), required=True)
    ap.add_argument("--small", action="store_true", help="a 100K-node graph (a rehearsal)")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side, at least")
    ap.add_argument("--block", type=int, default=200,
                    help="calls per timed block of the head-alone sides (a block of a few "
                         "calls is shorter than the host's own hiccups)")
    ap.add_argument("--head-only", action="store_true", help="skip the model steps")
    ap.add_argument("--rows", type=int, default=None,
                    help="with --head-only: another number of rows (the threshold sweep)")
    ap.add_argument("--classes", type=int, default=None, help="with --rows: the class count")
    ap.add_argument("--stride", type=int, default=None,
                    help="with --rows: idx_train = arange(0, rows, stride); 0: no index")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/sup_head_ab.py needs a ROCm device: no CPU path to time")
    from graphneuralnetwork_amd import _lib, ops
    from graphneuralnetwork_amd import loss as L
    from graphneuralnetwork_amd.rmat import rmat_edges
    from spmm_bf16_ab import alternate
    dev = torch.device("cuda:0")
    big = args.cfg == "cfg4"
    n, e = (10_000_000, 100_000_000) if big else (1_000_000, 10_000_000)
    if args.small:
        n, e = n // 10, e // 10
    N, C, stride = (8192, 3, 0) if big else (n, 7, 10)
    if args.rows is not None:
        if not args.head_only:
            raise SystemExit("--rows goes with --head-only")
        N = args.rows
        C = args.classes if args.classes is not None else C
        stride = args.stride if args.stride is not None else stride
    gen = torch.Generator(device=dev).manual_seed(0)
    z = (torch.randn(N, C, device=dev, generator=gen) * 2).requires_grad_()
    labels = torch.randint(0, C, (N,), device=dev, generator=gen)
    idx = torch.arange(0, N, stride, device=dev) if stride else None
    # the dispatcher's row threshold is what these numbers decide: both sides at every size
    res["default_min_rows"] = {"no_index": L.SUPERVISED_HEAD_MIN_ROWS,
                               "indexed": L.SUPERVISED_HEAD_MIN_ROWS_INDEXED}
    L.SUPERVISED_HEAD_MIN_ROWS = L.SUPERVISED_HEAD_MIN_ROWS_INDEXED = 0
    n_sel = N if idx is None else idx.numel()
    ce = torch.nn.CrossEntropyLoss()
    res.update({"workload": args.cfg + (" (small)" if args.small else ""), "nodes": n,
                "edges": e, "rows": N, "classes": C, "selected": n_sel,
                "index": "none" if idx is None else f"arange(0, N, {stride})",
                "switch": "loss.SUPERVISED_HEAD_FUSED",
                "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "timing": f"device events around blocks of calls ({args.block} per block for "
                          f"the head alone, 1 for the steps), sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})

    def sel(t):
        return t if idx is None else t[idx]

    # ---- a. the head alone
    def head_torch(acc):
        def fn():
            loss = ce(sel(z), sel(labels))
            a = ref_accuracy(sel(z), sel(labels)) if acc else None
            (g,) = torch.autograd.grad(loss, z)
            return loss, a, g
        return fn

    def head_fused(acc):
        def fn():
            if acc:
                loss, correct = L.supervised_loss(z, labels, idx, count_correct=True)
                a = float(correct) / n_sel
            else:
                loss, a = L.supervised_loss(z, labels, idx), None
            (g,) = torch.autograd.grad(loss, z)
            return loss, a, g
        return fn

    L.SUPERVISED_HEAD_FUSED = True
    zd = z.detach()
    count, status = (None, None) if idx is None else ops.sup_head_count(idx, N)
    _, _, inv_valid, status = ops.sup_head_forward(zd, labels, idx, status=status)
    up = torch.ones(1, device=dev)
    kernels = {"sup_head_forward": lambda: ops.sup_head_forward(zd, labels, idx),
               "sup_head_backward": lambda: ops.sup_head_backward(zd, labels, count, up,
                                                                  inv_valid, status)}
    nbytes = {"sup_head_forward": n_sel * (8 + C * 4) + (0 if idx is None else n_sel * 8),
              "sup_head_backward": (n_sel * (8 + C * 4) + (0 if idx is None else N * 4)
                                    + N * C * 4)}
    if idx is not None:
        kernels["sup_head_count"] = lambda: ops.sup_head_count(idx, N)
        nbytes["sup_head_count"] = n_sel * 8 + N * 4 + n_sel * 4
    sides = {"torch_head_with_accuracy": head_torch(True),
             "fused_head_with_accuracy": head_fused(True),
             "torch_head": head_torch(False), "fused_head": head_fused(False), **kernels}
    for fn in sides.values():  # one untimed block each: the allocator's pool at its final size
        for _ in range(args.block):
            fn()
    t = alternate(torch, sides, args.seconds, args.block)
    head = {k: summary(v, nbytes.get(k)) for k, v in t.items()}
    for tag in ("", "_with_accuracy"):
        a, b = head["torch_head" + tag], head["fused_head" + tag]
        head["torch_over_fused" + tag] = a["median_ms"] / b["median_ms"]
        head["fused_faster_outside_block_ranges" + tag] = b["max_ms"] < a["min_ms"]
    a_, b_ = head_torch(True)(), head_fused(True)()
    head["fused_vs_torch_max_abs_diff_over_max_abs"] = {
        "loss": float((b_[0] - a_[0]).detach().abs() / a_[0].detach().abs()),
        "dz": float((b_[2] - a_[2]).abs().max() / a_[2].abs().max())}
    head["accuracy_equal"] = a_[1] == b_[1]
    del a_, b_
    res["head_alone"] = head
    print(json.dumps({"head_alone": head}), flush=True)
    write()
    if args.head_only:
        return

    # ---- b. the whole step, switch off / on
    if args.cfg in ("cfg2", "cfg3"):
        from graphneuralnetwork_amd.preprocess import gcn_adjacency
        s, d = rmat_edges(n, e, 0)
        g = gcn_adjacency(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), n,
                          device=dev)
        del s, d
        torch.manual_seed(0)
        if args.cfg == "cfg2":
            from graphneuralnetwork_amd.gcn import GCN_Model
            make = lambda p: GCN_Model(128, 128, 7, 2, p).to(dev).train()  # noqa: E731
            what = "GCN_Model(128, 128, 7, 2, 0.5)"
            X = torch.randn(n, 128, device=dev, generator=gen)
        else:
            from graphneuralnetwork_amd.gat import GAT
            make = lambda p: GAT(64, 8, 7, dropout=p, alpha=0.2,  # noqa: E731
                                 nheads=8).to(dev).train()
            what = "GAT(64, 8, 7, dropout=0.6, alpha=0.2, nheads=8)"
            X = torch.randn(n, 64, device=dev, generator=gen)
        model = make(0.6 if args.cfg == "cfg3" else 0.5)
        forward = lambda m: m(X, g)  # noqa: E731
        y = labels
    else:
        from graphneuralnetwork_amd.graphsage import GraphSAGE
        from graphneuralnetwork_amd.sampler import (degree_ordered, sample_batch,
                                                    symmetric_adjacency)
        s, d = rmat_edges(n, e, 0)
        adj = symmetric_adjacency(s, d, n, device=dev)
        del s, d
        adj, _, _ = degree_ordered(adj)
        table = torch.randn(n, 128, device=dev, generator=gen)
        deg = adj.rowptr[1:] - adj.rowptr[:-1]
        cand = torch.nonzero(deg > 0).view(-1)
        seeds = cand[torch.randperm(cand.numel(), device=dev, generator=gen)[:8192]]
        batch = sample_batch(adj, seeds, (25, 10), seed=0)
        fargs = (*batch.forward_args(table), None, None, None, None, None)
        torch.manual_seed(0)
        make = lambda p: GraphSAGE(2, 128, 128, False, agg_func="MEAN",  # noqa: E731
                                   Unsupervised=False, class_size=3).to(dev).train()
        what = "GraphSAGE(2, 128, 128, MEAN, Unsupervised=False, class_size=3)"
        model = make(0.0)
        forward = lambda m: m(*fargs)[1]  # noqa: E731
        y = labels[:seeds.numel()]
    print("dataset built", flush=True)

    def step(m, fused, acc=False):
        def fn():
            L.SUPERVISED_HEAD_FUSED = fused
            m.zero_grad(set_to_none=True)
            out = forward(m)
            if fused:  # the loop with the drop-in lines
                if acc:
                    loss, correct = L.supervised_loss(out, y, idx, count_correct=True)
                    a = float(correct) / n_sel
                else:
                    loss, a = L.supervised_loss(out, y, idx), None
            else:      # the loop as the reference writes it
                loss = ce(sel(out), sel(y))
                a = ref_accuracy(sel(out), sel(y)) if acc else None
            loss.backward()
            return loss, a
        return fn

    t = alternate(torch, {"off": step(model, False), "on": step(model, True)}, args.seconds, 1)
    res["model_step"] = {"what": what + ".train(): forward, loss on the selection, backward",
                         **compare(t, "off", "on")}
    t = alternate(torch, {"off": step(model, False, True), "on": step(model, True, True)},
                  args.seconds, 1)
    res["model_step_with_accuracy"] = compare(t, "off", "on")
    print(json.dumps({k: res[k] for k in ("model_step", "model_step_with_accuracy")}),
          flush=True)
    write()

    # ---- c. the same numbers? one step per side of the same model without dropout
    del model
    model = make(0.0)
    got = {}
    for fused in (False, True):
        loss, _ = step(model, fused)()
        got[fused] = {"loss": loss.detach(), **{k: p.grad.clone()
                                                for k, p in model.named_parameters()
                                                if p.grad is not None}}
    res["agreement_on_vs_off_max_abs_diff_over_max_abs"] = {
        k: float((got[True][k] - v).abs().max() / v.abs().max()) for k, v in got[False].items()}
    L.SUPERVISED_HEAD_FUSED = True
    print(json.dumps({"agreement": res["agreement_on_vs_off_max_abs_diff_over_max_abs"]}),
          flush=True)
    write()


if __name__ == "__main__":
    main()
