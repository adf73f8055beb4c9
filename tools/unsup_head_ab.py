"""The head of the unsupervised GraphSAGE step (graphsage._SageScoreFn + unsupervised_loss over
csrc/sage_score.hip, switch graphsage.SAGE_SCORE_FUSED) against torch's bmm +
binary_cross_entropy_with_logits on the cfg4 dataset, measured in one process, and where the
step's time goes.

    python tools/unsup_head_ab.py [--small] --out profiles/unsup_head_ab_cfg4.json

The dataset, the batch (8192 seeds, fanouts [25, 10], window 5, K 5: B = 8192, S = 30, H = 128)
and the protocol are tools/sage_train_ab.py's: device events around blocks of calls, the sides
alternated, every side warmed first and given at least --seconds of timed work, median and
min-max of the block means. Needs a ROCm device: there is nothing to fall back to.

  a. head_alone: forward + backward of the head on the second tower's real embeddings, torch
     (bmm, the loss, autograd down to contiguous d_center / d_second) against the fused head,
     and each of the three kernels' calls alone with the bytes its arguments imply over its time
     as a share of 8 TB/s (bytes from the shapes, not measured HBM traffic).
  b. unsupervised_step / unsupervised_pending_inference: the training step and the inference
     forward on a pending batch with the switch off (the previous path: bmm and torch's loss) and
     on (with unsupervised_loss), over an fp32 and a bf16 table, the four sides alternated.
  c. phases: device-event time of each phase of one step (sampling, the host read that trims
     the pending batch, the two towers forward, the head forward with the loss, the head
     backward, the two towers backward), switch off and on, fp32 table; their sum beside the
     step of (b), which runs without the phase events.
  d. agreement: the largest difference between the two sides over the largest magnitude of the
     off side, for the scores, the loss and every weight gradient.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

PHASES = ("sampling", "host_read", "centre_forward", "second_forward", "head_forward",
          "head_backward", "second_backward", "centre_backward")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1M nodes / 10M edges (not cfg4)")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side, at least")
    ap.add_argument("--phase-steps", type=int, default=30, help="instrumented steps per side")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    n, e = (1_000_000, 10_000_000) if args.small else (10_000_000, 100_000_000)
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    import torch.nn.functional as Fn
    if not torch.cuda.is_available():
        raise SystemExit("tools/unsup_head_ab.py needs a ROCm device: no CPU path to time")
    from graphneuralnetwork_amd import _lib, graphsage, ops
    from graphneuralnetwork_amd import sampler as S
    from graphneuralnetwork_amd.graphsage import GraphSAGE, _SageScoreFn, unsupervised_loss
    from graphneuralnetwork_amd.rmat import rmat_edges
    from sage_train_ab import HBM_BYTES_PER_S, K, WINDOW, compare, summary
    from spmm_bf16_ab import alternate
    dev = torch.device("cuda:0")
    F = H = args.feat
    fanouts = (25, 10)
    # the dataset and the batch of tools/sage_train_ab.py
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
    pu = S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, contexts=ctx_b,
                                     negatives=neg_b)
    qu = S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, contexts=ctx_b,
                                     negatives=neg_b, sync=False)
    labels = pu.labels
    Sn = labels.shape[1]
    y_u = labels.to(torch.float32)
    res.update({"workload": "cfg4" if not args.small else "small", "nodes": n, "edges": e,
                "feat": F, "hidden": H, "seeds": B, "window": WINDOW, "K": K, "S": Sn,
                "fanout": list(fanouts), "switch": "graphsage.SAGE_SCORE_FUSED",
                "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "centre_tower_layers": list(pu.center.layer_sizes),
                "second_tower_layers": list(pu.context.layer_sizes),
                "timing": f"device events around blocks of calls, sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})
    torch.manual_seed(0)
    net = GraphSAGE(2, F, H, False, agg_func="MEAN", Unsupervised=True).to(dev).train()
    none5 = (None,) * 5

    def towers(a):
        centre, _ = net(*a[:4], *none5)
        second, _ = net(*a[4:8], *none5)
        return centre, second

    # ---- a. the head alone, on the embeddings the towers give this batch
    with torch.no_grad():
        c0, x0 = towers(pu.forward_args(table))
    c0, x0 = c0.clone().requires_grad_(), x0.reshape(B, Sn, H).clone().requires_grad_()

    def head_torch():
        sc = torch.bmm(c0.unsqueeze(1), x0.permute(0, 2, 1))
        loss = Fn.binary_cross_entropy_with_logits(sc.reshape(labels.shape).float(),
                                                   labels.float())
        dc, dx = torch.autograd.grad(loss, (c0, x0))
        return sc, loss, dc.contiguous(), dx.contiguous()

    def head_fused():
        sc = _SageScoreFn.apply(c0, x0)
        loss = unsupervised_loss(sc, labels)
        dc, dx = torch.autograd.grad(loss, (c0, x0))
        return sc, loss, dc, dx

    graphsage.SAGE_SCORE_FUSED = True
    cd, xd = c0.detach(), x0.detach().reshape(B * Sn, H)
    z = ops.sage_score(cd, xd, Sn)
    _, g = ops.bce_logits(z, labels)
    t = alternate(torch, {
        "torch_head": head_torch, "fused_head": head_fused,
        "sage_score": lambda: ops.sage_score(cd, xd, Sn),
        "bce_logits": lambda: ops.bce_logits(z, labels),
        "sage_score_backward": lambda: ops.sage_score_backward(g, cd, xd)}, args.seconds, 8)
    head = {k_: summary(v) for k_, v in t.items()}
    head["torch_over_fused"] = head["torch_head"]["median_ms"] / head["fused_head"]["median_ms"]
    head["fused_faster_outside_block_ranges"] = (head["fused_head"]["max_ms"]
                                                 < head["torch_head"]["min_ms"])
    for name, nbytes in (("sage_score", (B * Sn * H + B * H) * 4),
                         ("sage_score_backward", 2 * B * Sn * H * 4)):
        head[name]["bytes_from_shapes"] = nbytes
        head[name]["share_of_8TBps_from_shapes"] = (nbytes / (head[name]["median_ms"] * 1e-3)
                                                    / HBM_BYTES_PER_S)
    a_, b_ = head_torch(), head_fused()
    head["fused_vs_torch_max_abs_diff_over_max_abs"] = {
        k_: float((q.detach() - p.detach()).abs().max() / p.detach().abs().max())
        for k_, p, q in zip(("scores", "loss", "d_center", "d_second"), a_, b_)}
    head["d_second_contiguous"] = {"torch_before_copy": bool(torch.autograd.grad(
        torch.bmm(c0.unsqueeze(1), x0.permute(0, 2, 1)).sum(), x0)[0].is_contiguous()),
        "fused": bool(b_[3].is_contiguous())}
    del a_, b_
    res["head_alone"] = head
    print(json.dumps({"head_alone": head}), flush=True)
    write()

    # ---- b. the step and the pending inference forward, off / on, fp32 / bf16
    def step(tab, fused):
        a = pu.forward_args(tab)

        def fn():
            graphsage.SAGE_SCORE_FUSED = fused
            net.zero_grad(set_to_none=True)
            _, score = net(*a)
            if fused:
                unsupervised_loss(score, labels).backward()
            else:  # the previous path, as tools/sage_train_ab.py times it
                Fn.binary_cross_entropy_with_logits(score.squeeze(1), y_u).backward()
        return fn

    def infer(tab, fused):
        a = qu.forward_args(tab)

        def fn():
            graphsage.SAGE_SCORE_FUSED = fused
            with torch.no_grad():
                return net(*a)
        return fn

    for name, make in (("unsupervised_step", step), ("unsupervised_pending_inference", infer)):
        net.train(make is step)
        t = alternate(torch, {"fp32_off": make(table, False), "fp32_on": make(table, True),
                              "bf16_off": make(table16, False), "bf16_on": make(table16, True)},
                      args.seconds, 1)
        res[name] = compare(t)
        res[name]["bf16_on_not_slower"] = (res[name]["bf16_on"]["median_ms"]
                                           <= res[name]["bf16_off"]["median_ms"])
        print(json.dumps({name: res[name]}), flush=True)
        write()
    net.train()

    # ---- d. the same numbers? one step per side on the fp32 table
    got = {}
    for fused in (False, True):
        graphsage.SAGE_SCORE_FUSED = fused
        net.zero_grad(set_to_none=True)
        _, score = net(*pu.forward_args(table))
        loss = (unsupervised_loss(score, labels) if fused else
                Fn.binary_cross_entropy_with_logits(score.squeeze(1), y_u))
        loss.backward()
        got[fused] = {"scores": score.detach(), "loss": loss.detach(),
                      **{k_: p.grad.clone() for k_, p in net.named_parameters()}}
    res["agreement_on_vs_off_max_abs_diff_over_max_abs"] = {
        k_: float((got[True][k_] - v).abs().max() / v.abs().max()) for k_, v in got[False].items()}
    print(json.dumps({"agreement": res["agreement_on_vs_off_max_abs_diff_over_max_abs"]}),
          flush=True)
    write()

    # ---- c. where one step's time goes: an event after every phase
    def phased(fused):
        graphsage.SAGE_SCORE_FUSED = fused
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
        net.zero_grad(set_to_none=True)
        ev[0].record()
        p = S.sample_unsupervised_batch(adj, seeds, fanouts, WINDOW, K, seed=1, contexts=ctx_b,
                                        negatives=neg_b, sync=False)
        ev[1].record()
        p = p.sync()
        ev[2].record()
        a = p.forward_args(table)
        centre, _ = net(*a[:4], *none5)
        ev[3].record()
        second, _ = net(*a[4:8], *none5)
        ev[4].record()
        cl, xl = centre.detach().requires_grad_(), second.detach().requires_grad_()
        x3 = xl.reshape(B, Sn, H)
        if fused:
            loss = unsupervised_loss(_SageScoreFn.apply(cl, x3), p.labels)
        else:
            sc = torch.bmm(cl.unsqueeze(1), x3.permute(0, 2, 1))
            loss = Fn.binary_cross_entropy_with_logits(sc.squeeze(1), y_u)
        ev[5].record()
        dc, dx = torch.autograd.grad(loss, (cl, xl))
        ev[6].record()
        second.backward(dx)
        ev[7].record()
        centre.backward(dc)
        ev[8].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(PHASES))]

    phases = {}
    for _ in range(3):  # warm both sides
        phased(False), phased(True)
    runs = {False: [], True: []}
    for _ in range(args.phase_steps):
        for fused in (False, True):
            runs[fused].append(phased(fused))
    for fused, key in ((False, "off"), (True, "on")):
        cols = list(zip(*runs[fused]))
        out = {ph: {"median_ms": statistics.median(c), "min_ms": min(c), "max_ms": max(c)}
               for ph, c in zip(PHASES, cols)}
        model = [sum(r[2:]) for r in runs[fused]]
        out["sum_of_model_phases_median_ms"] = statistics.median(model)
        out["sum_of_all_phases_median_ms"] = statistics.median(sum(r) for r in runs[fused])
        out["step_without_phase_events_median_ms"] = \
            res["unsupervised_step"][f"fp32_{key}"]["median_ms"]
        phases[key] = out
    phases["note"] = ("fp32 table; %d steps per side, alternated. The phase split runs the head on "
                      "detached embeddings and the towers' backward from the head's gradients, "
                      "so the two towers' weight gradients are accumulated as in the step. "
                      "second_backward per layer: not measured" % args.phase_steps)
    res["phases"] = phases
    graphsage.SAGE_SCORE_FUSED = True
    u = res["unsupervised_step"]
    res["switch_default_rule"] = {
        "fp32_on_faster_outside_block_ranges": u["fp32_on_faster_outside_block_ranges"],
        "bf16_on_not_slower": u["bf16_on_not_slower"],
        "default_true": bool(u["fp32_on_faster_outside_block_ranges"]
                             and u["bf16_on_not_slower"])}
    print(json.dumps({"phases": phases, "switch_default_rule": res["switch_default_rule"]}),
          flush=True)
    write()


if __name__ == "__main__":
    main()
