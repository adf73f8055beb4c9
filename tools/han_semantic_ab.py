"""HAN's semantic attention in the kernels of csrc/han_semantic.hip (han.SemanticAttention over
han._SemanticFn, switch han.SEMANTIC_FUSED) against the reference's torch expression
(HAN/models/SemanticAttention.py:15-20), measured in one process.

    python tools/han_semantic_ab.py --out profiles/han_semantic_ab.json

The protocol is tools/sup_head_ab.py's: device events around blocks of calls, the sides
alternated, every side warmed first and given at least --seconds of timed work, median and
min-max of the block means (1000 calls per block up to N = 3,025, 40 at 100K, 8 at 1M). Needs
a ROCm device: there is nothing to fall back to.

  a. attention_alone: for N in {32, 3025, 100K, 1M}, M = 3, D in {32, 64}: the module's forward
     (no grad) and forward + backward (loss = sum(out * gy), gradients of z and the parameters),
     torch against fused; then the three calls of the ops alone -- forward (scores, finish,
     combine), backward for dz alone (dbeta, coefficients, the dz pass), backward for the
     parameters alone (dbeta, coefficients, the parameter pass, its reduction) -- with the bytes
     their arguments imply over their time as a share of 8 TB/s (bytes from the shapes, not
     measured HBM traffic); the peak of torch.cuda.max_memory_allocated over a forward +
     backward of each side above what is allocated before it.
  b. model_steps: three R-MAT metapath CsrGraphs (N = 1M, 10M edges each before symmetrising,
     seeds 0, 1, 2): a HANLayer(3, 64, 8, 8) inference forward and a
     HANModel(3, 64, 8, 7, [8], 0.6) training step (forward, cross entropy, backward), switch
     off and on.
  c. agreement: the largest difference between the sides over the largest magnitude on the off
     side, for the output and every gradient (dropout 0 in the model).

``--trace D``: only 3 + 20 forward and backward calls of the ops at N = 1M, M = 3, for the
per-kernel times of a profiler run (the stats file's rows of the han_* kernels are kept as
profiles/han_semantic_kernel_stats_1M_D<D>.csv):

    rocprofv3 --kernel-trace --stats -d bench_out/han_trace -o run --output-format csv -- \
        python3 tools/han_semantic_ab.py --trace 64 --out bench_out/unused.json
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
           "blocks": len(ms)}
    if nbytes is not None:
        out["bytes_from_shapes"] = nbytes
        out["share_of_8TBps_from_shapes"] = nbytes / (out["median_ms"] * 1e-3) / HBM_BYTES_PER_S
    return out


def compare(t, off, on):
    a, b = summary(t[off]), summary(t[on])
    return {off: a, on: b, "off_over_on": a["median_ms"] / b["median_ms"],
            "on_faster_outside_block_ranges": b["max_ms"] < a["min_ms"],
            "ranges_overlap": not (b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"])}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per side, at least")
    ap.add_argument("--small-block", type=int, default=1000,
                    help="calls per timed block at N <= 3025, where a call is bound by the host "
                         "(a block of 200 such calls, 30-60 ms, is no longer than one of the "
                         "host's own hiccups: profiles/han_semantic_ab_block200.json); such a "
                         "side gets at least 0.6 ms x this of timed work")
    ap.add_argument("--small", action="store_true", help="100K-node graphs (a rehearsal)")
    ap.add_argument("--no-model", action="store_true", help="skip the model steps")
    ap.add_argument("--trace", type=int, default=None, metavar="D",
                    help="only 23 forward + backward calls of the ops at N = 1M (for a profiler)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/han_semantic_ab.py needs a ROCm device: no CPU path to time")
    from graphneuralnetwork_amd import _lib, han, ops
    from spmm_bf16_ab import alternate
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    res.update({"switch": "han.SEMANTIC_FUSED", "default_min_rows": han.SEMANTIC_MIN_ROWS,
                "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "transform_precision": ops.transform_precision(),
                "timing": "device events around blocks of calls, sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})
    han.SEMANTIC_MIN_ROWS = None  # both sides at every size: the threshold is what this decides
    if args.trace is not None:
        N, M, D = 1_000_000, 3, args.trace
        att = han.SemanticAttention(D).to(dev)
        w1, b1, w2 = (p.detach() for p in att.parameters())
        z = torch.randn(N, M, D, device=dev, generator=gen)
        gy = torch.randn(N, D, device=dev, generator=gen)
        for _ in range(23):
            _, beta = ops.han_semantic_forward(z, w1, b1, w2)
            ops.han_semantic_backward(gy, z, w1, b1, w2, beta)
        torch.cuda.synchronize()
        return

    def set_side(fused):
        han.SEMANTIC_FUSED = fused

    # ---- a. the attention alone
    alone = {}
    M = 3
    for N in (32, 3025, 100_000, 1_000_000):
        for D in (32, 64):
            block = args.small_block if N <= 3025 else 40 if N <= 100_000 else 8
            seconds = max(args.seconds, 6e-4 * block) if N <= 3025 else args.seconds
            att = han.SemanticAttention(D).to(dev)
            z = (torch.randn(N, M, D, device=dev, generator=gen)
                 + 0.4 * torch.arange(M, device=dev).view(1, M, 1)).requires_grad_()
            gy = torch.randn(N, D, device=dev, generator=gen)
            zd = z.detach()
            l1, _, l2 = att.project
            w1, b1, w2 = l1.weight.detach(), l1.bias.detach(), l2.weight.detach()

            def fwd(fused):
                def fn():
                    set_side(fused)
                    with torch.no_grad():
                        return att(zd)
                return fn

            def fwdbwd(fused):
                def fn():
                    set_side(fused)
                    out = att(z)
                    return (out, *torch.autograd.grad((out * gy).sum(), [z, *att.parameters()]))
                return fn

            _, beta = ops.han_semantic_forward(zd, w1, b1, w2)
            zb, gb = N * M * D * 4, N * D * 4
            ops_alone = {
                "op_forward": (lambda: ops.han_semantic_forward(zd, w1, b1, w2), 2 * zb + gb),
                "op_backward_dz": (lambda: ops.han_semantic_backward(
                    gy, zd, w1, b1, w2, beta, need_params=False), 3 * zb + 2 * gb),
                "op_backward_params": (lambda: ops.han_semantic_backward(
                    gy, zd, w1, b1, w2, beta, need_dz=False), 2 * zb + gb)}
            sides = {"torch_forward": fwd(False), "fused_forward": fwd(True),
                     "torch_forward_backward": fwdbwd(False),
                     "fused_forward_backward": fwdbwd(True),
                     **{k: v[0] for k, v in ops_alone.items()}}
            for fn in sides.values():  # one untimed block each: the allocator's pool settles
                for _ in range(block):
                    fn()
            t = alternate(torch, sides, seconds, block)
            r = {"block": block, "seconds_per_side": seconds,
                 "forward": compare(t, "torch_forward", "fused_forward"),
                 "forward_backward": compare(t, "torch_forward_backward",
                                             "fused_forward_backward"),
                 **{k: summary(t[k], v[1]) for k, v in ops_alone.items()}}
            peak = {}
            for name, fused in (("torch", False), ("fused", True)):
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                got = fwdbwd(fused)()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated(dev) - base
                del got
            r["peak_bytes_forward_backward_above_inputs"] = peak
            a_, b_ = fwdbwd(False)(), fwdbwd(True)()
            r["fused_vs_torch_max_abs_diff_over_max_abs"] = {
                k: rel(y.detach(), x.detach())
                for k, x, y in zip(("out", "dz", "dW1", "db1", "dw2"), a_, b_)}
            del a_, b_
            alone[f"N={N},M={M},D={D}"] = r
            print(json.dumps({f"N={N},D={D}": {
                "fwd torch/fused ms": [r["forward"]["torch_forward"]["median_ms"],
                                       r["forward"]["fused_forward"]["median_ms"]],
                "fwd+bwd torch/fused ms": [
                    r["forward_backward"]["torch_forward_backward"]["median_ms"],
                    r["forward_backward"]["fused_forward_backward"]["median_ms"]]}}), flush=True)
            res["attention_alone"] = alone
            write()
            del att, z, gy, zd, sides, ops_alone
    set_side(True)
    if args.no_model:
        return

    # ---- b. the model steps, switch off / on
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    from graphneuralnetwork_amd.rmat import rmat_edges
    n, e = (100_000, 1_000_000) if args.small else (1_000_000, 10_000_000)
    gs = []
    for seed in range(3):
        s, d = rmat_edges(n, e, seed)
        gs.append(gcn_adjacency(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), n,
                                device=dev))
        del s, d
    X = torch.randn(n, 64, device=dev, generator=gen)
    y = torch.randint(0, 7, (n,), device=dev, generator=gen)
    print("dataset built", flush=True)
    torch.manual_seed(0)
    layer = han.HANLayer(3, 64, 8, 8, 0.6).to(dev).eval()

    def infer(fused):
        def fn():
            set_side(fused)
            with torch.no_grad():
                return layer(gs, X)
        return fn

    t = alternate(torch, {"off": infer(False), "on": infer(True)}, args.seconds, 2)
    res["model_steps"] = {"nodes": n, "edges_per_metapath_before_symmetrising": e,
                          "hanlayer_inference": {"what": "HANLayer(3, 64, 8, 8, 0.6).eval() forward",
                                                 **compare(t, "off", "on")}}
    a_, b_ = infer(False)(), infer(True)()
    agreement = {"hanlayer_inference_out": rel(b_, a_)}
    del a_, b_, layer
    write()

    def make(p):
        torch.manual_seed(0)
        return han.HANModel(3, 64, 8, 7, [8], p).to(dev).train()

    def step(m, fused):
        def fn():
            set_side(fused)
            m.zero_grad(set_to_none=True)
            out = m(gs, X)
            loss = torch.nn.functional.cross_entropy(out, y)
            loss.backward()
            return out, loss
        return fn

    model = make(0.6)
    t = alternate(torch, {"off": step(model, False), "on": step(model, True)}, args.seconds, 1)
    res["model_steps"]["hanmodel_training_step"] = {
        "what": "HANModel(3, 64, 8, 7, [8], 0.6).train(): forward, cross entropy, backward",
        **compare(t, "off", "on")}
    write()

    # ---- c. the same numbers? one step per side of the same model without dropout
    del model
    model = make(0.0)
    got = {}
    for fused in (False, True):
        out, loss = step(model, fused)()
        got[fused] = {"out": out.detach(), "loss": loss.detach(),
                      **{k: p.grad.clone() for k, p in model.named_parameters()
                         if p.grad is not None}}
    agreement.update({k: rel(got[True][k], v) for k, v in got[False].items()})
    res["agreement_on_vs_off_max_abs_diff_over_max_abs"] = agreement
    set_side(True)
    print(json.dumps({k: res[k] for k in ("model_steps",
                                          "agreement_on_vs_off_max_abs_diff_over_max_abs")}),
          flush=True)
    write()


if __name__ == "__main__":
    main()
