"""GATNE on the kernels of csrc/gatne.hip (graphneuralnetwork_amd.gatne, switch gatne.GATNE_FUSED)
against the reference's torch lines on the same device tensors (the module's fallback), measured
in one process.

    python tools/gatne_ab.py --out profiles/gatne_ab.json

The protocol is tools/han_semantic_ab.py's: device events around blocks of calls, the sides
alternated, every side warmed first and given at least --seconds of timed work; median and
min-max of the block means. Needs a ROCm device.

  shapes: run.py's defaults (N = 10,000, T = 2, K = 10, B = 1024, S = 30, widths E, U, A =
     256, 128, 128) and a large one (N = 1M, T = 5, K = 10, B = 8192, S = 30, the same widths).
  per shape: the encoder forward (no grad); forward + loss + backward of the whole model (the
     loss line of train_utils/train_eval.py:119); the training step (zero_grad, forward, loss,
     backward, AdamW step); the peak of torch.cuda.max_memory_allocated over a forward + backward
     of each side above what is allocated before it; the largest difference between the sides
     over the largest magnitude on the torch side for pred and every gradient.
  embed_all_types (chunks of 4096 nodes, all N nodes) against ValScale.get_model's loop of one
     encoder call per node: the loop is timed over a slice of nodes and EXTRAPOLATED to N
     (``loop_extrapolated_ms``); nobody waits for a million calls.
  rows: at the default shape, the encoder forward and forward + backward at B in
     {16, 64, 256, 1024}: whether small batches need a row threshold (they do not: none exists).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "blocks": len(ms)}


def compare(t, off, on):
    a, b = summary(t[off]), summary(t[on])
    return {off: a, on: b, "torch_over_fused": a["median_ms"] / b["median_ms"],
            "fused_faster_outside_block_ranges": b["max_ms"] < a["min_ms"],
            "ranges_overlap": not (b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"])}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per side, at least")
    ap.add_argument("--block", type=int, default=20, help="calls per timed block")
    ap.add_argument("--loop-nodes", type=int, default=300,
                    help="nodes of the per-node loop that are timed (the rest is extrapolated)")
    ap.add_argument("--no-large", action="store_true", help="the default shape only")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gatne_ab.py needs a ROCm device: no CPU path to time")
    from graphneuralnetwork_amd import _lib, gatne
    from spmm_bf16_ab import alternate
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    res.update({"switch": "gatne.GATNE_FUSED",
                "check_indices": gatne.CHECK_INDICES,
                "device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "timing": "device events around blocks of calls, sides alternated, >= "
                          f"{args.seconds} s per side; median and min-max over block means"})
    E, U, A = 256, 128, 128
    loss_fn = gatne.SigmoidBCELoss()

    def set_side(fused):
        gatne.GATNE_FUSED = fused

    def batch(N, T, K, B, S):
        ri = lambda hi, *s: torch.randint(0, hi, s, device=dev, generator=gen)  # noqa: E731
        masks = (torch.rand(B, S, device=dev, generator=gen) < 0.7).float()
        masks[:, 0] = 1
        labels = torch.zeros(B, S, device=dev)
        labels[:, 0] = 1
        return ri(N, B), ri(T, B), ri(N, B, T, K), ri(N, B, S), masks, labels

    def sides_of(model, b, opt=None):
        c, ty, nb, cx, mk, lb = b

        def enc(fused):
            def fn():
                set_side(fused)
                with torch.no_grad():
                    return model.encoder(c, ty, nb)
            return fn

        def fwdbwd(fused):
            def fn():
                set_side(fused)
                model.zero_grad(set_to_none=True)
                pred = model(c, ty, nb, cx)
                (loss_fn(pred, lb, mk) / mk.sum(axis=1) * mk.shape[1]).sum().backward()
                return pred
            return fn

        def train(fused):
            def fn():
                fwdbwd(fused)()
                opt.step()
            return fn
        return enc, fwdbwd, train

    shapes = {"defaults": dict(N=10_000, T=2, K=10, B=1024, S=30)}
    if not args.no_large:
        shapes["large"] = dict(N=1_000_000, T=5, K=10, B=8192, S=30)
    for name, s in shapes.items():
        torch.manual_seed(0)
        model = gatne.GATNEModel(s["N"], E, U, s["T"], A, None).to(dev)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-3)
        b = batch(s["N"], s["T"], s["K"], s["B"], s["S"])
        enc, fwdbwd, train = sides_of(model, b, opt)
        r = {"shape": {**s, "E": E, "U": U, "A": A}}
        # the same numbers? (before any optimiser step)
        got = {}
        for fused in (False, True):
            pred = fwdbwd(fused)()
            got[fused] = {"pred": pred.detach(),
                          **{k: p.grad.clone() for k, p in model.named_parameters()}}
        r["fused_vs_torch_max_abs_diff_over_max_abs"] = {k: rel(got[True][k], v)
                                                         for k, v in got[False].items()}
        del got
        peak = {}
        for side, fused in (("torch", False), ("fused", True)):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            fwdbwd(fused)()
            torch.cuda.synchronize()
            peak[side] = torch.cuda.max_memory_allocated(dev) - base
        r["peak_bytes_forward_backward_above_inputs"] = peak
        block = args.block if name == "defaults" else max(args.block // 5, 2)
        t = alternate(torch, {"torch": enc(False), "fused": enc(True)}, args.seconds, block)
        r["encoder_forward"] = compare(t, "torch", "fused")
        t = alternate(torch, {"torch": fwdbwd(False), "fused": fwdbwd(True)}, args.seconds, block)
        r["forward_backward"] = compare(t, "torch", "fused")
        t = alternate(torch, {"torch": train(False), "fused": train(True)}, args.seconds, block)
        r["training_step"] = compare(t, "torch", "fused")
        res[name] = r
        write()
        print(json.dumps({name: {k: [r[k]["torch"]["median_ms"], r[k]["fused"]["median_ms"]]
                                 for k in ("encoder_forward", "forward_backward",
                                           "training_step")}}), flush=True)

        # embed_all_types against the per-node loop (a slice, extrapolated)
        model.zero_grad(set_to_none=True)
        N, T, K = s["N"], s["T"], s["K"]
        nbr = torch.randint(0, N, (N, T, K), device=dev, generator=gen)
        types = torch.arange(T, device=dev)
        n_loop = min(args.loop_nodes, N)

        def loop(fused):
            def fn():
                set_side(fused)
                with torch.no_grad():
                    for i in range(n_loop):
                        model.encoder(torch.full((T,), i, device=dev), types,
                                      nbr[i].unsqueeze(0).expand(T, T, K))
            return fn

        def all_types(fused):
            def fn():
                set_side(fused)
                return model.encoder.embed_all_types(nbr, chunk=4096)
            return fn

        t = alternate(torch, {"loop_torch": loop(False), "loop_fused": loop(True),
                              "all_torch": all_types(False), "all_fused": all_types(True)},
                      args.seconds, 1)
        ev = {k: summary(v) for k, v in t.items()}
        for k in ("loop_torch", "loop_fused"):
            ev[k]["nodes_timed"] = n_loop
            ev[k]["loop_extrapolated_ms"] = ev[k]["median_ms"] * N / n_loop
            ev[k]["extrapolated"] = f"measured over {n_loop} nodes, scaled to N = {N}"
        ev["all_types"] = compare(t, "all_torch", "all_fused")
        r["embed_all_types"] = ev
        write()
        print(json.dumps({name: {"loop (extrapolated) ms": ev["loop_torch"]["loop_extrapolated_ms"],
                                 "embed_all_types torch/fused ms": [
                                     ev["all_torch"]["median_ms"], ev["all_fused"]["median_ms"]]}}),
              flush=True)
        del model, opt, b, nbr

    # ---- would a row threshold pay? small batches at the default shape
    s = shapes["defaults"]
    torch.manual_seed(0)
    model = gatne.GATNEModel(s["N"], E, U, s["T"], A, None).to(dev)
    rows = {}
    for B in (16, 64, 256, 1024):
        b = batch(s["N"], s["T"], s["K"], B, s["S"])
        enc, fwdbwd, _ = sides_of(model, b)
        block = 200
        seconds = max(args.seconds, 1e-3 * block)
        t = alternate(torch, {"torch": enc(False), "fused": enc(True)}, seconds, block)
        t2 = alternate(torch, {"torch": fwdbwd(False), "fused": fwdbwd(True)}, seconds, block)
        rows[f"B={B}"] = {"block": block, "encoder_forward": compare(t, "torch", "fused"),
                          "forward_backward": compare(t2, "torch", "fused")}
        res["rows_at_defaults"] = rows
        write()
        print(json.dumps({f"B={B}": {k: [v["torch"]["median_ms"], v["fused"]["median_ms"]]
                                     for k, v in rows[f"B={B}"].items() if k != "block"}}),
              flush=True)
    set_side(True)


if __name__ == "__main__":
    main()
