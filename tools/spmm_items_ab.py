"""Pass 1 of the XCD-sliced direct SpMM on the plain kernel against gnn_spmm_items_f32 (one
wave per item, the edge stream in scalar registers), measured in one process.

    python tools/spmm_items_ab.py --build-variants iu8,iu16            (CPU side)
    python tools/spmm_items_ab.py [--workload cfg2|ns] [--feat 128] [--variants iu8,iu16]
                                  [--out profiles/spmm_items_ab_cfg2.json]

Builds the workload as bench.py does (R-MAT graph, the normalised adjacency, the
column-degree-ordered graph A P^T, a bias row, ``out=Y``), warms every side, then times
``spmm_forward`` with ``ops.SPMM_ITEMS_KERNEL`` off / on / off-again in turn: ``--rounds``
rounds of ``--steps`` device-event-timed steps per side. ``off`` against ``off_again`` is the
A/A spread of the process. ``--variants``: the switch on, through a variant library of
tools/lib_ab.py (``iu8`` / ``iu16``: batches of 8 / 16 edges at both widths). Every side's
full output is compared with ``off``'s (``torch.equal``) before the timing. Reports the median
of the rounds' means.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "ns"])
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--variants", default="", help="lib_ab.py tags timed with the switch on")
    ap.add_argument("--build-variants", default="", help="build these tags and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.build_variants:
        from graphneuralnetwork_amd.build import build_variant
        from lib_ab import VARIANTS
        for tag in args.build_variants.split(","):
            print(build_variant(tag, VARIANTS[tag], only=["spmm.hip"]))
        return
    import torch
    from graphneuralnetwork_amd import _lib, ops
    from graphneuralnetwork_amd.preprocess import gcn_adjacency
    from graphneuralnetwork_amd.rmat import rmat_edges
    dev = torch.device("cuda:0")
    n, e = (1_000_000, 10_000_000) if args.workload == "cfg2" else (10_000_000, 100_000_000)
    F = args.feat
    s, d = rmat_edges(n, e, 0)
    g = gcn_adjacency(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), n, device=dev)
    del s, d
    order = ops.column_order(g, F)
    if order is None:
        raise SystemExit("no column order for this graph: pass 1 does not run")
    ga = order.graph
    gen = torch.Generator(device=dev).manual_seed(0)
    bias = torch.randn(F, device=dev, generator=gen)
    X = torch.randn(n, F, device=dev, generator=gen)
    Y = torch.empty(n, F, device=dev)

    tags = [t for t in args.variants.split(",") if t]
    libs = {t: ROOT / "graphneuralnetwork_amd" / "lib" / "variants" / f"libgnn_{t}.so" for t in tags}
    for t, p in libs.items():
        if not p.exists():
            raise SystemExit(f"{p} missing: run --build-variants {t} first")
    sides = {"off": (False, None), "on": (True, None), "off_again": (False, None)}
    sides.update({f"on_{t}": (True, libs[t]) for t in tags})

    def select(side):
        on, lib = sides[side]
        ops.SPMM_ITEMS_KERNEL = on
        _lib.use_variant(lib)

    def step():
        ops.spmm_forward(ga, X, bias, out=Y)

    ref, equal = None, {}
    for side in sides:  # warm every side, and compare what it computes
        select(side)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        if ref is None:
            ref = Y.clone()
        equal[side] = bool(torch.equal(Y, ref))
    del ref
    times = {side: [] for side in sides}
    for _ in range(args.rounds):
        for side in sides:
            select(side)
            step()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                step()
            b.record()
            torch.cuda.synchronize()
            times[side].append(a.elapsed_time(b) / args.steps)
    select("on")
    _lib.use_variant(None)

    med = {side: statistics.median(t) for side, t in times.items()}
    aa = abs(med["off"] - med["off_again"])
    res = {"workload": args.workload, "nodes": n, "nnz": g.nnz, "feat": F,
           "device": torch.cuda.get_device_name(dev),
           "library_stamp": _lib.load().gnn_build_stamp().decode(),
           "timing": f"{args.rounds} rounds of {args.steps} device-event-timed steps per side, "
                     "sides in turn; median over the rounds' means",
           "sides": {side: {"median_ms": med[side], "min_ms": min(t), "max_ms": max(t),
                            "equal_to_off": equal[side],
                            "over_off": med[side] / med["off"]}
                     for side, t in times.items()},
           "aa_spread_ms": aa, "aa_spread_frac": aa / med["off"],
           "on_gain_ms": med["off"] - med["on"], "on_gain_frac": 1 - med["on"] / med["off"],
           "on_gain_over_aa_spread": (med["off"] - med["on"]) / aa if aa else None}
    print(json.dumps(res), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    if not all(equal.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
