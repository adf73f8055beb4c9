"""GTN on an EdgeTypeGraph (gtn.GTN_Model over csrc/gtn.hip) against the reference's dense
lines (the same model given the dense [N, N, T] tensor) on the same device, in one process.

    python tools/gtn_ab.py --out profiles/gtn_ab.json

Graph: P papers, A authors, S subjects; ``--per-row`` (3) authors per paper drawn with
``numpy.random.default_rng(seed).choice(A, p ~ 1 / (rank + 1) ** 0.5)`` (a Zipf-like author
popularity), one uniformly drawn subject per paper; relations PA, AP, PS, SP and I, T = 5.
``acm`` is the ACM shape (3,025 papers, 5,912 authors, 57 subjects; N = 8,994), where both
paths run; ``100K`` and ``1M`` papers keep ACM's ratios and run the sparse path alone (a single
dense [N, N] fp32 slice would be 354 GB and 35 TB; ``--no-dense`` skips the dense side at
``acm`` too). Model: C = 2 channels, w_in = 64,
w_out = 64, 3 classes, L = 2 and 3 layers; the loss is cross-entropy over 1,000 target papers.

Every timed call is wall clock around the call and a device synchronise; blocks of calls, the
sides alternated, median and min-max of the block means (the protocol of tools/metapath_ab.py).
Peak memory is torch.cuda.max_memory_allocated above what is allocated before the call (the
inputs and the parameters; for the sparse path the cached patterns too, stated separately).
No threshold switches paths -- the input type decides -- so there is no pass/fail ratio here:
the file records what was measured.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"acm": (3025, 5912, 57), "100K": (100_000, 195_440, 1884),
          "1M": (1_000_000, 1_954_400, 18_843)}
EXPONENT = 0.5


def relations(P, A, S, per_row, seed):
    """[(row, col)] of PA, AP, PS, SP and I over N = P + A + S nodes."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, A + 1) ** EXPONENT
    p /= p.sum()
    paper = np.repeat(np.arange(P, dtype=np.int64), per_row)
    author = rng.choice(A, size=paper.size, p=p).astype(np.int64) + P
    key = np.unique(paper * (P + A + S) + author)          # one edge per (paper, author)
    paper, author = key // (P + A + S), key % (P + A + S)
    sp = np.arange(P, dtype=np.int64)
    subject = rng.integers(0, S, size=P).astype(np.int64) + P + A
    eye = np.arange(P + A + S, dtype=np.int64)
    return [(paper, author), (author, paper), (sp, subject), (subject, sp), (eye, eye)]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "blocks": len(ms)}


def timed_blocks(sides, seconds, block, sync):
    """{name: [ms per call, one per block]}: blocks of ``block`` calls per side (an int, or a
    dict by side: sides of very different cost get blocks of similar length), alternating, until
    every side has ``seconds`` of timed work (at least 3 blocks each)."""
    if not isinstance(block, dict):
        block = {k: block for k in sides}
    times = {k: [] for k in sides}
    total = {k: 0.0 for k in sides}
    for fn in sides.values():
        fn()
    sync()
    while min(total.values()) < seconds or min(len(v) for v in times.values()) < 3:
        for k, fn in sides.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(block[k]):
                fn()
            sync()
            t = time.perf_counter() - t0
            total[k] += t
            times[k].append(t * 1e3 / block[k])
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per side, at least")
    ap.add_argument("--per-row", type=int, default=3)
    ap.add_argument("--shapes", default="acm,100K,1M")
    ap.add_argument("--layers", default="2,3")
    ap.add_argument("--no-dense", action="store_true", help="skip the dense reference lines")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {}

    def write():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("tools/gtn_ab.py needs a ROCm device")
    from graphneuralnetwork_amd import _lib, gtn, hetero, ops
    from graphneuralnetwork_amd.graph import from_coo
    dev = torch.device("cuda:0")

    def sync():
        torch.cuda.synchronize(dev)

    def log(*a):
        print("[gtn_ab]", *a, file=sys.stderr, flush=True)

    lane_max, chunk = ops.masked_product_class_limits()
    res.update({"device": torch.cuda.get_device_name(dev),
                "library_stamp": _lib.load().gnn_build_stamp().decode(),
                "generator": f"numpy default_rng(0).choice(A, p ~ 1/(rank+1)^{EXPONENT}), "
                             f"{args.per_row} authors per paper (duplicates dropped), one "
                             "uniform subject per paper",
                "model": "GTN_Model(5, 2, 64, 64, 3, L, True), conv weights normal(0, 1), "
                         "seed 0; cross-entropy over 1,000 target papers",
                "class_limits": {"lane_max": lane_max, "wave_chunk": chunk},
                "timing": "wall clock around blocks of calls and a device synchronise, sides "
                          f"alternated, >= {args.seconds} s and >= 3 blocks per side; median "
                          "and min-max over block means"})
    shapes = {}
    for name in args.shapes.split(","):
        P, A, S = SHAPES[name]
        N = P + A + S
        rels = relations(P, A, S, args.per_row, 0)
        graphs = [from_coo(torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev),
                           torch.ones(r.size, device=dev), N, N, check=False) for r, c in rels]
        etg = hetero.edge_type_graph(graphs)
        gen = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(N, 64, device=dev, generator=gen)
        target = torch.randperm(P, device=dev, generator=gen)[:1000]
        labels = torch.randint(0, 3, (1000,), device=dev, generator=gen)
        dense = None
        if name == "acm" and not args.no_dense:
            dense = torch.zeros((N, N, 5), device=dev)
            for t, (r, c) in enumerate(rels):
                dense[torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev), t] = 1
        deg = etg.U.rowptr[1:] - etg.U.rowptr[:-1]
        r_ = {"papers": P, "authors": A, "subjects": S, "N": N, "nnz_U": int(etg.U.nnz),
              "max_row_U": int(deg.max()), "max_subject_row_U": int(deg[P + A:].max()),
              "layers": {}}
        for L in (int(v) for v in args.layers.split(",")):
            torch.manual_seed(0)
            model = gtn.GTN_Model(5, 2, 64, 64, 3, L, True).to(dev)
            with torch.no_grad():
                for k_, p_ in model.named_parameters():
                    if ".conv" in k_ and k_.endswith("weight"):
                        p_.normal_()

            def forward(a):
                with torch.no_grad():
                    return model(a, X, target)[0]

            def train(a):
                model.zero_grad(set_to_none=True)
                y = model(a, X, target)[0]
                F.cross_entropy(y, labels).backward()
                return y

            sync()
            t0 = time.perf_counter()
            nnz_s = [int(etg.S(l).nnz) for l in range(2, L + 2)]     # builds and caches S_l
            for l in range(1, L + 2):
                etg.S(l).T
            sync()
            r = {"nnz_S": {f"S{l}": v for l, v in zip(range(2, L + 2), nnz_s)},
                 "pattern_build_ms_once_per_graph": (time.perf_counter() - t0) * 1e3,
                 "pattern_bytes": int(sum(
                     8 * (etg.S(l).g.rowptr.numel() + etg.S(l).T.g.rowptr.numel())
                     + 4 * 2 * etg.S(l).nnz + 8 * 2 * etg.S(l).nnz for l in range(1, L + 2)))}
            sides_f = {"sparse": lambda: forward(etg)}
            sides_t = {"sparse": lambda: train(etg)}
            if dense is not None:
                sides_f["dense_reference_lines"] = lambda: forward(dense)
                sides_t["dense_reference_lines"] = lambda: train(dense)
            block = 50 if name == "acm" else 1
            log(name, f"L={L}", "patterns built", r["nnz_S"])
            for what, sides in (("forward", sides_f), ("forward_backward", sides_t)):
                for side, fn in sides.items():          # one call each, timed and shown
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    log(name, f"L={L}", what, side, "first call",
                        f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
                t = timed_blocks(sides, args.seconds,
                                 {"sparse": block, "dense_reference_lines": 1}, sync)
                log(name, f"L={L}", what, {k_: statistics.median(v) for k_, v in t.items()})
                r[what] = {k_: summary(v) for k_, v in t.items()}
                if dense is not None:
                    r[what]["dense_over_sparse"] = (r[what]["dense_reference_lines"]["median_ms"]
                                                    / r[what]["sparse"]["median_ms"])
                peak = {}
                for side, fn in sides.items():
                    sync()
                    model.zero_grad(set_to_none=True)
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    fn()
                    sync()
                    peak[side] = torch.cuda.max_memory_allocated(dev) - base
                r[what]["peak_bytes_above_inputs"] = peak
            if dense is not None:
                ys, yd = forward(etg), forward(dense)
                r["max_abs_y_difference"] = float((ys - yd).abs().max())
                r["max_abs_y"] = float(yd.abs().max())
            # the three graph operations of the sparse step, each alone (forward + adjoint)
            u = etg.pattern
            q = torch.rand((2, u.nnz), device=dev, requires_grad=True)
            qt = torch.rand((2, u.nnz), device=dev, requires_grad=True)
            s2 = etg.S(2)
            h = torch.rand((2, s2.nnz), device=dev, requires_grad=True)
            xw = torch.randn(N, 64, device=dev, requires_grad=True)
            s3 = etg.S(3)
            last = etg.S(L + 1)
            hl = torch.rand((2, last.nnz), device=dev, requires_grad=True)

            def fb(fn, *ins):
                out = fn()
                torch.autograd.grad(out, ins, torch.ones_like(out))

            parts = {
                "product_first_layer_S2": lambda: fb(
                    lambda: gtn._MaskedProduct.apply(q, qt, 0, u, u, s2), q, qt),
                "product_next_layer_S3": lambda: fb(
                    lambda: gtn._MaskedProduct.apply(h, qt, 1, s2, u.T, s3), h, qt),
                "norm_S2": lambda: fb(lambda: gtn._Norm.apply(h, s2), h),
                f"aggregate_S{L + 1}": lambda: fb(
                    lambda: gtn._Aggregate.apply(hl, xw, last), hl, xw)}
            parts_fwd = {
                "product_first_layer_S2": lambda: gtn._product(0, u, q.detach(), u, qt.detach(),
                                                               s2),
                "product_next_layer_S3": lambda: gtn._product(1, s2, h.detach(), u.T,
                                                              qt.detach(), s3)}
            log(name, f"L={L}", "parts")
            t = timed_blocks(parts, args.seconds / 2, block, sync)
            r["parts_forward_backward"] = {k_: summary(v) for k_, v in t.items()}
            t = timed_blocks(parts_fwd, args.seconds / 2, block, sync)
            r["parts_forward"] = {k_: summary(v) for k_, v in t.items()}
            # the hub rows: the product restricted to P's subject rows
            rows = torch.arange(P + A, N, device=dev)
            sub = s2.g.rowptr[rows + 1] - s2.g.rowptr[rows]
            r["subject_rows"] = {"rows": S, "nnz_S2_in_them": int(sub.sum()),
                                 "longest_S2_row": int(sub.max()),
                                 "walked_row_length_max": int(deg[P + A:].max())}
            from graphneuralnetwork_amd.graph import CsrGraph
            rp = torch.zeros(N + 1, dtype=torch.int64, device=dev)
            rp[P + A + 1:] = torch.cumsum(sub, 0)
            lo = int(s2.g.rowptr[P + A])
            hub = CsrGraph(rp, s2.g.col[lo:].contiguous(),
                           torch.ones(s2.nnz - lo, device=dev), N, N)
            qd, qtd = q.detach(), qt.detach()
            t = timed_blocks({"hub_rows_only": lambda: ops.masked_product(
                0, u.g, qd, u.g, qtd, hub, validate=False)}, args.seconds / 2, block, sync)
            r["subject_rows"]["product_ms"] = summary(t["hub_rows_only"])
            r_["layers"][f"L{L}"] = r
            shapes[name] = r_
            res["shapes"] = shapes
            print(json.dumps({name: {f"L{L}": r}}), flush=True)
            write()
            del model, q, qt, h, xw, hl, hub
        del etg, dense, graphs, X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
