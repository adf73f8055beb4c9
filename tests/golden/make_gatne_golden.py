"""Generate tests/golden/gatne.npz by running the REFERENCE GATNE model.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gatne_golden.py

A fresh subprocess puts the reference's GATNE_Pytorch directory on sys.path and runs the
reference's ``GATNEModel`` and ``SigmoidBCELoss`` in fp32 on the CPU for eight cases: widths
(E, U, A) = (32, 16, 16) and (64, 32, 16), agg_func SUM and MEAN, with and without ``features``
(F = 12). All share one seeded batch: N = 97 nodes, T = 3 edge types, K = 5 neighbours, B = 37
rows, S = 7 contexts. Edge type 1 is absent from the batch; centres, neighbours and contexts
repeat (drawn from small pools); row 5 has e = 0 exactly (a zero centre row -- node 3's
embedding, or its feature row -- and trans_weights[2] = 0, the type of that row). Parameters are
the reference's own initialisation under a seed, rounded to multiples of 1/256 (exact in fp32,
so the file stays small) and shared by the SUM and MEAN cases. Stored: the inputs, every
parameter, ``pred``, the encoder output and every parameter gradient after the training loop's
loss line (train_utils/train_eval.py:119, with masks and labels) and ``.sum().backward()``.
Everything is asserted finite. Nothing from the reference is copied: only data is written.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
N, T, K, B, S, FEAT = 97, 3, 5, 37, 7, 12
WIDTHS = ((32, 16, 16), (64, 32, 16))
ZERO_NODE, ZERO_ROW, ZERO_TYPE = 3, 5, 2


def batch(rng):
    centres = rng.choice(rng.choice(N, size=8, replace=False), size=B).astype(np.int64)
    types = rng.choice(np.array([0, 2]), size=B).astype(np.int64)      # type 1 is absent
    centres[ZERO_ROW], types[ZERO_ROW] = ZERO_NODE, ZERO_TYPE
    centres[20] = ZERO_NODE                                            # the zero centre repeats
    nbr = rng.choice(rng.choice(N, size=12, replace=False), size=(B, T, K)).astype(np.int64)
    ctx = rng.choice(rng.choice(N, size=10, replace=False), size=(B, S)).astype(np.int64)
    masks = (rng.random((B, S)) < 0.7).astype(np.float32)
    masks[:, 0] = 1.0
    labels = np.zeros((B, S), np.float32)
    labels[:, 0] = 1.0
    feats = rng.standard_normal((N, FEAT)).astype(np.float32)
    feats[ZERO_NODE] = 0.0
    return centres, types, nbr, ctx, masks, labels, feats


def part_gatne():
    sys.path.insert(0, str(REF / "GATNE_Pytorch"))
    import torch
    from models.GATNE import GATNEModel                  # reference GATNE_Pytorch/models/GATNE.py
    from train_utils.loss_utils import SigmoidBCELoss    # reference train_utils/loss_utils.py
    rng = np.random.default_rng(41)
    centres, types, nbr, ctx, masks, labels, feats = batch(rng)
    out = dict(centres=centres, types=types, nbr=nbr, ctx=ctx, masks=masks, labels=labels,
               features=feats, widths=np.array(WIDTHS, np.int64),
               dims=np.array([N, T, K, B, S, FEAT], np.int64))
    tens = [torch.from_numpy(a) for a in (centres, types, nbr, ctx, masks, labels)]
    loss = SigmoidBCELoss()
    for wi, (E, U, A) in enumerate(WIDTHS):
        for fi, use_feat in enumerate((False, True)):
            state = None
            for agg in ("SUM", "MEAN"):
                torch.manual_seed(7 + 10 * wi + fi)
                model = GATNEModel(N, E, U, T, A, torch.from_numpy(feats) if use_feat else None)
                model.encoder.agg_func = agg             # the reference's model takes no kwargs
                with torch.no_grad():
                    for name, p in model.named_parameters():
                        p.copy_(torch.round(p * 256) / 256)
                    model.encoder.trans_weights[ZERO_TYPE].zero_()
                    if not use_feat:
                        model.encoder.node_embeddings[ZERO_NODE].zero_()
                tag = f"w{wi}_f{fi}"
                if state is None:                        # SUM and MEAN share the parameters
                    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
                    out[f"{tag}_keys"] = np.array(list(state))
                    for k, v in state.items():
                        out[f"{tag}_param_{k}"] = v.numpy()
                c, ty, nb, cx, mk, lb = tens
                enc = model.encoder(c, ty, nb)
                pred = model.decoder(enc, cx)
                train_loss = loss(pred.float(), lb.float(), mk) / mk.sum(axis=1) * mk.shape[1]
                train_loss.sum().backward()
                assert float(enc[ZERO_ROW].detach().abs().max()) == 0.0, "row 5: e = 0 exactly"
                case = f"{tag}_{agg}"
                out[f"{case}_enc"] = enc.detach().numpy()
                out[f"{case}_pred"] = pred.detach().numpy()
                assert np.isfinite(out[f"{case}_enc"]).all()
                assert np.isfinite(out[f"{case}_pred"]).all()
                for name, p in model.named_parameters():
                    g = p.grad.numpy()
                    assert np.isfinite(g).all(), (case, name)
                    out[f"{case}_grad_{name}"] = g
                print(f"{case}: pred {tuple(pred.shape)} max|pred| "
                      f"{float(pred.detach().abs().max()):.4f}, "
                      f"{sum(1 for _ in model.parameters())} parameters")
    np.savez_compressed(HERE / "gatne.npz", **out)
    print(f"gatne.npz: {(HERE / 'gatne.npz').stat().st_size} bytes")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    if len(sys.argv) > 1 and sys.argv[1] == "--part":
        part_gatne()
        sys.exit(0)
    if not REF.exists():
        sys.exit("the reference is not mounted at /root/reference: fixtures cannot be regenerated")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
    subprocess.run([sys.executable, __file__, "--part"], check=True, env=env,
                   cwd=tempfile.gettempdir())
