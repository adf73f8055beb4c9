"""The drop-in GATNE modules on the device (the kernels of csrc/gatne.hip behind
graphneuralnetwork_amd.gatne): the reference's fixture, the module's own fallback in float64,
tile edges, the scatter's chunk path, determinism, one optimiser step, unsupported widths and
``embed_all_types``.

Bounds (those of tests/test_han_semantic_gpu.py): ``pred`` and the encoder output element-wise,
rtol 1e-4 and atol 2e-5 max|ref|; parameter gradients -- weight and table gradients, sums over the
rows -- within 1e-4 of the largest entry."""
import copy

import numpy as np
import pytest
import torch

from test_gatne_cpu import CASES, build_model, close, train_loss

pytestmark = pytest.mark.gpu


def close_sum(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (np.abs(a - b).max(), np.abs(b).max())


@pytest.fixture(autouse=True)
def fused_on(monkeypatch):
    from graphneuralnetwork_amd import gatne
    monkeypatch.setattr(gatne, "GATNE_FUSED", True)


@pytest.fixture
def calls(monkeypatch):
    """How often the attention kernels ran: a test of the fused path must not pass on the
    fallback."""
    from graphneuralnetwork_amd import ops
    n = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.gatne_attend_forward, ops.gatne_attend_backward

    def f(*a, **k):
        n["fwd"] += 1
        return fwd(*a, **k)

    def b(*a, **k):
        n["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(ops, "gatne_attend_forward", f)
    monkeypatch.setattr(ops, "gatne_attend_backward", b)
    return n


def step(model, batch):
    model.zero_grad(set_to_none=True)
    enc, pred, loss = train_loss(model, batch)
    loss.backward()
    return enc.detach(), pred.detach(), {k: p.grad.detach().clone()
                                         for k, p in model.named_parameters()}


@pytest.mark.parametrize("w,f,agg", CASES)
def test_fixture_parity_on_the_device(golden, dev, calls, w, f, agg):
    g = golden("gatne")
    model, batch = build_model(g, w, f, agg, device=dev)
    enc, pred, grads = step(model, batch)
    assert calls == {"fwd": 1, "bwd": 1}
    case = f"w{w}_f{f}_{agg}"
    assert not enc[5].any()                         # the e = 0 row
    close(enc.cpu().numpy(), g[f"{case}_enc"])
    close(pred.cpu().numpy(), g[f"{case}_pred"])
    for name, grad in grads.items():
        close_sum(grad.cpu().numpy(), g[f"{case}_grad_{name}"])


def random_case(N, T, K, B, S, E, U, A, feat=0, agg="SUM", types=None, seed=0):
    """A seeded model on the CPU in float32 and a batch; centres and contexts repeat."""
    from graphneuralnetwork_amd import gatne
    gen = torch.Generator().manual_seed(seed + 31 * B + 7 * T + E)
    feats = torch.randn(N, feat, generator=gen) if feat else None
    torch.manual_seed(seed + 1)
    model = gatne.GATNEModel(N, E, U, T, A, feats, agg_func=agg)
    ri = lambda hi, *s: torch.randint(0, hi, s, generator=gen)  # noqa: E731
    types = ri(T, B) if types is None else types
    masks = (torch.rand(B, S, generator=gen) < 0.7).float()
    masks[:, 0] = 1
    labels = torch.zeros(B, S)
    labels[:, 0] = 1
    return model, [ri(N, B), types, ri(N, B, T, K), ri(N, B, S), masks, labels]


def on_device(model, batch, dev):
    m = copy.deepcopy(model).to(dev)
    if m.encoder.features is not None:
        m.encoder.features = m.encoder.features.to(dev)
    return m, [t.to(dev) for t in batch]


def in_float64(model, batch):
    """The module's fallback (CPU, float64: the reference's arithmetic op for op)."""
    m = copy.deepcopy(model).double()
    if m.encoder.features is not None:
        m.encoder.features = m.encoder.features.double()
    return m, batch


def check_against_float64(model, batch, dev, calls):
    enc, pred, grads = step(*on_device(model, batch, dev))
    assert calls["fwd"] >= 1 and calls["bwd"] >= 1
    renc, rpred, rgrads = step(*in_float64(model, batch))
    close(enc.cpu().numpy(), renc.numpy())
    close(pred.cpu().numpy(), rpred.numpy())
    for name, grad in grads.items():
        close_sum(grad.cpu().numpy(), rgrads[name].numpy())


@pytest.mark.parametrize("E,U,A", [(256, 128, 128), (16, 16, 16)])
@pytest.mark.parametrize("feat,agg", [(0, "SUM"), (0, "MEAN"), (12, "SUM")])
def test_widths_against_float64(dev, calls, E, U, A, feat, agg):
    model, batch = random_case(64, 2, 10, 50, 6, E, U, A, feat=feat, agg=agg)
    check_against_float64(model, batch, dev, calls)


EDGES = {
    "16_17_0": dict(N=40, T=3, K=4, B=33, types=torch.tensor([2] * 9 + [0] * 16 + [2] * 8)),
    "T1": dict(N=40, T=1, K=4, B=21),
    "T8": dict(N=40, T=8, K=3, B=45),
    "K1": dict(N=40, T=2, K=1, B=19),
    "B1": dict(N=40, T=2, K=4, B=1),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_tile_edges_against_float64(dev, calls, name):
    e = EDGES[name]
    model, batch = random_case(e["N"], e["T"], e["K"], e["B"], 5, 32, 16, 32,
                               types=e.get("types"))
    check_against_float64(model, batch, dev, calls)


def test_scatter_chunk_path_against_float64(dev, calls):
    """N = 5, T = 2, K = 10, B = 160: every (node, type) target of the table gradient is drawn
    about 320 times, over the 256 slots of a chunk; every centre about 32 times."""
    model, batch = random_case(5, 2, 10, 160, 4, 32, 16, 16)
    nbr = batch[2]
    ids = (nbr * 2 + torch.arange(2).view(1, 2, 1)).reshape(-1)
    assert int(torch.bincount(ids, minlength=10).min()) > 256
    check_against_float64(model, batch, dev, calls)


@pytest.mark.parametrize("feat", [0, 12])
def test_gradients_are_bit_identical_from_run_to_run(dev, calls, feat):
    model, batch = random_case(30, 3, 6, 70, 5, 64, 32, 16, feat=feat)
    m, b = on_device(model, batch, dev)
    e1, p1, g1 = step(m, b)
    e2, p2, g2 = step(m, b)
    assert calls["bwd"] == 2
    assert torch.equal(e1, e2) and torch.equal(p1, p2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_one_adamw_step_fused_and_fallback(dev, calls, monkeypatch):
    """The state after one AdamW step (run.py's weight decay) with the kernels and with
    GATNE_FUSED off, on the device. Adam's first step is lr g / (|g| + eps): with the default
    eps = 1e-8 it is lr sign(g), which turns the fp32 rounding of a gradient element near zero
    into a difference of 2 lr whatever produced it; eps = 1e-3 keeps the step a smooth function
    of g, so gradients equal within their bounds give states equal within theirs."""
    from graphneuralnetwork_amd import gatne
    model, batch = random_case(64, 2, 10, 50, 6, 64, 32, 32)
    states = []
    for fused in (True, False):
        monkeypatch.setattr(gatne, "GATNE_FUSED", fused)
        m, b = on_device(model, batch, dev)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-3, eps=1e-3)
        opt.zero_grad()
        train_loss(m, b)[2].backward()
        opt.step()
        states.append({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
    assert calls == {"fwd": 1, "bwd": 1}            # the second pass ran the fallback
    start = model.state_dict()
    for k in states[0]:
        assert not np.array_equal(states[0][k], start[k].numpy()), k     # the step moved it
        close(states[0][k], states[1][k])


def test_unsupported_width_runs_the_fallback(dev, calls):
    model, batch = random_case(30, 2, 4, 17, 3, 32, 24, 16)              # U = 24
    m, b = on_device(model, batch, dev)
    enc, pred, grads = step(m, b)
    assert calls == {"fwd": 0, "bwd": 0}
    renc, rpred, _ = step(*in_float64(model, batch))
    close(enc.cpu().numpy(), renc.numpy())
    close(pred.cpu().numpy(), rpred.numpy())


def test_hooked_module_and_features_with_grad_run_the_fallback(dev, calls):
    model, batch = random_case(30, 2, 4, 17, 3, 32, 16, 16, feat=12)
    m, b = on_device(model, batch, dev)
    m.encoder(b[0], b[1], b[2])
    assert calls["fwd"] == 1
    seen = []
    handle = m.encoder.register_forward_hook(lambda mod, args, out: seen.append(out.shape))
    hooked = m.encoder(b[0], b[1], b[2])
    handle.remove()
    assert calls["fwd"] == 1 and seen == [hooked.shape]
    m.encoder.features = m.encoder.features.clone().requires_grad_()
    out = m.encoder(b[0], b[1], b[2])
    assert calls["fwd"] == 1
    out.sum().backward()
    assert m.encoder.features.grad is not None


def test_check_indices_raises(dev, monkeypatch):
    from graphneuralnetwork_amd import gatne
    model, batch = random_case(30, 2, 4, 17, 3, 32, 16, 16)
    m, b = on_device(model, batch, dev)
    monkeypatch.setattr(gatne, "CHECK_INDICES", True)
    b[1] = b[1].clone()
    b[1][3] = 2                                                          # a type equal to T
    with pytest.raises(IndexError):
        m.encoder(b[0], b[1], b[2])
    monkeypatch.setattr(gatne, "CHECK_INDICES", False)
    out = m.encoder(b[0], b[1], b[2])
    assert bool(torch.isnan(out[3]).all()) and bool(torch.isfinite(out[:3]).all())


def test_embed_all_types_matches_the_loop(dev, calls):
    model, _ = random_case(40, 3, 5, 8, 3, 32, 16, 16)
    m = copy.deepcopy(model).to(dev)
    nbr = torch.randint(0, 40, (40, 3, 5))
    got = m.encoder.embed_all_types(nbr.to(dev), chunk=16)
    assert calls["fwd"] == 3                                             # 16 + 16 + 8 nodes
    with torch.no_grad():
        want = torch.stack([m.encoder(torch.tensor([i] * 3, device=dev),
                                      torch.arange(3, device=dev),
                                      torch.stack([nbr[i]] * 3).to(dev)) for i in range(40)])
    close(got.cpu().numpy(), want.cpu().numpy())
