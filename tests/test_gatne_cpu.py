"""The drop-in GATNE modules (graphneuralnetwork_amd.gatne) on CPU tensors -- the fallback path,
the reference's arithmetic in PyTorch -- against tests/golden/gatne.npz, which the REFERENCE model
wrote (tests/golden/make_gatne_golden.py): state_dict keys and shapes, ``pred``, the encoder
output and every parameter gradient after the training loop's loss line, for widths (32, 16, 16)
and (64, 32, 16), SUM and MEAN, with and without ``features``. Row 5 of the batch has e = 0
exactly. Bounds: the project's fp32 bounds, rtol 1e-4 and atol 2e-5 max|ref|."""
import numpy as np
import pytest
import torch

CASES = [(w, f, agg) for w in (0, 1) for f in (0, 1) for agg in ("SUM", "MEAN")]


def close(a, b, rtol=1e-4):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-5 * scale)


def build_model(g, w, f, agg, device="cpu", dtype=torch.float32):
    """The module with the fixture's parameters of case (w, f), and the fixture's batch."""
    from graphneuralnetwork_amd import gatne
    N, T = int(g["dims"][0]), int(g["dims"][1])
    E, U, A = (int(v) for v in g["widths"][w])
    feats = torch.from_numpy(g["features"]).to(device=device, dtype=dtype) if f else None
    model = gatne.GATNEModel(N, E, U, T, A, feats, agg_func=agg)
    tag = f"w{w}_f{f}"
    state = {k: torch.from_numpy(g[f"{tag}_param_{k}"]) for k in g[f"{tag}_keys"]}
    model.load_state_dict(state, strict=True)
    model = model.to(device=device, dtype=dtype)
    batch = [torch.from_numpy(g[k]).to(device) for k in ("centres", "types", "nbr", "ctx", "masks",
                                                       "labels")]
    return model, batch


def train_loss(model, batch):
    """(encoder output, pred, the loss of train_utils/train_eval.py:119-120 summed)."""
    from graphneuralnetwork_amd.gatne import SigmoidBCELoss
    c, ty, nb, cx, mk, lb = batch
    mk, lb = mk.to(model.decoder.weights.dtype), lb.to(model.decoder.weights.dtype)
    enc = model.encoder(c, ty, nb)
    pred = model.decoder(enc, cx)
    loss = SigmoidBCELoss()(pred, lb, mk) / mk.sum(axis=1) * mk.shape[1]
    return enc, pred, loss.sum()


@pytest.mark.parametrize("w,f", [(w, f) for w in (0, 1) for f in (0, 1)])
def test_state_dict_keys_and_shapes(golden, w, f):
    from graphneuralnetwork_amd import gatne
    g = golden("gatne")
    N, T = int(g["dims"][0]), int(g["dims"][1])
    E, U, A = (int(v) for v in g["widths"][w])
    model = gatne.GATNEModel(N, E, U, T, A, torch.from_numpy(g["features"]) if f else None)
    sd = model.state_dict()
    keys = [str(k) for k in g[f"w{w}_f{f}_keys"]]
    assert list(sd) == keys
    want = ({"encoder.embed_trans", "encoder.u_embed_trans"} if f else
            {"encoder.node_embeddings", "encoder.node_type_embeddings"})
    assert set(keys) == want | {"encoder.trans_weights", "encoder.trans_weights_s1",
                                "encoder.trans_weights_s2", "decoder.weights"}
    for k in keys:
        assert tuple(sd[k].shape) == g[f"w{w}_f{f}_param_{k}"].shape, k
        assert torch.isfinite(sd[k]).all(), k      # initialised, as the reference's reset_parameters


@pytest.mark.parametrize("w,f,agg", CASES)
def test_fallback_reproduces_the_reference(golden, w, f, agg):
    g = golden("gatne")
    model, batch = build_model(g, w, f, agg)
    enc, pred, loss = train_loss(model, batch)
    loss.backward()
    case = f"w{w}_f{f}_{agg}"
    assert float(enc[5].detach().abs().max()) == 0.0        # the e = 0 row: F.normalize gives 0
    close(enc.detach().numpy(), g[f"{case}_enc"])
    close(pred.detach().numpy(), g[f"{case}_pred"])
    for name, p in model.named_parameters():
        close(p.grad.numpy(), g[f"{case}_grad_{name}"])


@pytest.mark.parametrize("f", [0, 1])
def test_embed_all_types_equals_the_per_node_loop(golden, f):
    g = golden("gatne")
    model, _ = build_model(g, 0, f, "SUM")
    N, T, K = (int(v) for v in g["dims"][:3])
    nbr = torch.randint(0, N, (N, T, K))
    got = model.encoder.embed_all_types(nbr, chunk=10)      # 97 nodes: a short last chunk
    assert got.shape == (N, T, model.encoder.embedding_size)
    with torch.no_grad():
        for i in range(N):
            want = model.encoder(torch.tensor([i] * T), torch.arange(T),
                                 torch.stack([nbr[i]] * T))
            assert torch.equal(got[i], want), i


def test_valscale_returns_the_dict_of_dicts(golden):
    from graphneuralnetwork_amd import gatne
    g = golden("gatne")
    model, _ = build_model(g, 0, 0, "SUM")
    N, T, K = (int(v) for v in g["dims"][:3])
    nbr = torch.randint(0, N, (N, T, K))

    class Vocab:
        def to_tokens(self, i):
            return f"n{i}"

    names = ["a", "b", "c"]
    vs = gatne.ValScale(N, names, T, nbr.tolist(), Vocab(), chunk=16)
    fm = vs.get_model(model, torch.device("cpu"))
    assert list(fm) == names and all(len(fm[n]) == N for n in names)
    with torch.no_grad():
        want = model.encoder(torch.tensor([11] * T), torch.arange(T), torch.stack([nbr[11]] * T))
    for j, n in enumerate(names):
        assert isinstance(fm[n]["n11"], np.ndarray)
        assert np.array_equal(fm[n]["n11"], want[j].numpy())


def test_sigmoid_bce_loss_is_the_masked_row_mean():
    from graphneuralnetwork_amd.gatne import SigmoidBCELoss
    z, y = torch.randn(5, 7), (torch.rand(5, 7) < 0.3).float()
    m = (torch.rand(5, 7) < 0.6).float()
    want = (m * (torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs())))).mean(1)
    assert torch.allclose(SigmoidBCELoss()(z, y, m), want, atol=1e-6)


NEW_ENTRIES = ("gnn_typed_gather_sum_f32", "gnn_gatne_order_workspace_bytes", "gnn_gatne_order",
               "gnn_gatne_supported", "gnn_gatne_attend_workspace_bytes",
               "gnn_gatne_attend_fwd_f32", "gnn_gatne_attend_bwd_f32",
               "gnn_sage_scatter_agg_scaled_f32")


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_header_declares_and_the_library_binds(name):
    from graphneuralnetwork_amd import _lib
    assert name in _lib.SIGNATURES and name in _lib.PARAMS
    lib = _lib.load(build_if_missing=True)
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]


def test_supported_set():
    from graphneuralnetwork_amd import _lib
    lib = _lib.load(build_if_missing=True)
    ok = lambda E, U, A, T: bool(lib.gnn_gatne_supported(E, U, A, T))  # noqa: E731
    assert ok(256, 128, 128, 2)                                  # run.py's defaults
    assert all(ok(E, U, A, T) for E in (16, 32, 64, 128, 256) for U in (16, 32, 64, 128)
               for A in (16, 32, 64, 128) for T in (1, 8))
    assert not any(ok(*s) for s in ((512, 128, 128, 2), (8, 16, 16, 1), (48, 16, 16, 1),
                                    (32, 24, 16, 2), (32, 16, 256, 2), (32, 16, 16, 0),
                                    (32, 16, 16, 9)))


def test_scaled_scatter_signature_carries_the_scale():
    from graphneuralnetwork_amd import _lib
    base, scaled = (_lib.PARAMS[n] for n in ("gnn_sage_scatter_agg_f32",
                                             "gnn_sage_scatter_agg_scaled_f32"))
    assert [p for p in scaled if p != "scale"] == list(base)
    import ctypes
    assert _lib.SIGNATURES["gnn_sage_scatter_agg_scaled_f32"][1][scaled.index("scale")] \
        is ctypes.c_float


def test_short_workspace_and_bad_widths_are_refused_on_the_host():
    """The entries check their arguments before anything reaches the device: host buffers stand
    in for the device pointers, which are never dereferenced."""
    import ctypes
    from graphneuralnetwork_amd import _lib
    lib = _lib.load(build_if_missing=True)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    need = lib.gnn_gatne_order_workspace_bytes(5, 3)
    assert need > 0
    assert lib.gnn_gatne_order(p, 5, 3, p, p, p, p, need - 1, None) == _lib.E_ARG
    assert lib.gnn_gatne_order_workspace_bytes(5, 9) == _lib.E_UNSUPPORTED
    need = lib.gnn_gatne_attend_workspace_bytes(5, 3, 32, 16, 16)
    assert need > 0
    args = (p, 32, p, 32, p, p, p, p, p, 5, 3, 32, 16, 16, p, p, p, p, p, p, p, p, p)
    assert lib.gnn_gatne_attend_bwd_f32(*args, need - 1, None) == _lib.E_ARG
    assert lib.gnn_gatne_attend_workspace_bytes(5, 3, 32, 24, 16) == _lib.E_UNSUPPORTED
    assert lib.gnn_gatne_attend_fwd_f32(p, 32, p, p, p, 5, 3, 32, 24, 16, p, p, p, p, 32, p, p,
                                        None) == _lib.E_UNSUPPORTED
    assert lib.gnn_gatne_attend_fwd_f32(p, 16, p, p, p, 5, 3, 32, 16, 16, p, p, p, p, 32, p, p,
                                        None) == _lib.E_ARG            # ldc < E
    assert lib.gnn_typed_gather_sum_f32(p, 16, 16, 4, p, 2, 2, 3, 16, 1.0, p, 16, p,
                                        None) == _lib.E_ARG            # ld_n < (T - 1) ld_t + W
    assert lib.gnn_typed_gather_sum_f32(p, 32, 16, 4, p, 2, 2, 3, 6, 1.0, p, 16, p,
                                        None) == _lib.E_UNSUPPORTED    # W not a multiple of 4
    assert bytes(buf) == bytes(4096)
