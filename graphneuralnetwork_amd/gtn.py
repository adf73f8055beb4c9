"""Drop-in Graph Transformer Network (reference GTN/models/GTConv.py, GTLayer.py, GTN.py).

Same class names, constructor arguments, ``forward`` signatures, return values ``(y, Ws)`` and
state_dict keys as the reference. The input type decides the path; no threshold switches it:

* a dense ``[N, N, T]`` tensor ``A`` runs the reference's own arithmetic, op for op, on any
  device and in any dtype (its NaN behaviour included);
* an ``hetero.EdgeTypeGraph`` runs the sparse path: every matrix of the model is a set of
  VALUES ``[C, nnz]`` over a FIXED CSR pattern known beforehand (U, the union of the relations,
  and S_{l+1} = (S_l . U) > 0 from ``relation_product``), and the three graph operations are
  ``autograd.Function``s over csrc/gtn.hip: the masked sparse product, ``norm`` and the GCN
  aggregation, each with a hand-written adjoint that is again a masked product, a segment sum
  in stored order or an aggregation -- no float atomics and no ``index_add_`` anywhere, so a
  step's gradients are bit-identical from run to run.

Two defects of the reference, handled here:

(a) ``GTConv.weight`` is ``torch.Tensor(...)`` and never initialised. Here it is
    ``nn.init.constant_(weight, 0.1)``.
(b) When a node's off-diagonal column of H is empty, the reference's in-place
    ``deg_inv[deg_inv == inf] = 0`` after ``pow(-1)`` gives NaN gradients to every earlier
    layer's conv weights (0 * inf). The sparse path takes 1/0 -> 0 in the forward AND in the
    adjoint, so its gradients are finite; the dense path keeps the reference's behaviour.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .hetero import EdgeTypeGraph, Pattern


class SparseValues:
    """What travels between the layers of the sparse path: values [C, nnz] over a Pattern."""

    def __init__(self, pattern: Pattern, values: torch.Tensor):
        self.pattern, self.values = pattern, values


def _safe_inverse(d: torch.Tensor) -> torch.Tensor:
    """1 / d with 1 / 0 -> 0 (no inf is ever formed, so no 0 * inf in an adjoint)."""
    zero = d == 0
    return torch.where(zero, torch.zeros_like(d), 1.0 / torch.where(zero, torch.ones_like(d), d))


def _product(mode, pa: Pattern, av, pb: Pattern, bv, pp: Pattern):
    """``ops.masked_product`` over Patterns; an operand set is validated on its first use."""
    key = (mode, id(pa), id(pb))
    out = ops.masked_product(mode, pa.g, av, pb.g, bv, pp.g, validate=key not in pp.checked)
    pp.checked.add(key)
    return out


class _MaskedProduct(torch.autograd.Function):
    """out = (A . B) o P (mode 0) or (A . B^T) o P (mode 1) over fixed patterns. Both adjoints
    are again products masked to a known pattern, with the short operand the one walked."""

    @staticmethod
    def forward(ctx, av, bv, mode, pa, pb, pp):
        ctx.save_for_backward(av, bv)
        ctx.meta = (mode, pa, pb, pp)
        return _product(mode, pa, av, pb, bv, pp)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        av, bv = ctx.saved_tensors
        mode, pa, pb, pp = ctx.meta
        g = g.contiguous()
        da = db = None
        if mode == 0:    # A [n, k] walked, B [k, m] searched
            if ctx.needs_input_grad[0]:   # dA = (dOut . B^T) o pa: dOut searched, B walked
                da = _product(1, pp, g, pb, bv, pa)
            if ctx.needs_input_grad[1]:   # dB = (A^T . dOut) o pb: A^T walked, dOut searched
                db = _product(0, pa.T, av[:, pa.perm], pp, g, pb)
        else:            # A [n, k] searched, B [m, k] walked
            if ctx.needs_input_grad[0]:   # dA = (dOut . B) o pa: dOut searched, B^T walked
                da = _product(1, pp, g, pb.T, bv[:, pb.perm], pa)
            if ctx.needs_input_grad[1]:   # dB^T = (A^T . dOut) o pb^T, then back to pb's layout
                db = _product(0, pa.T, av[:, pa.perm], pp, g, pb.T)[:, pb.T.perm]
        return da, db, None, None, None, None


class _Norm(torch.autograd.Function):
    """The reference's ``norm(H, add=False)`` on values: y_e = x_e [row != col] / d[col_e] with
    d[j] the off-diagonal sum of column j (a segment sum over the column view in stored
    order) and 1/0 -> 0."""

    @staticmethod
    def forward(ctx, x, p):
        g, t = p.g, p.T.g
        d = ops.edge_rowsum(t, x[:, p.perm], skip_diag=True)            # [C, n]
        inv = _safe_inverse(d)
        scale = inv[:, g.col.to(torch.int64)] * ops._offdiag(g)         # [C, nnz]
        y = x * scale
        ctx.save_for_backward(y, scale)
        ctx.p = p
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        y, scale = ctx.saved_tensors
        p = ctx.p
        s = ops.edge_rowsum(p.T.g, (gy * y)[:, p.perm])                 # [C, n]
        return (gy - s[:, p.g.col.to(torch.int64)]) * scale, None


class _Aggregate(torch.autograd.Function):
    """The reference's ``gcn_conv`` for all channels at once, X W given:
    Y_c[j] = (sum_{i != j} H_c[i, j] XW[i] + XW[j]) / (1 + d_c[j]), over H's column view."""

    @staticmethod
    def forward(ctx, v, xw, p):
        t = p.T.g
        vt = v[:, p.perm].contiguous()
        z = ops.edge_aggregate(t, vt, xw, skip_diag=True)               # [C, n, F]
        inv = _safe_inverse(1.0 + ops.edge_rowsum(t, vt, skip_diag=True))
        z += xw
        ctx.save_for_backward(v, xw, z, inv)
        ctx.p = p
        return z * inv[:, :, None]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        v, xw, z, inv = ctx.saved_tensors
        p = ctx.p
        t = p.T.g
        gz = (gy * inv[:, :, None]).contiguous()                        # d(sum + XW)
        dv = dxw = None
        if ctx.needs_input_grad[0]:
            dd = -(gy * z).sum(-1) * inv * inv                          # d(1 + d), [C, n]
            dvt = ops.edge_dot(t, gz, xw, skip_diag=True) + \
                dd[:, ops._entry_rows(t)] * ops._offdiag(t)
            dv = dvt[:, p.T.perm]
        if ctx.needs_input_grad[1]:
            # the transpose of the column view is the pattern itself: per-channel inputs
            dxw = (ops.edge_aggregate(p.g, v.contiguous(), gz, skip_diag=True) + gz).sum(0)
        return dv, dxw, None


def _norm_dense(H, add):
    """The reference's dense ``norm`` (GTN/models/GTN.py:7-19), op for op."""
    n = H.shape[0]
    eye = torch.eye(n).type(torch.FloatTensor).to(H.device)
    off = (torch.eye(n) == 0).type(torch.FloatTensor).to(H.device)
    H = H.t()
    H = H * off + eye if add else H * off
    deg = torch.sum(H, dim=1)
    deg_inv = deg.pow(-1)
    deg_inv[deg_inv == float("inf")] = 0
    deg_inv = deg_inv * eye
    return torch.mm(deg_inv, H).t()


def norm(H, add=False):
    """``norm`` of the reference: each column of H divided by its off-diagonal sum (with
    ``add``: the diagonal set to 1 and counted). A dense H runs the reference's ops; a
    ``SparseValues`` runs the column sums over the cached column view (add=False)."""
    if isinstance(H, SparseValues):
        if add:
            raise ValueError("the sparse path folds norm(add=True) into the aggregation")
        return SparseValues(H.pattern, _Norm.apply(H.values, H.pattern))
    return _norm_dense(H, add)


class GTConv(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__(**kwargs)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 1, 1))
        self.bias = None
        self.scale = nn.Parameter(torch.Tensor([0.1]), requires_grad=False)
        nn.init.constant_(self.weight, 0.1)   # the reference leaves it uninitialised

    def forward(self, A, transposed: bool = False):
        w = F.softmax(self.weight, dim=1)
        if isinstance(A, EdgeTypeGraph):      # Q [C, nnz_U] (or Q^T over U's column view)
            return w[:, :, 0, 0] @ (A.tval_t if transposed else A.tval)
        return torch.sum(A * w, dim=1)


class GTLayer(nn.Module):
    def __init__(self, in_channels, out_channels, first=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.first = first
        self.conv1 = GTConv(in_channels, out_channels)
        if first:
            self.conv2 = GTConv(in_channels, out_channels)

    def forward(self, A, H_=None):
        sparse = isinstance(A, EdgeTypeGraph)
        if self.first:
            a, b = self.conv1(A), self.conv2(A)
            if sparse:       # H = Q1 . Q2 on S_2: Q1 walked, Q2 searched
                u, s2 = A.pattern, A.product_pattern(A.pattern)
                H = SparseValues(s2, _MaskedProduct.apply(a, b, 0, u, u, s2))
            else:
                H = torch.bmm(a, b)
            W = [F.softmax(self.conv1.weight, dim=1).detach(),
                 F.softmax(self.conv2.weight, dim=1).detach()]
        else:
            if sparse:       # H' = N . Q on S_{l+1}: N searched, Q^T walked
                nxt = A.product_pattern(H_.pattern)
                qt = self.conv1(A, transposed=True)
                H = SparseValues(nxt, _MaskedProduct.apply(H_.values, qt, 1, H_.pattern,
                                                           A.pattern.T, nxt))
            else:
                H = torch.bmm(H_, self.conv1(A))
            W = [F.softmax(self.conv1.weight, dim=1).detach()]
        return H, W


class GTN_Model(nn.Module):
    def __init__(self, num_edge, num_channels, w_in, w_out, num_class, num_layers, is_norm,
                 **kwargs):
        super().__init__(**kwargs)
        self.num_edge = num_edge
        self.num_channels = num_channels
        self.w_in = w_in
        self.w_out = w_out
        self.num_class = num_class
        self.num_layers = num_layers
        self.is_norm = is_norm
        self.layers = nn.ModuleList(GTLayer(num_edge, num_channels, first=i == 0)
                                    for i in range(num_layers))
        self.weight = nn.Parameter(torch.empty(w_in, w_out))
        self.bias = nn.Parameter(torch.empty(w_out))
        self.linear1 = nn.Linear(self.w_out * self.num_channels, self.w_out)
        self.linear2 = nn.Linear(self.w_out, self.num_class)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        nn.init.zeros_(self.bias)

    def gcn_conv(self, X, H):
        X = torch.mm(X, self.weight)
        if isinstance(H, SparseValues):       # all channels at once: [C, N, w_out]
            return _Aggregate.apply(H.values, X, H.pattern)
        return torch.mm(norm(H, add=True).t(), X)

    def normalization(self, H):
        if isinstance(H, SparseValues):
            return norm(H)
        return torch.stack([norm(H[i]) for i in range(self.num_channels)])

    def forward(self, A, X, target_x):
        sparse = isinstance(A, EdgeTypeGraph)
        if not sparse:
            A = A.unsqueeze(0).permute(0, 3, 1, 2)
        Ws = []
        H = None
        for i, layer in enumerate(self.layers):
            if i == 0:
                H, W = layer(A)
            else:
                H, W = layer(A, self.normalization(H))
            Ws.append(W)
        if sparse:
            Y = F.relu(self.gcn_conv(X, H))                       # [C, N, w_out]
            X_ = Y.permute(1, 0, 2).reshape(Y.shape[1], -1)       # channels side by side
        else:
            X_ = torch.cat([F.relu(self.gcn_conv(X, H[i])) for i in range(self.num_channels)],
                           dim=1)
        X_ = F.relu(self.linear1(X_))
        y = self.linear2(X_[target_x])
        return y, Ws
