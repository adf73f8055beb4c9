"""Drop-in GATNE modules (reference: GATNE_Pytorch/models/GATNE.py, train_utils/loss_utils.py,
train_utils/train_eval.py ValScale; the same model in GATNE/).

Same class names, constructor arguments, ``forward`` signatures, initialisation and state_dict
keys (``encoder.node_embeddings``, ``encoder.node_type_embeddings``, ``encoder.trans_weights``,
``encoder.trans_weights_s1``, ``encoder.trans_weights_s2``, ``decoder.weights``; with
``features``: ``encoder.embed_trans``, ``encoder.u_embed_trans``).

The reference gathers a whole weight matrix per batch row (``trans_weights[node_types]`` is
[B, U, E]) and multiplies with batched matmuls. Here the rows are sorted by edge type on the
device and go through the matrix cores in tiles of 16 rows of one type (csrc/gatne.hip):

  row gather (``ops.gather_rows``) -> typed neighbour sum (``ops.typed_gather_sum``) ->
  edge-type attention (``ops.gatne_attend_forward``: scores, softmax over the types, weighted
  sum, the type's transform, L2 normalisation) -> the score head (``graphsage._SageScoreFn``)

with device adjoints: the attention's (``ops.gatne_attend_backward``) and, for the three gathers,
the stable transpose + fixed-order scatter of csrc/sage_bwd.hip (``ops.sage_scatter_agg`` with
``scale=``). Every sum has a fixed order: gradients are bit-identical from run to run.

``GATNE_FUSED`` off, CPU tensors, other dtypes, widths outside ``ops.gatne_supported``, a module
with forward hooks, or ``features`` that require a gradient run the fallback: the reference's
arithmetic, op for op, in PyTorch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import graphsage, ops

# the kernels of csrc/gatne.hip (GraphEncoder.forward, GraphDecoder.forward). No row threshold:
# measured against the torch lines from B = 16 to 8192, the kernels win at every size with block
# ranges apart (tools/gatne_ab.py)
GATNE_FUSED = True
# True: an id or edge type out of range raises IndexError (one host read per gather, as
# ops.sage_gather_aggregate); False: no host read in a step -- such an id is skipped by the
# kernels, such a type gives NaN rows (the reference trips a device-side assert)
CHECK_INDICES = False


def _hooked(m: nn.Module) -> bool:
    return bool(m._forward_hooks or m._forward_pre_hooks)


def _f32_dev(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


class _GatherRowsFn(torch.autograd.Function):
    """table[idx] for a float32 [N, F] table (``ops.gather_rows``); the gradient of the table is
    the fixed-order scatter over the transposed index map (k = 1, scale 1): rows nobody drew
    are zeros, a row drawn many times is summed in batch order."""

    @staticmethod
    def forward(ctx, table, idx, check):
        idx = idx.reshape(-1).to(torch.int64)
        ctx.save_for_backward(idx)
        ctx.n = table.shape[0]
        # unchecked, the kernel skips an id out of range: its row stays the zeros given here
        out = None if check else torch.zeros((idx.numel(), table.shape[1]), dtype=table.dtype,
                                             device=table.device)
        return ops.gather_rows(table, idx, out=out, check=check)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        tr = ops.sage_maps_transpose_nbr(idx.view(-1, 1), ctx.n, check=False)
        d = None if tr is None else ops.sage_scatter_agg(g.contiguous(), tr, ctx.n, scale=1.0)
        if d is None:
            raise RuntimeError("the scatter refused a width the module reports as covered")
        return d, None, None


class _TypedGatherFn(torch.autograd.Function):
    """``ops.typed_gather_sum`` of a float32 table [N, T, W] (differentiable) or [N, W] (a
    feature table: no gradient). The gradient of a typed table is the scatter of du viewed as
    [B T, W] over the ids nbr T + t of the table viewed as [N T, W], scale 1 (SUM) or 1 / K."""

    @staticmethod
    def forward(ctx, table, nbr, agg_func, check):
        ctx.save_for_backward(nbr)
        ctx.shape = tuple(table.shape)
        ctx.scale = 1.0 if agg_func == "SUM" else 1.0 / nbr.shape[2]
        return ops.typed_gather_sum(table, nbr, agg_func, check=check)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        (nbr,) = ctx.saved_tensors
        N, T, W = ctx.shape
        B, _, K = nbr.shape
        ids = (nbr * T + torch.arange(T, device=nbr.device).view(1, T, 1)).view(B * T, K)
        tr = ops.sage_maps_transpose_nbr(ids, N * T, check=False)
        d = None if tr is None else ops.sage_scatter_agg(g.contiguous().view(B * T, W), tr, N * T,
                                                        scale=ctx.scale)
        if d is None:
            raise RuntimeError("the scatter refused a width the module reports as covered")
        return d.view(N, T, W), None, None, None


class _AttendFn(torch.autograd.Function):
    """The edge-type attention stage on the device (``ops.gatne_attend_forward`` /
    ``ops.gatne_attend_backward``), differentiable in c, u and the three weights; saves alpha
    [B, T] and 1 / max(|e|, eps) [B], recomputes the tanh; once-differentiable."""

    @staticmethod
    def forward(ctx, c, u, w1, w2, m, types, check):
        order = ops.gatne_order(types, w1.shape[0], check=check)
        out, alpha, inv = ops.gatne_attend_forward(c, u, w1, w2, m, order)
        ctx.save_for_backward(u, w1, w2, m, out, alpha, inv, order.perm, order.seg)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        u, w1, w2, m, out, alpha, inv, perm, seg = ctx.saved_tensors
        need = ctx.needs_input_grad
        dc, du, dw1, dw2, dm = ops.gatne_attend_backward(
            g, out, u, alpha, inv, w1, w2, m, ops.GatneOrder(perm, seg, w1.shape[0]),
            need_du=need[1], need_params=any(need[2:5]))
        return (dc if need[0] else None, du, dw1 if need[2] else None,
                dw2.view_as(w2) if need[3] else None, dm if need[4] else None, None, None)


class GraphEncoder(nn.Module):
    """GATNE_Pytorch/models/GATNE.py:6-97."""

    def __init__(self, num_nodes, embedding_size, embedding_u_size, edge_type_count,
                 attention_size, features, agg_func='SUM', **kwargs):
        super().__init__(**kwargs)
        self.num_nodes = num_nodes
        self.embedding_size = embedding_size
        self.embedding_u_size = embedding_u_size
        self.edge_type_count = edge_type_count
        self.dim_a = attention_size
        self.agg_func = agg_func
        self.features = None
        if features is not None:
            self.features = features
            self.feature_dim = self.features.shape[-1]
            self.embed_trans = nn.Parameter(torch.empty(self.feature_dim, embedding_size))
            self.u_embed_trans = nn.Parameter(
                torch.empty(edge_type_count, self.feature_dim, embedding_u_size))
        else:
            self.node_embeddings = nn.Parameter(torch.empty(num_nodes, embedding_size))
            self.node_type_embeddings = nn.Parameter(
                torch.empty(num_nodes, edge_type_count, embedding_u_size))
        self.trans_weights = nn.Parameter(
            torch.empty(edge_type_count, embedding_u_size, embedding_size))
        self.trans_weights_s1 = nn.Parameter(
            torch.empty(edge_type_count, embedding_u_size, attention_size))
        self.trans_weights_s2 = nn.Parameter(torch.empty(edge_type_count, attention_size, 1))
        self.reset_parameters()

    def reset_parameters(self):
        if self.features is not None:
            nn.init.xavier_uniform_(self.embed_trans.data)
            nn.init.xavier_uniform_(self.u_embed_trans.data)
        else:
            nn.init.uniform_(self.node_embeddings.data)
            nn.init.uniform_(self.node_type_embeddings.data)
        nn.init.xavier_uniform_(self.trans_weights.data)
        nn.init.xavier_uniform_(self.trans_weights_s1.data)
        nn.init.xavier_uniform_(self.trans_weights_s2.data)

    # ------------------------------------------------------------------ the two paths
    def _fused_ok(self, inputs, node_types, node_neigh) -> bool:
        if not (GATNE_FUSED and not _hooked(self) and self.agg_func in ("SUM", "MEAN")
                and all(torch.is_tensor(t) and t.is_cuda for t in (inputs, node_types, node_neigh))
                and inputs.dim() == 1 and node_types.dim() == 1 and node_neigh.dim() == 3):
            return False
        B, T, K = node_neigh.shape
        if (B == 0 or K == 0 or T != self.edge_type_count or inputs.numel() != B
                or node_types.numel() != B):
            return False
        if not _f32_dev(*self.parameters()):
            return False
        if self.features is not None and not (
                torch.is_tensor(self.features) and _f32_dev(self.features)
                and self.features.dim() == 2 and not self.features.requires_grad
                and self.feature_dim % 4 == 0):
            return False
        return ops.gatne_supported(self.embedding_size, self.embedding_u_size, self.dim_a, T)

    def _fallback(self, inputs, node_types, node_neigh):
        """The reference's expression (GATNE.py:57-97)."""
        T = self.edge_type_count
        if self.features is None:
            centre = self.node_embeddings[inputs]
            per_type = [self.node_type_embeddings[:, t, :][node_neigh[:, t, :]].unsqueeze(1)
                        for t in range(T)]
            neigh = torch.cat(per_type, dim=1)                               # [B, T, K, U]
        else:
            centre = torch.mm(self.features[inputs], self.embed_trans)
            rows = self.features[node_neigh].permute(1, 0, 2, 3).reshape(T, -1, self.feature_dim)
            neigh = torch.bmm(rows, self.u_embed_trans).reshape(
                T, -1, node_neigh.shape[-1], self.embedding_u_size).permute(1, 0, 2, 3)
        if self.agg_func == 'SUM':
            u = torch.sum(neigh, dim=2)
        elif self.agg_func == 'MEAN':
            u = torch.mean(neigh, dim=2)
        else:
            raise ValueError("please choice else aggregator!")
        m = self.trans_weights[node_types]                                   # [B, U, E]
        w1 = self.trans_weights_s1[node_types]                               # [B, U, A]
        w2 = self.trans_weights_s2[node_types]                               # [B, A, 1]
        scores = torch.matmul(torch.tanh(torch.matmul(u, w1)), w2).squeeze(2)
        alpha = F.softmax(scores, dim=1).unsqueeze(1)                        # [B, 1, T]
        v = torch.matmul(alpha, u)                                           # [B, 1, U]
        e = centre + torch.matmul(v, m).squeeze(1)
        return F.normalize(e, dim=1)

    def _fused(self, inputs, node_types, node_neigh):
        check = CHECK_INDICES
        node_neigh = node_neigh.to(torch.int64)
        if self.features is None:
            centre = _GatherRowsFn.apply(self.node_embeddings, inputs, check)
            u = _TypedGatherFn.apply(self.node_type_embeddings, node_neigh, self.agg_func, check)
        else:
            centre = torch.mm(ops.gather_rows(self.features, inputs, check=check),
                              self.embed_trans)
            # sum_k (features[nbr] W_t) = (sum_k features[nbr]) W_t: K times fewer GEMM rows
            s = _TypedGatherFn.apply(self.features, node_neigh, self.agg_func, check)
            u = torch.bmm(s.transpose(0, 1), self.u_embed_trans).transpose(0, 1).contiguous()
        return _AttendFn.apply(centre, u, self.trans_weights_s1, self.trans_weights_s2,
                               self.trans_weights, node_types, check)

    def forward(self, inputs, node_types, node_neigh):
        if self._fused_ok(inputs, node_types, node_neigh):
            return self._fused(inputs, node_types, node_neigh)
        return self._fallback(inputs, node_types, node_neigh)

    @torch.no_grad()
    def embed_all_types(self, neighbors, chunk: int = 4096) -> torch.Tensor:
        """[N, T, E]: every node under every edge type, as ValScale.get_model's per-node calls
        ``encoder([i] * T, [0 .. T-1], [neighbors[i]] * T)`` give them, in chunks of ``chunk``
        nodes (chunk T rows per call). neighbors: [N, T, K] (a tensor or nested lists)."""
        dev = self.trans_weights.device
        neighbors = torch.as_tensor(neighbors).to(dev)
        N, T = neighbors.shape[0], self.edge_type_count
        out = torch.empty((N, T, self.embedding_size), dtype=self.trans_weights.dtype, device=dev)
        types = torch.arange(T, device=dev)
        for lo in range(0, N, max(int(chunk), 1)):
            ids = torch.arange(lo, min(lo + max(int(chunk), 1), N), device=dev)
            emb = self(ids.repeat_interleave(T), types.repeat(ids.numel()),
                       neighbors[ids].repeat_interleave(T, dim=0))
            out[ids] = emb.view(ids.numel(), T, -1)
        return out


class GraphDecoder(nn.Module):
    """GATNE_Pytorch/models/GATNE.py:100-114."""

    def __init__(self, num_nodes, embedding_size, **kwargs):
        super().__init__(**kwargs)
        self.num_nodes = num_nodes
        self.embedding_size = embedding_size
        self.weights = nn.Parameter(torch.empty(num_nodes, embedding_size))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weights.data)

    def _fused_ok(self, embed, contest_negative) -> bool:
        return (GATNE_FUSED and not _hooked(self) and torch.is_tensor(embed)
                and torch.is_tensor(contest_negative) and contest_negative.is_cuda
                and _f32_dev(embed, self.weights) and embed.dim() == 2
                and contest_negative.dim() == 2 and contest_negative.shape[0] == embed.shape[0]
                and embed.shape[0] > 0 and contest_negative.shape[1] > 0
                and embed.shape[1] == self.embedding_size
                and ops.sage_scatter_supported(self.embedding_size))

    def forward(self, embed, contest_negative):
        if self._fused_ok(embed, contest_negative):
            B, S = contest_negative.shape
            second = _GatherRowsFn.apply(self.weights, contest_negative, CHECK_INDICES)
            second = second.view(B, S, self.embedding_size)
            if graphsage._score_fused_ok(embed, second):
                return graphsage._SageScoreFn.apply(embed, second).squeeze(1)
            return torch.bmm(embed.unsqueeze(1), second.permute(0, 2, 1)).squeeze(1)
        return torch.bmm(embed.unsqueeze(1),
                         self.weights[contest_negative].permute(0, 2, 1)).squeeze(1)


class GATNEModel(nn.Module):
    """GATNE_Pytorch/models/GATNE.py:117-127."""

    def __init__(self, num_nodes, embedding_size, embedding_u_size, edge_type_count,
                 attention_size, features, **kwargs):
        super().__init__()
        self.encoder = GraphEncoder(num_nodes, embedding_size, embedding_u_size, edge_type_count,
                                    attention_size, features, **kwargs)
        self.decoder = GraphDecoder(num_nodes, embedding_size)

    def forward(self, inputs, node_types, node_neigh, context_negative):
        return self.decoder(self.encoder(inputs, node_types, node_neigh), context_negative)


class SigmoidBCELoss(nn.Module):
    """GATNE_Pytorch/train_utils/loss_utils.py: the masked per-row mean of the BCE with logits."""

    def forward(self, inputs, target, mask=None):
        out = F.binary_cross_entropy_with_logits(inputs, target, weight=mask, reduction="none")
        return out.mean(dim=1)


class ValScale:
    """GATNE_Pytorch/train_utils/train_eval.py:47-85 with ``get_model`` on
    ``GraphEncoder.embed_all_types`` (chunked batches) instead of one encoder call per node.
    ``val_eval`` scores with the training script's own ``evaluate`` (given, or imported from
    ``train_utils.train_eval`` as run.py has it on its path)."""

    def __init__(self, num_nodes, edge_types, edge_type_count, neighbors, vocab, chunk=4096):
        self.num_nodes = num_nodes
        self.edge_types = edge_types
        self.edge_type_count = edge_type_count
        self.neighbors = neighbors
        self.vocab = vocab
        self.chunk = chunk

    def get_model(self, model, device):
        nbr = torch.as_tensor(self.neighbors)[:self.num_nodes].to(device)
        emb = model.encoder.embed_all_types(nbr, chunk=self.chunk).cpu().numpy()
        final_model = {t: {} for t in self.edge_types[:self.edge_type_count]}
        for i in range(self.num_nodes):
            token = self.vocab.to_tokens(i)
            for j in range(self.edge_type_count):
                final_model[self.edge_types[j]][token] = emb[i, j]
        return final_model

    def val_eval(self, model, device, valid_true_data_by_edge, valid_false_data_by_edge, args,
                 evaluate=None):
        if evaluate is None:
            from train_utils.train_eval import evaluate      # the training script's scorer
        final_model = self.get_model(model, device)
        scores = []
        for i in range(self.edge_type_count):
            name = self.edge_types[i]
            if args.eval_type == "all" or name in args.eval_type.split(","):
                scores.append([float(v) for v in evaluate(
                    final_model[name], valid_true_data_by_edge[name],
                    valid_false_data_by_edge[name])])
        loss, acc, f1, rcl = (sum(col) / len(col) for col in zip(*scores))
        return loss, acc, f1, rcl
