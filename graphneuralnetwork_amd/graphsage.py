"""Drop-in GraphSAGE modules (reference: GraphSAGE/GraphSAGE.py, GraphSAGE/graph_utils.py).

Same names, constructor arguments, 9-argument ``forward`` and state_dict keys
(``sage_blocks.sage_layer{i}.weight.weight`` [H, 2F or F], ``dense.weight`` /
``dense.bias``) as the reference.

Hot path on gfx950:

* ``Aggregator`` (graph_utils.py:4-11) -> one HIP launch (mean, or torch.argmax's
  int64 first-max indices, bit-exact; plus 'MAXPOOL', the value max-pool of the north star);
* the re-gathers of GraphSAGE.py:47-49 (``torch.embedding(feats, map)`` followed
  by the next layer's ``Aggregator``) -> ONE fused gather-aggregate launch that
  never materialises the [M, k, H] neighbour tensor, plus one row-gather
  launch for the centre rows;
* ``SageLayer``'s ``Linear(cat[self, agg])`` -> two accumulating MFMA GEMMs on
  the two halves of W (no concatenated copy);
* training on the device sampler's batches (``l.backward()``, train_eval.py:112-119) -> one
  autograd function per MEAN layer (``_SageTrainLayerFn``): the inference launches forward,
  the weight gradient in one masked pass and the concat gather's adjoint on the device
  (``csrc/sage_bwd.hip``) backward; per MAXPOOL layer ``_SageMaxPoolTrainLayerFn``: the concat
  gather records the winning neighbour as one byte per (row, feature), the adjoint sums the
  gradient through that mask in a fixed order (no ``index_put_``, no float atomics);
* ``gcn=True`` (``relu(W . agg)``, the sampler's maps holding each node among its neighbours):
  the same over the aggregate alone -- inference as one gather-aggregate into an [M, F] buffer
  plus the MFMA GEMM (a pending batch stays pending), training as ``_SageGcnTrainLayerFn``
  with the adjoint of the gcn gather on the device (``SAGE_GCN_FUSED``);
* the unsupervised head (GraphSAGE.py:61 ``torch.bmm`` over a permuted operand, and the loop's
  ``binary_cross_entropy_with_logits``, train_eval.py:113-114) -> ``_SageScoreFn`` and
  ``unsupervised_loss`` over ``csrc/sage_score.hip``: the second tower's gradient written in its
  own [B S, H] layout, fixed-order sums, no float atomics (``SAGE_SCORE_FUSED``).
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from .graph import from_coo
from .ops import (_bce_takes, _bf16_inference_only, _masked_grad, _score_takes,
                  _transform_or_mm, bce_logits, gather_rows, gcn_transform, gemm_tn_masked,
                  linear_relu_classify, sage_aggregate, sage_gather_aggregate,
                  sage_gather_aggregate_arg, sage_gather_concat, sage_gather_concat_arg,
                  sage_layer, sage_maps_transpose, sage_maps_transpose_nbr, sage_scatter_agg,
                  sage_scatter_agg_maxpool, sage_scatter_concat, sage_scatter_concat_maxpool,
                  sage_score, sage_score_backward, sage_train_layer_supported, spmm_forward)

# the inference SageLayer GEMM relu([self | agg] @ W^T) runs on the hand-written MFMA kernel
# (gnn_linear_relu_f32). With the split-bf16 arithmetic (the default, ops.set_transform_precision)
# it beats hipBLASLt at every size (K=256, N=128, tools/transform_prec_ab.py,
# profiles/r03w_transform_prec_ab.log: 8192 rows 11.0 vs 19.9 us, 61771 rows 32.6 vs 40.1,
# 200000 rows 90.2 vs 136.5); on the fp32-MFMA arithmetic it ran up to SAGE_MFMA_MAX_SMALL rows and
# from SAGE_MFMA_MIN_LARGE rows up, hipBLASLt in between (62479 rows 46.8 vs 41.0 us,
# profiles/r03f_gemm_ab.log).
SAGE_MFMA_MAX_SMALL = 16384
SAGE_MFMA_MIN_LARGE = 131072


def _sage_gemm_on_mfma(rows: int) -> bool:
    from .ops import transform_precision
    if transform_precision() == "split-bf16":
        return True
    return rows <= SAGE_MFMA_MAX_SMALL or rows >= SAGE_MFMA_MIN_LARGE


class Gathered(NamedTuple):
    """A feature tensor given as (table, index): ``table[index]`` without materialising it.

    Accepted by ``GraphSAGE.forward`` in place of the pre-gathered
    ``center_feats_data`` ([M] index) / ``center_neigh_feats_data`` ([M, k] index)
    the reference's collate_fn builds with torch.embedding
    (GraphSAGE/data_utils.py:161-162); see ``sampler.sample_batch``.
    ``trusted``: the indices are known to be in range (built by the device
    sampler), so the gather skips its index check and the host sync it costs.
    ``live``: a device int64 scalar -- only ``index[:live]`` is real (a batch from
    ``sample_batch(..., sync=False)``, whose sizes the host never read; ``index`` is then
    the buffer at its capacity). The fused inference layer runs on it as it is; any other
    path reads the count back and slices.
    """
    table: torch.Tensor
    index: torch.Tensor
    trusted: bool = False
    live: torch.Tensor | None = None


def _trim(g):
    """A Gathered with a device row count as an ordinary one (one host read)."""
    if not isinstance(g, Gathered) or g.live is None:
        return g
    return Gathered(g.table, g.index[:int(g.live.item())], g.trusted)


def trust_map(t: torch.Tensor) -> torch.Tensor:
    """Mark an index map as -1-free and in range (the device sampler's maps): the
    forward then skips the reference's ``map != -1`` filtering and the index check,
    i.e. every host synchronisation."""
    t._gnn_trusted = True
    return t


def _trusted(t) -> bool:
    return bool(getattr(t, "_gnn_trusted", False))


def _scatter_rows(g: torch.Tensor, idx: torch.Tensor, n: int, scale: float) -> torch.Tensor:
    """out[t] = scale * sum of g[m] over the (m, j) with idx[m, j] == t  (the adjoint of a
    row gather), as the HIP SpMM over the transposed index map: deterministic, no atomics.
    ``idx`` was bounds-checked by the forward gather."""
    M = idx.shape[0]
    k = idx.numel() // max(M, 1)
    rows = idx.reshape(-1)
    cols = torch.arange(M, device=idx.device, dtype=torch.int64).repeat_interleave(k)
    at = from_coo(rows, cols, torch.full((rows.numel(),), scale, dtype=torch.float32,
                                         device=idx.device), n, M, check=False)
    return spmm_forward(at, g.contiguous())


class _MeanAgg(torch.autograd.Function):
    """Pre-gathered MEAN / SUM with autograd (d neigh = d out (/ k) broadcast over k)."""

    @staticmethod
    def forward(ctx, neigh, kind="MEAN"):
        ctx.k = neigh.shape[1]
        ctx.kind = kind
        return sage_aggregate(neigh, kind)

    @staticmethod
    def backward(ctx, g):
        g = g / ctx.k if ctx.kind == "MEAN" else g
        return g.unsqueeze(1).expand(-1, ctx.k, -1), None


class _GatherMeanAgg(torch.autograd.Function):
    """Fused gather + MEAN / SUM with autograd w.r.t. the table (scatter of d out (/ k))."""

    @staticmethod
    def forward(ctx, table, idx, kind="MEAN", check=True):
        ctx.save_for_backward(idx)
        ctx.n = table.shape[0]
        ctx.kind = kind
        return sage_gather_aggregate(table, idx, kind, check=check)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        scale = 1.0 / idx.shape[1] if ctx.kind == "MEAN" else 1.0
        return _scatter_rows(g, idx, ctx.n, scale), None, None, None


class _MaxPoolAgg(torch.autograd.Function):
    """Value max-pool over a pre-gathered [M, k, F] tensor with autograd: the gradient goes
    to the first maximal neighbour of every (row, feature) -- the argmax kernel's index."""

    @staticmethod
    def forward(ctx, neigh):
        arg = sage_aggregate(neigh, "MAX")
        ctx.save_for_backward(arg)
        ctx.k = neigh.shape[1]
        return sage_aggregate(neigh, "MAXPOOL")

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        M, F = g.shape
        out = torch.zeros((M, ctx.k, F), dtype=g.dtype, device=g.device)
        return out.scatter_(1, arg.unsqueeze(1), g.unsqueeze(1))


class _GatherMaxPoolAgg(torch.autograd.Function):
    """Fused gather + value max-pool with autograd w.r.t. the table (the gradient of each
    (row, feature) lands on the table row of its first maximal neighbour)."""

    @staticmethod
    def forward(ctx, table, idx, check=True):
        arg = sage_gather_aggregate(table, idx, "MAX", check=check)
        ctx.save_for_backward(idx, arg)
        ctx.n = table.shape[0]
        return sage_gather_aggregate(table, idx, "MAXPOOL", check=False)

    @staticmethod
    def backward(ctx, g):
        idx, arg = ctx.saved_tensors
        rows = idx.to(torch.int64).gather(1, arg)                     # [M, F] table rows
        cols = torch.arange(g.shape[1], device=g.device).expand_as(rows)
        out = torch.zeros((ctx.n, g.shape[1]), dtype=g.dtype, device=g.device)
        return out.index_put_((rows, cols), g, accumulate=True), None, None


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, check=True):
        ctx.save_for_backward(idx)
        ctx.n = x.shape[0]
        return gather_rows(x, idx, check=check)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return _scatter_rows(g, idx.reshape(-1, 1), ctx.n, 1.0), None, None


def Aggregator(neigh_feat, agg_func='MEAN'):
    """GraphSAGE/graph_utils.py:4-11 on the device ('MEAN' -> fp32, 'MAX' -> int64 argmax).

    Extension beyond the reference: 'MAXPOOL' -> the fp32 value max-pool the north star
    names (torch.max(neigh_feat, dim=1).values); the reference's own names keep their
    meaning, and any other name prints and raises as the reference does."""
    if agg_func not in ('MEAN', 'MAX', 'MAXPOOL'):
        print('请选择合适的聚合函数')  # the reference prints this, then a bare raise
        raise RuntimeError("No active exception to reraise")
    return reduce_neighbors(neigh_feat, agg_func)


def _gather_aggregate(table, idx, agg_func, trusted=False):
    _bf16_inference_only(table, "GraphSAGE aggregation")  # no gradient w.r.t. a bf16 table
    if agg_func in ('MEAN', 'SUM') and torch.is_grad_enabled() and table.requires_grad:
        return _GatherMeanAgg.apply(table, idx, agg_func, not trusted)
    if agg_func == 'MAXPOOL' and torch.is_grad_enabled() and table.requires_grad:
        return _GatherMaxPoolAgg.apply(table, idx, not trusted)
    return sage_gather_aggregate(table, idx, agg_func, check=not trusted)


def reduce_neighbors(neigh_feat, kind='MEAN'):
    """MEAN / SUM / MAX(argmax) / MAXPOOL over dim 1 of a pre-gathered [M, k, F] tensor or a
    ``Gathered`` (table, [M, k] index), with autograd for MEAN / SUM / MAXPOOL."""
    if isinstance(neigh_feat, Gathered):
        return _gather_aggregate(neigh_feat.table, neigh_feat.index, kind, neigh_feat.trusted)
    _bf16_inference_only(neigh_feat, "GraphSAGE aggregation")
    if kind in ('MEAN', 'SUM') and torch.is_grad_enabled() and neigh_feat.requires_grad:
        return _MeanAgg.apply(neigh_feat, kind)
    if kind == 'MAXPOOL' and torch.is_grad_enabled() and neigh_feat.requires_grad:
        return _MaxPoolAgg.apply(neigh_feat)
    return sage_aggregate(neigh_feat, kind)


def _gather(x, idx, trusted=False):
    _bf16_inference_only(x, "GraphSAGE row gather")
    if torch.is_grad_enabled() and x.requires_grad:
        return _GatherRows.apply(x, idx, not trusted)
    return gather_rows(x, idx, check=not trusted)


class SageLayer(nn.Module):
    """GraphSAGE/GraphSAGE.py:7-20: relu(W . cat[self, agg]) (or relu(W . agg) in gcn mode)."""

    def __init__(self, input_size, output_size, gcn=False, **kwargs):
        super().__init__(**kwargs)
        self.input_size = input_size
        self.output_size = output_size
        self.gcn = gcn
        self.weight = nn.Linear(self.input_size if self.gcn else 2 * self.input_size, self.output_size, bias=False)

    def forward(self, self_feats, aggregate_feats):
        W = self.weight.weight
        if self.gcn:  # the reference feeds the aggregate straight into Linear (int64 argmax fails there too)
            return F.relu(self.weight(aggregate_feats))
        if aggregate_feats.dtype != torch.float32:  # MAX mode: argmax indices promote like torch.cat
            aggregate_feats = aggregate_feats.to(torch.float32)
        if self_feats.dtype != torch.float32:
            self_feats = self_feats.to(torch.float32)
        n = self.input_size
        # cat([self, agg]) @ W^T == self @ W[:, :n]^T + agg @ W[:, n:]^T (no concat copy)
        part = F.linear(self_feats, W[:, :n])
        if torch.is_grad_enabled() and (W.requires_grad or self_feats.requires_grad
                                        or aggregate_feats.requires_grad):
            return F.relu(torch.addmm(part, aggregate_feats, W[:, n:].t()))
        # inference: ReLU in the GEMM epilogue (hipBLASLt), one kernel fewer
        return torch._addmm_activation(part, aggregate_feats, W[:, n:].t())


def _fused_sage_layer(block, center, neigh: Gathered, dense: nn.Linear | None = None,
                      agg: str = 'MEAN'):
    """Inference SageLayer on a (table, index map) aggregate.

    The table may hold the input features as bfloat16 (``neigh.table.dtype``): the gathers
    read 2-byte elements and write the float32 [self | agg] buffer (the centre rows widened,
    the aggregate reduced in fp32), so the GEMM and everything after it are unchanged.

    ``agg`` 'MAX' / 'MAXPOOL' (centre and neighbours Gathered from one table): the concat
    launch writes the argmax index as fp32 (the value torch.cat([self, argmax]) promotes it
    to) / the value max-pool into the [self | agg] buffer, then the same GEMM.

    Covered shapes (``ops.sage_layer``): ONE launch gathers the centre rows and the
    neighbour mean into an LDS tile and multiplies it by W on the matrix cores, ReLU fused.
    Otherwise the centre rows and the fused gather-mean write the two halves of ONE
    [M, 2F] buffer (the reference's torch.cat, never copied), then a single K=2F GEMM with
    the ReLU in the hipBLASLt epilogue: GraphSAGE.py:18-20 + the gathers of :47-49 as 3
    launches instead of 7; with the centre rows and the neighbours drawn from the same table
    (the sampler's Gathered maps) the two halves come from ONE launch
    (``ops.sage_gather_concat``), then the GEMM: 2 launches.

    ``dense`` (the last layer of a supervised net): the classifier of GraphSAGE.py:51-52 runs in
    the GEMM's epilogue when the MFMA kernel takes the shape (``ops.linear_relu_classify``);
    the return value is then ``(y, logits)``, else ``y`` alone."""
    live = neigh.live
    if live is not None:
        # a device row count: the concat gather + MFMA GEMM run on the buffers' capacity and
        # read the count themselves (no host round trip); other shapes / the classifier
        # epilogue read it back and slice
        W = block.weight.weight
        if (dense is not None or not isinstance(center, Gathered) or center.table is not neigh.table
                or center.live is None or not _sage_gemm_on_mfma(neigh.index.shape[0])
                or W.dtype != torch.float32):
            center, neigh, live = _trim(center), _trim(neigh), None
    if isinstance(center, Gathered):
        self_src, self_idx, trusted = center.table, center.index, center.trusted
    else:
        self_src, self_idx, trusted = center, None, True
    y = None
    if live is None and agg == 'MEAN':
        y = sage_layer(neigh.table, neigh.index, block.weight.weight, self_src, self_idx,
                       check=not (trusted and neigh.trusted))
    if y is not None:
        return y
    M, n = neigh.index.shape[0], block.input_size
    dev = neigh.table.device
    buf = torch.empty((M, 2 * n), dtype=torch.float32, device=dev)
    if live is not None:
        sage_gather_concat(neigh.table, center.index, neigh.index, agg,
                           check=not (center.trusted and neigh.trusted), out=buf, live=live)
        y = gcn_transform(buf, block.weight.weight, relu=True, live=live)
        if y is not None:
            return y
        # the transform does not take the shape: the rows past the count are never read
        buf = buf[:int(live.item())]
        M = buf.shape[0]
    elif isinstance(center, Gathered) and center.table is neigh.table:
        # both halves of cat[self, agg] in one launch (gnn_sage_gather_concat_f32)
        sage_gather_concat(neigh.table, center.index, neigh.index, agg,
                           check=not (center.trusted and neigh.trusted), out=buf)
    else:
        if isinstance(center, Gathered):
            gather_rows(center.table, center.index, out=buf[:, :n], check=not center.trusted)
        else:
            buf[:, :n].copy_(center)  # (widens a bfloat16 centre tensor)
        sage_gather_aggregate(neigh.table, neigh.index, "MEAN", check=not neigh.trusted,
                              out=buf[:, n:])
    return _sage_layer_gemm(block, buf, dense)


def _sage_layer_gemm(block, buf, dense):
    """relu(buf @ W^T) of an inference SageLayer over its input buffer ([self | agg], or the
    aggregate alone in gcn mode); ``(y, logits)`` where ``dense`` ran in the epilogue."""
    M = buf.shape[0]
    W = block.weight.weight
    if dense is not None and _sage_gemm_on_mfma(M):
        yl = linear_relu_classify(buf, W, dense.weight, dense.bias)
        if yl is not None:
            return yl
    if _sage_gemm_on_mfma(M):  # relu(buf @ W^T) on the hand-written fp32-MFMA kernel
        y = gcn_transform(buf, W, relu=True)
        if y is not None:
            return y
    # the addmm's bias operand: a zero vector cached on the block (not a registered buffer,
    # so state_dict keys stay the reference's); a fresh torch.zeros cost a 5 us fill launch
    # per call (profiles/r03k_sage_trace_summary.txt)
    zero = block.__dict__.get("_zero_bias")
    if zero is None or zero.device != W.device or zero.dtype != W.dtype or \
            zero.numel() != W.shape[0]:
        zero = torch.zeros(W.shape[0], dtype=W.dtype, device=W.device)
        block.__dict__["_zero_bias"] = zero
    return torch._addmm_activation(zero, buf, W.t())


# The gcn-mode layers (GraphSAGE(.., gcn=True): relu(W . agg), no centre half) on their own
# kernels: inference through ``_fused_gcn_layer``, training through ``_SageGcnTrainLayerFn``.
# False: the paths from before -- the centre gather nobody reads, ``_GatherMeanAgg`` /
# ``_GatherMaxPoolAgg``, torch's linear and relu (tools/sage_train_ab.py --gcn flips it).
SAGE_GCN_FUSED = True


def _fused_gcn_layer(block, neigh: Gathered, dense: nn.Linear | None = None, agg: str = 'MEAN'):
    """Inference SageLayer in gcn mode on a (table, index map) aggregate: ONE gather-aggregate
    ('MEAN' / 'MAXPOOL', the table fp32 or bf16) straight into an [M, F] buffer, then
    ``_sage_layer_gemm`` (GraphSAGE.py:13-14, 18-20 over the gathers of :48-49; no centre gather:
    the layer never reads it). ``neigh.live`` (a pending batch): the live gather and the live
    GEMM run on the buffers' capacity under the concat layer's conditions, else one host read."""
    live = neigh.live
    W = block.weight.weight
    if live is not None and (dense is not None or not _sage_gemm_on_mfma(neigh.index.shape[0])
                             or W.dtype != torch.float32):
        neigh, live = _trim(neigh), None
    M = neigh.index.shape[0]
    buf = torch.empty((M, block.input_size), dtype=torch.float32, device=neigh.table.device)
    sage_gather_aggregate(neigh.table, neigh.index, agg, check=not neigh.trusted, out=buf,
                          live=live)
    if live is not None:
        y = gcn_transform(buf, W, relu=True, live=live)
        if y is not None:
            return y
        # the transform does not take the shape: the rows past the count are never read
        buf = buf[:int(live.item())]
    return _sage_layer_gemm(block, buf, dense)


# The training SageLayer over a sampler batch as ONE autograd function (``_SageTrainLayerFn``).
# False: the separate row gather, gather-mean and torch linear + addmm + relu, each with its own
# backward (tools/sage_train_ab.py flips it to time both paths in one process).
SAGE_TRAIN_FUSED = True


def _train_layer_backward(ctx, dy, buf, y, W, scatter):
    """The backward of the three training-layer functions, with dY' = dY . [y > 0]:
    dW = dY'^T buf in one masked pass (``gemm_tn_masked``; torch's mm where it declines) and,
    only for a table that requires grad, d table = ``scatter(dBuf)`` with dBuf = dY' W -- the
    adjoint of the layer's own gather, which each function supplies."""
    d_table = dW = g = None
    if ctx.needs_input_grad[1]:
        r = gemm_tn_masked(buf, dy, y, 1.0, False, trans=True)
        if r is not None:
            dW = r[0]
        else:
            g = _masked_grad(dy, y, 1.0)
            dW = torch.mm(g.t(), buf)
    if ctx.needs_input_grad[0]:
        if g is None:
            g = _masked_grad(dy, y, 1.0)
        d_table = scatter(_transform_or_mm(g, W.t().contiguous()))
    return d_table, dW, None, None


class _SageTrainLayerFn(torch.autograd.Function):
    """relu(W . cat[table[cidx], mean_j table[idx[:, j]]]) (GraphSAGE/GraphSAGE.py:17-20 over
    the gathers of :47-49) with autograd w.r.t. W and, where it asks for it, the fp32 table.

    Forward: the inference launches -- ``sage_gather_concat`` writes buf = [self | agg] (the
    table fp32 or bf16), ``gcn_transform`` gives y = relu(buf W^T). Backward, with
    dY' = dY . [y > 0]: dW = dY'^T buf in one masked pass (``gemm_tn_masked``); only for a table
    that requires grad (the layers after the first) dBuf = dY' W and dX = the adjoint of the
    concat gather, ``sage_scatter_concat`` over the device-built transposed maps
    (``sage_maps_transpose``): no sort, CSR or value array built in Python, no float atomics.
    The maps are the device sampler's (in range): nothing is checked, nothing read back."""

    @staticmethod
    def forward(ctx, table, W, cidx, idx):
        buf = sage_gather_concat(table, cidx, idx, "MEAN", check=False)
        y = gcn_transform(buf, W, relu=True)
        if y is None:  # sage_train_layer_supported said the transform takes the shape
            raise RuntimeError("the SageLayer transform refused a shape it reports as covered")
        ctx.save_for_backward(buf, y, W, cidx, idx)
        ctx.n_prev = table.shape[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        buf, y, W, cidx, idx = ctx.saved_tensors

        def scatter(dbuf):
            tr = sage_maps_transpose(cidx, idx, ctx.n_prev, check=False)
            d = None if tr is None else sage_scatter_concat(dbuf, tr, ctx.n_prev)
            if d is None:  # a shape the kernel declines: the SpMM over a Python-built CSR
                n = W.shape[1] // 2
                d = (_scatter_rows(dbuf[:, :n], cidx.reshape(-1, 1), ctx.n_prev, 1.0)
                     + _scatter_rows(dbuf[:, n:], idx, ctx.n_prev, 1.0 / idx.shape[1]))
            return d

        return _train_layer_backward(ctx, dy, buf, y, W, scatter)


# The same for agg_func 'MAXPOOL' (``_SageMaxPoolTrainLayerFn``). False: the separate row gather,
# the argmax and the value launches of ``_GatherMaxPoolAgg`` with its index_put_ backward, and
# torch linear + addmm + relu (tools/sage_train_ab.py --agg MAXPOOL times both in one process).
SAGE_TRAIN_FUSED_MAXPOOL = True


def _maxpool_scatter_torch(dbuf, arg, cidx, idx, n_prev):
    """The masked sum of ``sage_scatter_concat_maxpool`` in torch, for a shape it declines:
    the centre rows by index_add_, each (row, feature) of the aggregate half onto the table row
    of its winner by index_put_ (float atomics: the order of the sums is not fixed).
    ``cidx`` None: ``sage_scatter_agg_maxpool``'s (the gcn-mode layer), dbuf [M, F] with no
    centre half."""
    n = dbuf.shape[1] if cidx is None else dbuf.shape[1] // 2
    out = torch.zeros((n_prev, n), dtype=dbuf.dtype, device=dbuf.device)
    if cidx is not None:
        out.index_add_(0, cidx, dbuf[:, :n])
        dbuf = dbuf[:, n:]
    rows = idx.gather(1, arg.to(torch.int64))                     # [M, F] table rows
    cols = torch.arange(n, device=dbuf.device).expand_as(rows)
    return out.index_put_((rows, cols), dbuf, accumulate=True)


def _gcn_maxpool_scatter_torch(dbuf, arg, idx, n_prev):
    """``_maxpool_scatter_torch`` without the centre half (tools/sage_train_ab.py times it)."""
    return _maxpool_scatter_torch(dbuf, arg, None, idx, n_prev)


class _SageMaxPoolTrainLayerFn(torch.autograd.Function):
    """relu(W . cat[table[cidx], max_j table[idx[:, j]]]) (GraphSAGE/GraphSAGE.py:17-20 over the
    gathers of :47-49, the aggregate torch.max(neigh, dim=1).values) with autograd w.r.t. W and,
    where it asks for it, the fp32 table.

    Forward: ``sage_gather_concat_arg`` writes buf = [self | max-pool] and the winning neighbour
    column of every (row, feature) as a uint8 (the first maximum, a NaN first: torch's rule),
    ``gcn_transform`` gives y = relu(buf W^T). Backward as ``_SageTrainLayerFn``: dW in one
    masked pass; only for a table that requires grad dBuf = dY' W and dX =
    ``sage_scatter_concat_maxpool`` over the device-built transposed maps: each neighbour slot
    adds the gradient elements it won, in slot order -- no [n_prev, F] zero table, no [M, F]
    int64 row ids, no index_put_, no float atomics."""

    @staticmethod
    def forward(ctx, table, W, cidx, idx):
        r = sage_gather_concat_arg(table, cidx, idx, check=False)
        if r is None:  # sage_train_layer_supported said the gather takes the shape
            raise RuntimeError("the max-pool concat gather refused a shape it reports as covered")
        buf, arg = r
        y = gcn_transform(buf, W, relu=True)
        if y is None:
            raise RuntimeError("the SageLayer transform refused a shape it reports as covered")
        ctx.save_for_backward(buf, y, W, cidx, idx, arg)
        ctx.n_prev = table.shape[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        buf, y, W, cidx, idx, arg = ctx.saved_tensors

        def scatter(dbuf):
            tr = sage_maps_transpose(cidx, idx, ctx.n_prev, check=False)
            d = None if tr is None else sage_scatter_concat_maxpool(dbuf, arg, tr, ctx.n_prev)
            if d is None:  # a shape the kernel declines
                d = _maxpool_scatter_torch(dbuf, arg, cidx, idx, ctx.n_prev)
            return d

        return _train_layer_backward(ctx, dy, buf, y, W, scatter)


class _SageGcnTrainLayerFn(torch.autograd.Function):
    """relu(W . agg_j table[idx[:, j]]) (the gcn-mode SageLayer, GraphSAGE/GraphSAGE.py:13-14,
    18-20 over the gathers of :48-49; ``agg`` 'MEAN' or 'MAXPOOL') with autograd w.r.t. W and,
    where it asks for it, the fp32 table.

    Forward: ``sage_gather_aggregate`` (MEAN) or ``sage_gather_aggregate_arg`` (MAXPOOL: the
    winner of every (row, feature) as one byte) writes buf [M, F], ``gcn_transform`` gives
    y = relu(buf W^T). Backward as ``_SageTrainLayerFn``: dW = dY'^T buf in one masked pass; only
    for a table that requires grad dBuf = dY' W and dX = ``sage_scatter_agg`` /
    ``sage_scatter_agg_maxpool`` over ``sage_maps_transpose_nbr``: M k slots, fp32 sums in slot
    order, no float atomics. The maps are the device sampler's: nothing checked or read back."""

    @staticmethod
    def forward(ctx, table, W, idx, agg):
        arg = None
        if agg == 'MAXPOOL':
            r = sage_gather_aggregate_arg(table, idx, check=False)
            if r is None:  # sage_train_layer_supported said the gather takes the shape
                raise RuntimeError("the max-pool gather refused a shape it reports as covered")
            buf, arg = r
        else:
            buf = sage_gather_aggregate(table, idx, "MEAN", check=False)
        y = gcn_transform(buf, W, relu=True)
        if y is None:
            raise RuntimeError("the SageLayer transform refused a shape it reports as covered")
        ctx.save_for_backward(buf, y, W, idx, arg)
        ctx.n_prev = table.shape[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        buf, y, W, idx, arg = ctx.saved_tensors

        def scatter(dbuf):
            tr = sage_maps_transpose_nbr(idx, ctx.n_prev, check=False)
            d = None
            if tr is not None:
                d = (sage_scatter_agg(dbuf, tr, ctx.n_prev) if arg is None else
                     sage_scatter_agg_maxpool(dbuf, arg, tr, ctx.n_prev))
            if d is None:  # a shape the kernel declines
                d = (_scatter_rows(dbuf, idx, ctx.n_prev, 1.0 / idx.shape[1]) if arg is None else
                     _maxpool_scatter_torch(dbuf, arg, None, idx, ctx.n_prev))
            return d

        return _train_layer_backward(ctx, dy, buf, y, W, scatter)


def _train_layer_takes(table, W, idx, agg: str, gcn: bool) -> bool:
    """What both training layers ask of a batch before ``sage_train_layer_supported``: an int64
    [M, k] map with rows, somebody who wants a gradient, and no bfloat16 table among them."""
    return (idx.dim() == 2 and idx.dtype == torch.int64 and idx.shape[0] > 0
            and (W.requires_grad or table.requires_grad)
            and not (table.dtype == torch.bfloat16 and table.requires_grad)  # raises as before
            and sage_train_layer_supported(table, W, idx.shape[1], agg, gcn=gcn))


def _sage_gcn_train_layer(block, neigh: Gathered, agg: str):
    """The gcn-mode training SageLayer on a trusted map, or None where ``_SageGcnTrainLayerFn``
    does not cover the layer (the caller takes the unfused path)."""
    table, W, idx = neigh.table, block.weight.weight, neigh.index
    if not _train_layer_takes(table, W, idx, agg, True):
        return None
    return _SageGcnTrainLayerFn.apply(table, W, idx, agg)


def _sage_train_layer(block, center: Gathered, neigh: Gathered, agg: str = 'MEAN'):
    """The training SageLayer on trusted maps over one table, or None where
    ``_SageTrainLayerFn`` / ``_SageMaxPoolTrainLayerFn`` does not cover the layer (the caller
    takes the unfused path)."""
    table, W = neigh.table, block.weight.weight
    idx, cidx = neigh.index, center.index
    if (idx.dim() != 2 or cidx.dtype != torch.int64 or cidx.numel() != idx.shape[0]
            or not _train_layer_takes(table, W, idx, agg, False)):
        return None
    fn = _SageMaxPoolTrainLayerFn if agg == 'MAXPOOL' else _SageTrainLayerFn
    return fn.apply(table, W, cidx, idx)


# The head of the unsupervised step on the device (csrc/sage_score.hip): the scores of
# GraphSAGE.py:61 as ``_SageScoreFn`` in place of torch.bmm over a permuted operand, and
# ``unsupervised_loss`` in place of the training loop's binary_cross_entropy_with_logits.
# False: torch's bmm and torch's loss everywhere (tools/unsup_head_ab.py times both).
SAGE_SCORE_FUSED = True


class _SageScoreFn(torch.autograd.Function):
    """scores[b, 0, s] = center[b] . second[b, s] for center [B, H], second [B, S, H]:
    ``torch.bmm(center.unsqueeze(1), second.permute(0, 2, 1))`` as one launch
    (``sage_score``). Backward, one launch (``sage_score_backward``): d_second = g * center in
    the second tower's own [B S, H] layout (no permuted intermediate to copy back) and
    d_center = sum_s g second in a fixed order; a half nobody asks for is not computed."""

    @staticmethod
    def forward(ctx, center, second):
        B, S, H = second.shape
        z = sage_score(center, second.reshape(B * S, H), S)
        if z is None:  # _score_fused_ok said the kernel takes these operands
            raise RuntimeError("the score kernel refused operands it reports as covered")
        ctx.save_for_backward(center, second)
        return z.reshape(B, 1, S)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        center, second = ctx.saved_tensors
        B, S, H = second.shape
        r = sage_score_backward(g.reshape(B, S), center, second.reshape(B * S, H),
                                ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if r is None:
            raise RuntimeError("the score kernel refused operands it reports as covered")
        dc, dx = r
        return dc, None if dx is None else dx.reshape(B, S, H)


def _score_fused_ok(center, second) -> bool:
    """Whether ``_SageScoreFn`` takes center [B, H] and second [B, S, H]: the switch is on, both
    are fp32 device tensors and the score kernels take the width and the two layouts."""
    if not (SAGE_SCORE_FUSED and center.is_cuda and second.is_cuda
            and center.dtype == torch.float32 and second.dtype == torch.float32
            and center.dim() == 2 and second.dim() == 3 and second.shape[0] == center.shape[0]
            and second.shape[2] == center.shape[1] and second.is_contiguous()):
        return False
    return _score_takes(center, second.reshape(-1, center.shape[1]))


class _BceLogitsFn(torch.autograd.Function):
    """mean binary cross entropy with logits of z [rows, cols] against y (``bce_logits``): the
    forward launch also writes g = dL/dz, the backward is g times the incoming scalar."""

    @staticmethod
    def forward(ctx, z, y):
        loss, g = bce_logits(z, y, want_grad=ctx.needs_input_grad[0])
        if g is not None:
            ctx.save_for_backward(g)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return g * grad_out, None


def unsupervised_loss(scores, labels):
    """The unsupervised loss of the reference's loop (GraphSAGE/train_eval.py:113-114),
    ``F.binary_cross_entropy_with_logits(scores.reshape(labels.shape).float(), labels.float())``,
    as one autograd function over ``bce_logits``: ``scores`` [B, 1, S] or [B, S], ``labels``
    int64 or float [B, S]; a 0-dim tensor. torch's function where the kernel does not apply
    (CPU tensors, no elements, other dtypes, a layout it declines, SAGE_SCORE_FUSED off)."""
    z = scores.reshape(labels.shape)
    if (SAGE_SCORE_FUSED and z.is_cuda and labels.is_cuda and z.dtype == torch.float32
            and labels.dtype in (torch.float32, torch.int64) and z.dim() >= 1
            and z.numel() > 0 and not labels.requires_grad):
        z2, y2 = z.reshape(-1, z.shape[-1]), labels.reshape(-1, labels.shape[-1])
        if _bce_takes(z2, y2):
            return _BceLogitsFn.apply(z2, y2)
    return F.binary_cross_entropy_with_logits(z.float(), labels.float())


class GraphSAGE(nn.Module):
    """GraphSAGE/GraphSAGE.py:23-61 with the same 9-argument forward."""

    def __init__(self, num_layers, input_size, out_size, gcn=False, agg_func='MEAN', Unsupervised=True, class_size=None,
                 **kwargs):
        super().__init__(**kwargs)
        self.num_layers = num_layers
        self.gcn = gcn
        self.agg_func = agg_func
        self.sage_blocks = nn.Sequential()
        for index in range(0, num_layers):
            layer_size = out_size if index != 0 else input_size
            self.sage_blocks.add_module('sage_layer' + str(index), SageLayer(layer_size, out_size, gcn=self.gcn))
        self.Unsupervised = Unsupervised
        if not Unsupervised:
            self.dense = nn.Linear(out_size, class_size)

    def _fused_ok(self, block, center, neigh) -> bool:
        if torch.is_grad_enabled() or not isinstance(neigh, Gathered):
            return False
        if block.gcn:  # the aggregate alone (``_fused_gcn_layer``): no centre rows to place
            return (SAGE_GCN_FUSED and self.agg_func in ('MEAN', 'MAXPOOL')
                    and neigh.table.dtype in (torch.float32, torch.bfloat16))
        if self.agg_func == 'MEAN':
            return True
        # MAX / MAXPOOL: the one-launch concat form (centre and neighbours from one table)
        # (a float32 table, or the stored input features as bfloat16: both halves stay fp32)
        return (self.agg_func in ('MAX', 'MAXPOOL') and isinstance(center, Gathered)
                and center.table is neigh.table
                and neigh.table.dtype in (torch.float32, torch.bfloat16))

    def _train_fused_ok(self, block, center, neigh) -> bool:
        """The training layer (``_SageTrainLayerFn`` / ``_SageMaxPoolTrainLayerFn``): MEAN or
        MAXPOOL over cat[self, agg], centre and neighbours Gathered over ONE table through the
        device sampler's (trusted) maps."""
        on = {'MEAN': SAGE_TRAIN_FUSED, 'MAXPOOL': SAGE_TRAIN_FUSED_MAXPOOL}.get(self.agg_func)
        return (bool(on) and torch.is_grad_enabled() and not block.gcn
                and isinstance(center, Gathered)
                and isinstance(neigh, Gathered) and center.table is neigh.table
                and center.trusted and neigh.trusted)

    def _train_gcn_fused_ok(self, block, neigh) -> bool:
        """The gcn-mode training layer (``_SageGcnTrainLayerFn``): MEAN or MAXPOOL over the
        aggregate alone, the neighbours Gathered through the device sampler's (trusted) map."""
        return (SAGE_GCN_FUSED and torch.is_grad_enabled() and block.gcn
                and self.agg_func in ('MEAN', 'MAXPOOL')
                and isinstance(neigh, Gathered) and neigh.trusted)

    def forward(self, center_feats_data, center_nodes_map, center_neigh_feats_data, center_neigh_nodes_map,
                contexts_negatives_feats_data, contexts_negatives_nodes_map, contexts_negatives_neigh_feats_data,
                contexts_negatives_neigh_nodes_map, contexts_negatives_shape):
        if contexts_negatives_feats_data is None:
            center = center_feats_data         # tensor, or Gathered (table, [M] index)
            neigh = center_neigh_feats_data    # [M, k, F] tensor, or Gathered (table, [M, k] index)
            feats_data = classes = None
            for i, block in enumerate(self.sage_blocks):
                if self._fused_ok(block, center, neigh):
                    last = i == self.num_layers - 1 and not self.Unsupervised
                    dense = self.dense if last else None
                    if block.gcn:
                        feats_data = _fused_gcn_layer(block, neigh, dense, self.agg_func)
                    else:
                        feats_data = _fused_sage_layer(block, center, neigh, dense,
                                                       self.agg_func)
                    if isinstance(feats_data, tuple):  # the classifier ran in the epilogue
                        feats_data, classes = feats_data
                else:
                    center, neigh = _trim(center), _trim(neigh)
                    feats_data = None
                    if self._train_fused_ok(block, center, neigh):
                        feats_data = _sage_train_layer(block, center, neigh, self.agg_func)
                    elif self._train_gcn_fused_ok(block, neigh):
                        feats_data = _sage_gcn_train_layer(block, neigh, self.agg_func)
                    if feats_data is None:
                        if isinstance(center, Gathered):
                            center = _gather(center.table, center.index, center.trusted)
                        feats_data = block(center, Aggregator(neigh, self.agg_func))
                if i != self.num_layers - 1:
                    cm = center_nodes_map[i]
                    nm = center_neigh_nodes_map[i]
                    if _trusted(cm) and _trusted(nm):  # device-sampler maps: no -1, in range
                        lv = getattr(cm, "_gnn_live", None)  # sync=False batch: device size
                        center = Gathered(feats_data, cm, True, lv)
                        neigh = Gathered(feats_data, nm, True, lv)
                    else:                              # GraphSAGE.py:56-57 (-1 padding dropped)
                        center = Gathered(feats_data, cm[cm != -1], False)
                        neigh = Gathered(feats_data, nm[nm[:, 0] != -1, :], False)
            if not self.Unsupervised and classes is None:
                classes = self.dense(feats_data)
            return feats_data, classes
        center_feats_data, _ = self(center_feats_data, center_nodes_map, center_neigh_feats_data,
                                    center_neigh_nodes_map, None, None, None, None, None)
        contexts_negatives_feats_data, _ = self(contexts_negatives_feats_data, contexts_negatives_nodes_map,
                                                contexts_negatives_neigh_feats_data,
                                                contexts_negatives_neigh_nodes_map, None, None, None, None, None)
        contexts_negatives_feats_data = contexts_negatives_feats_data.reshape(*contexts_negatives_shape, -1)
        if _score_fused_ok(center_feats_data, contexts_negatives_feats_data):
            return center_feats_data, _SageScoreFn.apply(center_feats_data,
                                                         contexts_negatives_feats_data)
        return center_feats_data, torch.bmm(center_feats_data.unsqueeze(1), contexts_negatives_feats_data.permute(0, 2, 1))
