"""Device ops over the C-ABI: every call launches hand-written gfx950 kernels.

No op here has a CPU path: tensors must live on a ROCm device and the HIP
library must be loadable, otherwise a RuntimeError is raised.
"""
from __future__ import annotations

import contextlib
from typing import NamedTuple

import torch

from . import _lib
from .graph import GAT_SEG_BYTES, CsrGraph, seg_len_for, staged_plan

_ACT_FLAGS = {None: 0, "relu": _lib.EPI_RELU, "elu": _lib.EPI_ELU}


def _require_device(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "graphneuralnetwork_amd ops run only on a ROCm (MI355X) device tensor; "
                f"got a tensor on {t.device}. There is no CPU fallback.")


def _rows_f32(x: torch.Tensor, name: str) -> torch.Tensor:
    if x.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {x.dtype})")
    if x.dim() != 2:
        raise ValueError(f"{name} must be 2-D [rows, features]")
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def _rows_x(x: torch.Tensor, name: str) -> torch.Tensor:
    """The SpMM's gathered table: fp32, or bf16-stored rows (accumulated in fp32)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name} must be float32 or bfloat16 (got {x.dtype})")
    if x.dim() != 2:
        raise ValueError(f"{name} must be 2-D [rows, features]")
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def _bf16(t: torch.Tensor) -> bool:
    return t.dtype == torch.bfloat16


def _f32_or_bf16(t: torch.Tensor, name: str) -> None:
    """The dtype rule of the SAGE ops, applied before anything else looks at the tensor."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name} must be float32 or bfloat16 (got {t.dtype})")


def _bf16_inference_only(t: torch.Tensor, what: str) -> None:
    """bf16 rows are a storage type of the inputs: nothing differentiates with respect to them
    (a bf16 table WITHOUT grad works in training -- the gradients go to the weights)."""
    if torch.is_grad_enabled() and t.dtype == torch.bfloat16 and t.requires_grad:
        raise TypeError(f"{what}: a bfloat16 table is supported at inference only; training "
                        "runs in fp32 (gradients flow through float32 feature rows)")


# Hub staging (gnn_spmm_csr_hub_f32 / gnn_gat_csr_hub_f32): when the gathered table is
# too large to stay in the Infinity Cache, its highest-degree rows (at most HUB_ROWS rows,
# at most HUB_BYTES) are copied into one compact table per call. A/B on MI355X
# (tools/hub_ab.py, profiles/r01f_hub_ab_*.log): SpMM 10M/207M F=128 20.9 -> 14.4 ms
# (best 64-128 Ki rows), F=256 40.0 -> 30.0 ms (flat 32-128 Ki rows); 1M/20M F=128
# 1.57 -> 1.16 ms (flat 8-128 Ki rows), F=64 0.71 -> 0.59 ms (best 64 Ki rows); GAT
# 8x8 heads on 1M/20M 1.00 -> 0.94-0.95 ms (best 16-64 Ki rows); a 128 MB table (F=32)
# gains ~1 % and a 64 MB one (F=16) loses ~2 %, hence the size threshold.
HUB_MIN_X_BYTES = 192 << 20
HUB_BYTES = 64 << 20
HUB_ROWS = 131072


def hub_rows_for(n_cols: int, feat: int, elem_size: int = 4) -> int:
    """Default number of staged hub rows for a gathered table of n_cols x feat elements of
    ``elem_size`` bytes (4: fp32, 2: bf16; 0 = no staging). The size threshold is taken on the
    table's real bytes; the row caps are those of fp32, so a graph's hub plans are shared
    between the element types."""
    if n_cols * elem_size * feat < HUB_MIN_X_BYTES:
        return 0
    return min(n_cols, HUB_ROWS, max(1, HUB_BYTES // (4 * feat)))


# XCD-sliced hub staging (graph.XcdHubPlan): on graphs with at least XCD_MIN_NNZ stored
# entries whose X would be hub-staged, the hub edges of rows of degree >= XCD_MIN_DEG are
# reduced per (row, XCD slice) first, so each XCD's L2 serves 1/8 of the hub table.
# Measured with tools/workingset_probe.py and tools/xcd_hub_probe.py (profiles/r02y_*):
# a gather set that fits one XCD's L2 runs at ~50 G rows/s, 16-256 MiB sets at 14-19 (the
# Infinity Cache hardly beats HBM's 12); emulated, cfg2 1.14 -> 0.96 ms and the north star
# 14.4 -> 12.4 ms at 256 Ki hub rows, degree >= 128, items of <= 128 edges.
XCD_MIN_NNZ = 4_000_000
XCD_HUB_BYTES = 128 << 20
XCD_HUB_ROWS = 262144
XCD_MIN_DEG = 128
XCD_CHUNK = 128
XCD_PHASES = 1  # slices per XCD, run one after another (graph.xcd_hub_coo ``phases``)
XCD_ITEM_ROWS = None  # items read only the hottest XCD_ITEM_ROWS hub rows (None: all K)
# rows below XCD_MIN_DEG get items too, for each slice holding >= XCD_SMALL_ITEM of their hub
# edges (None: off; graph.xcd_hub_coo ``small_item``)
XCD_SMALL_ITEM = None
# on a degree-ordered graph (graph.degree_order) the hub rows are X's first rows: read them
# in place instead of copying them into a staged table (XcdHubPlan.prefix / direct)
XCD_DIRECT = True
# pass 1 of that direct form on gnn_spmm_items_f32 (one wave per item, the edge stream in
# scalar registers) where the entry covers the call: fp32 X of 128 or 256 columns on the
# 16-B vector path. Same partial rows bit for bit; A/B: tools/spmm_items_ab.py, DESIGN.md
# section 5.20.
SPMM_ITEMS_KERNEL = True
# bf16 rows (spmm_forward with a bfloat16 X): whether the default policy (``xcd=None``) takes
# the XCD-sliced direct form at all. Off: measured in one process at cfg2 on the
# column-ordered graph (tools/spmm_bf16_ab.py), the hub rows read in
# place by the hub-staged kernel beat the two-pass XCD form, whose second pass gathers bf16 X
# rows and fp32 partial rows through one kernel at half the occupancy. ``xcd=True`` still
# selects it.
XCD_BF16 = False


def xcd_hub_rows_for(n_cols: int, feat: int, elem_size: int = 4) -> int:
    """Default hub rows of the XCD-sliced staging (0 = X too small to stage; ``elem_size`` as
    in ``hub_rows_for``)."""
    if n_cols * elem_size * feat < HUB_MIN_X_BYTES:
        return 0
    return min(n_cols, XCD_HUB_ROWS, max(64, XCD_HUB_BYTES // (4 * feat)))


# Packed row tasks (gnn_spmm_csr_tasks_f32, spmm.hip packed_rows): rows of degree <=
# TASK_MAX_DEG are streamed a task (<= 63 consecutive rows, ~TASK_COST edges + rows) per wave
# instead of one wave per row, so the rowptr -> col -> X chain of short rows is paid once per
# task. Needs the 16-B vector path. Narrow rows (feat <= 32: LPR <= 8 lanes per row, 8 or more
# edge slots per wave) take tasks of up to TASK_COST_NARROW edges + rows, so that every slot of
# the wave gets rows (one wave per row left most of its lanes idle at feat 8).
SPMM_TASKS = True
SPMM_TASKS_NARROW = True
TASK_MAX_DEG = 128
TASK_COST = 128  # 256 until late round 4: 128 is 0.7 % faster with the slice groups (cfg2, north star)
TASK_COST_NARROW = 2048


def _task_cost(feat: int) -> int:
    return TASK_COST_NARROW if feat <= 32 else TASK_COST


def _tasks_ok(feat: int, *ts) -> bool:
    # every column block of the launch (<= 2048 wide) must be a vector block; one of 32 or
    # fewer columns only with the narrow tasks. A bf16 table's vector path holds 8 elements per
    # lane: whole 16-B pieces per row, row pitch a multiple of 8
    bf16 = any(t is not None and t.dtype == torch.bfloat16 for t in ts)
    if not SPMM_TASKS or feat % (8 if bf16 else 4) or (
            not SPMM_TASKS_NARROW and (feat <= 32 or 0 < feat % 2048 <= 32)):
        return False
    return all(t is None or (t.data_ptr() % 16 == 0 and (
        t.dim() == 1 or t.stride(0) % (8 if t.dtype == torch.bfloat16 else 4) == 0))
        for t in ts)


def _spmm_run(stem: str, g: CsrGraph, x, feat, bias, y, ldy, partial, flags, stream, **kw):
    """Run ``stem``_f32 or ``stem``_bf16 (by x's element type) of the gnn_spmm_csr entries: the
    operands every one of them takes and, in ``kw``, the entry's column array, plan and hub
    table."""
    _lib.run(stem + ("_bf16" if x.dtype == torch.bfloat16 else "_f32"),
             rowptr=g.rowptr.data_ptr(), val=g.val.data_ptr(), n_rows=g.n_rows, x=x.data_ptr(),
             ldx=x.stride(0), feat=feat, bias=_lib.ptr(bias), y=y.data_ptr(), ldy=ldy,
             partial=_lib.ptr(partial), flags=flags, stream=stream, **kw)


def _hub_table(x, xh) -> dict:
    """The hub table of the hub / tasks entries (None: no table). The bf16 entries also take its
    element type: ``xh_f32`` = 1 for an fp32 table (the XCD-direct partial rows), 0 for a bf16
    one or none."""
    kw = dict(xh=_lib.ptr(xh), ldh=xh.stride(0) if xh is not None else 0)
    if x.dtype == torch.bfloat16:
        kw["xh_f32"] = int(xh is not None and xh.dtype == torch.float32)
    return kw


def _spmm_tasks_call(g: CsrGraph, col: torch.Tensor, tp, x, xh, feat, bias, y, ldy, partial,
                     flags, stream):
    _spmm_run("gnn_spmm_csr_tasks", g, x, feat, bias, y, ldy, partial, flags, stream,
              col=col.data_ptr(), **_hub_table(x, xh), **tp.segments(), **tp.task_rows())


def _spmm_hub_call(g: CsrGraph, col: torch.Tensor, plan, skip_empty, x, xh, feat, bias, y, ldy,
                   partial, flags, stream):
    _spmm_run("gnn_spmm_csr_hub", g, x, feat, bias, y, ldy, partial, flags, stream,
              col_hub=col.data_ptr(), **_hub_table(x, xh), **plan.segments(),
              **plan.spmm_rows(skip_empty))


def _spmm_plain_call(g: CsrGraph, plan, skip_empty, x, feat, bias, y, ldy, partial, flags, stream):
    _spmm_run("gnn_spmm_csr", g, x, feat, bias, y, ldy, partial, flags, stream,
              col=g.col.data_ptr(), **plan.segments(), **plan.spmm_rows(skip_empty))


def _gather_hub_rows(lib, x, hub_ids, k, feat, out, err, stream):
    """out[:k] = x[hub_ids]: the staging copy of the hub rows (fp32 or bf16 elements)."""
    fn, name = ((lib.gnn_gather_rows_bf16, "gnn_gather_rows_bf16")
                if x.dtype == torch.bfloat16 else
                (lib.gnn_gather_rows_f32, "gnn_gather_rows_f32"))
    _lib.check(fn(x.data_ptr(), x.stride(0), x.shape[0], hub_ids.data_ptr(), k, feat,
                  out.data_ptr(), out.stride(0), err.data_ptr(), stream), name)


def spmm_forward(g: CsrGraph, x: torch.Tensor, bias: torch.Tensor | None = None,
                 activation: str | None = None, out: torch.Tensor | None = None,
                 seg_len: int | None = None, accumulate: bool = False,
                 hubs: int | None = None, xcd: bool | None = None) -> torch.Tensor:
    """Y = A.X (+ bias) (act) with A in CSR -- the GCN aggregation (GCN/GCN.py:43-45).

    ``accumulate=True`` adds into ``out`` (Y = out + A.X ...): the halo pass of
    the multi-GPU edge-cut aggregation.

    ``seg_len`` overrides the long-row threshold (rows with more edges are split
    across wavefronts); by default it is sized from the feature width.

    ``hubs`` = number of highest-degree rows of X staged into a compact table before
    the gather (0: none; default ``hub_rows_for``). It changes speed, not results: the
    output is bit-identical to the unstaged kernel's.

    ``xcd`` = XCD-sliced hub staging (``graph.XcdHubPlan``; default: on for graphs of at
    least XCD_MIN_NNZ entries whose X is staged and no explicit ``hubs``). Same sums,
    regrouped: equal to the unstaged result to fp32 rounding, bitwise reproducible.

    ``x`` may be bfloat16 (feature rows stored as under ``torch.autocast``): the gathered rows
    are widened exactly and accumulated in fp32 by the same kernels (gnn_spmm_csr_bf16 and its
    hub / tasks forms); ``bias``, ``out`` and the result stay float32, and every option above
    works. Two differences in routing, not in what is computed: the XCD-sliced form exists for
    bf16 only where the hub rows are X's first rows (a degree-ordered graph, read in place);
    elsewhere, where fp32 would stage hub and partial rows in one buffer, a bf16 ``x`` takes
    the hub-staged non-XCD path with the same ``hubs``. And by default (``xcd=None``) a bf16
    ``x`` takes the hub-staged path on every graph (``XCD_BF16``: it measured faster);
    ``xcd=True`` selects the XCD-sliced direct form.
    """
    if accumulate and out is None:  # checked first: it is a usage error on any device
        raise ValueError("accumulate=True needs `out` (it adds into the caller's buffer)")
    _require_device(g.rowptr, x, bias, out)
    x = _rows_x(x, "X")
    bf16 = x.dtype == torch.bfloat16
    esize = x.element_size()
    if x.shape[0] != g.n_cols:
        raise ValueError(f"X has {x.shape[0]} rows, adjacency has {g.n_cols} columns")
    feat = x.shape[1]
    if bias is not None:
        bias = bias.contiguous()
        if bias.dtype != torch.float32 or bias.numel() != feat:
            raise ValueError("bias must be float32 [features]")
    if out is None:
        out = torch.empty((g.n_rows, feat), dtype=torch.float32, device=x.device)
    elif out.shape != (g.n_rows, feat) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise ValueError("out must be float32 [n_rows, features] with unit column stride")
    if g.n_rows == 0 or feat == 0:
        return out
    seg = seg_len if seg_len is not None else seg_len_for(feat)
    if x.numel() == 0:  # no column to gather from (e.g. an empty halo): never read
        x = torch.empty((1, feat), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    flags = _ACT_FLAGS[activation] | (_lib.EPI_ACCUMULATE if accumulate else 0)
    stream = _lib.stream_handle(x.device)
    # out += A.X with no bias / activation: rows without edges stay as they are
    skip_empty = accumulate and bias is None and activation is None
    if xcd is None:
        xcd = (hubs is None and g.nnz >= XCD_MIN_NNZ and (not bf16 or XCD_BF16)
               and xcd_hub_rows_for(g.n_cols, feat, esize) > 0)
    if xcd and g.nnz:
        kx = (xcd_hub_rows_for(g.n_cols, feat, esize) if hubs is None
              else min(int(hubs), g.n_cols))
        chunk = min(XCD_CHUNK, seg)
        ok = kx >= 8 * XCD_PHASES and chunk >= 4
        if ok and bf16 and not (XCD_DIRECT and g.hub_plan(kx).prefix):
            ok = False  # bf16: the direct form only (one buffer cannot hold both row types)
        xp = (g.xcd_hub_plan(kx, XCD_MIN_DEG, chunk, XCD_PHASES, XCD_ITEM_ROWS, XCD_SMALL_ITEM)
              if ok else None)
        if xp is not None:
            _spmm_xcd(lib, g, xp, x, feat, bias, out, seg, skip_empty, flags, stream)
            return out
    plan = g.plan(seg)
    partial = None
    if plan.n_seg:
        partial = torch.empty((plan.n_seg, feat), dtype=torch.float32, device=x.device)
    k = hub_rows_for(g.n_cols, feat, esize) if hubs is None else min(int(hubs), g.n_cols)
    tasks = _tasks_ok(feat, x, out, bias, partial)
    if k > 0 and g.nnz:
        hp = g.hub_plan(k)
        if XCD_DIRECT and hp.prefix:  # degree-ordered columns: the hub rows are X's first rows
            xh = x
        else:
            xh = torch.empty((hp.k, feat), dtype=x.dtype, device=x.device)
            _gather_hub_rows(lib, x, hp.hub_ids, hp.k, feat, xh, hp.err, stream)
        if tasks:
            _spmm_tasks_call(g, hp.col_hub, g.task_plan(seg, TASK_MAX_DEG, _task_cost(feat)),
                             x, xh, feat, bias, out, out.stride(0), partial,
                             flags | (_lib.EPI_SKIP_EMPTY if skip_empty else 0), stream)
            return out
        _spmm_hub_call(g, hp.col_hub, plan, skip_empty, x, xh, feat, bias, out, out.stride(0),
                       partial, flags, stream)
        return out
    if tasks and g.nnz:
        _spmm_tasks_call(g, g.col, g.task_plan(seg, TASK_MAX_DEG, _task_cost(feat)), x, None,
                         feat, bias, out, out.stride(0), partial,
                         flags | (_lib.EPI_SKIP_EMPTY if skip_empty else 0), stream)
        return out
    _spmm_plain_call(g, plan, skip_empty, x, feat, bias, out, out.stride(0), partial, flags,
                     stream)
    return out


def _spmm_xcd(lib, g: CsrGraph, xp, x, feat, bias, out, seg, skip_empty, flags, stream):
    """The XCD-sliced hub SpMM: hub rows -> staged buffer, pass 1 (items -> partial rows of
    the same buffer, workgroup w on XCD w % 8 holds only slice w % 8), pass 2 (remaining
    edges + partial refs, with the epilogue). Three launches on one stream."""
    k, n_pos = xp.k, xp.n_pos
    if XCD_DIRECT and xp.prefix:
        _spmm_xcd_direct(xp, x, feat, bias, out, seg, skip_empty, flags, stream)
        return
    buf = torch.empty((k + n_pos, feat), dtype=torch.float32, device=x.device)
    hp = xp.hub
    _lib.check(lib.gnn_gather_rows_f32(x.data_ptr(), x.stride(0), x.shape[0],
                                       hp.hub_ids.data_ptr(), k, feat, buf.data_ptr(), feat,
                                       hp.err.data_ptr(), stream), "gnn_gather_rows_f32")
    p1 = xp.items.plan(seg)
    if p1.n_seg or p1.n_small:  # by construction every item is a 2..chunk-edge row
        raise RuntimeError("XCD hub plan: item rows outside the mid-row class")
    _spmm_hub_call(xp.items, xp.items.col, p1, False, x, buf, feat, None, buf[k:], feat, None, 0,
                   stream)
    if _tasks_ok(feat, x, out, bias, buf):
        tp = xp.rest.task_plan(seg, TASK_MAX_DEG, _task_cost(feat))
        partial = None
        if tp.base.n_seg:
            partial = torch.empty((tp.base.n_seg, feat), dtype=torch.float32, device=x.device)
        _spmm_tasks_call(xp.rest, xp.rest.col, tp, x, buf, feat, bias, out, out.stride(0),
                         partial, flags | (_lib.EPI_SKIP_EMPTY if skip_empty else 0), stream)
        return
    p2 = xp.rest_plan(seg)
    partial = None
    if p2.n_seg:
        partial = torch.empty((p2.n_seg, feat), dtype=torch.float32, device=x.device)
    _spmm_hub_call(xp.rest, xp.rest.col, p2, skip_empty, x, buf, feat, bias, out, out.stride(0),
                   partial, flags, stream)


# Storage type of the support tensor S = X W^T between Graph_conv_layer's transform and its
# aggregation at inference. torch.bfloat16: the transform stores S as bf16
# (gnn_gcn_transform_bf16out) and the SpMM gathers bf16 rows, accumulating in fp32
# (gnn_spmm_csr_bf16): half the bytes per gathered row and half the support's memory, for a
# relative rounding of 2^-9 per support element. Training, and layers whose shape the MFMA
# transform does not cover, stay fp32. Set it through ``support_dtype``.
SUPPORT_DTYPE = torch.float32


@contextlib.contextmanager
def support_dtype(dtype: torch.dtype):
    """Sets ``SUPPORT_DTYPE`` (torch.float32 or torch.bfloat16) for the block and restores the
    previous value on exit (nests)."""
    global SUPPORT_DTYPE
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"support dtype must be float32 or bfloat16 (got {dtype})")
    prev = SUPPORT_DTYPE
    SUPPORT_DTYPE = dtype
    try:
        yield
    finally:
        SUPPORT_DTYPE = prev


# Graph_conv_layer runs its aggregation over the column-degree-ordered graph A P^T
# (graph.degree_order(rows=False)) whenever the SpMM would take the XCD-sliced path: the
# transform writes the support rows in that order (gcn_transform rows=perm) and the SpMM reads
# the hub rows in place (no staging copy). Output rows stay in the original order.
DEGREE_ORDER = True


# None: every column ranked by in-degree; an int: only that many hub columns ranked first, the
# rest in id order (graph.degree_order ``prefix``), so the scattered-row producers (transform /
# projection) store the non-hub rows in ascending order. Must be >= every hub count K taken
# from the order (XCD_HUB_ROWS, HUB_ROWS).
COLUMN_ORDER_PREFIX = None


def _cached_column_order(g: CsrGraph):
    prefix = COLUMN_ORDER_PREFIX
    if prefix is not None and prefix < max(XCD_HUB_ROWS, HUB_ROWS):
        raise ValueError("COLUMN_ORDER_PREFIX must cover the hub rows (XCD_HUB_ROWS, HUB_ROWS)")
    key = ("_colorder",) if prefix is None else ("_colorder", prefix)
    o = g._plans.get(key)
    if o is None:
        from .graph import degree_order
        o = g._plans[key] = degree_order(g, rows=False, prefix=prefix)
    return o


def column_order(g: CsrGraph, feat: int, elem_size: int = 4):
    """The cached ``DegreeOrder(rows=False)`` of ``g`` when a feat-wide SpMM over it (rows of
    ``elem_size``-byte elements) would take the XCD-sliced hub path (else None)."""
    if not (DEGREE_ORDER and XCD_DIRECT) or g.nnz < XCD_MIN_NNZ or g._plans.get("_degree_ordered"):
        return None
    if xcd_hub_rows_for(g.n_cols, feat, elem_size) < 8 * XCD_PHASES:
        return None
    return _cached_column_order(g)


def gat_column_order(g: CsrGraph, heads: int, fh: int):
    """The cached ``DegreeOrder(rows=False)`` of ``g`` when the GAT aggregation over it would
    stage hub rows of Wh / er (``hub_rows_for``; else None): over A P^T those rows are the
    first rows of the projection's column-ordered output, read in place."""
    if not (DEGREE_ORDER and XCD_DIRECT) or g.nnz == 0 or g._plans.get("_degree_ordered"):
        return None
    if hub_rows_for(g.n_cols, heads * fh + heads) == 0:
        return None
    return _cached_column_order(g)


# Training (forward + backward) over P A P^T: every node relabelled once by degree, so the hub
# rows of every gathered table (X / S, Wh / er, dY / dout) are its first rows in the forward and
# in both backward passes, read in place (XCD-direct hub plans, no staging copy). The models
# (GATBase.forward, GCN_Model.forward) permute their input once on entry and the logits once
# on exit. cfg3 8-head GAT block: 3.89 -> 3.41 ms, node pass 1.16 -> 0.84 ms
# (profiles/r06c_gat_order_ab.log, tools/gat_order_ab.py).
GAT_TRAIN_ORDER = True
GCN_TRAIN_ORDER = True


def node_order(g: CsrGraph):
    """The cached ``DegreeOrder(rows=True)`` of a symmetric square graph: P A P^T, itself
    symmetric (marked so: backward passes walk it as its own transpose) and marked
    ``_degree_ordered`` (column_order / gat_column_order then return None for it: its hub rows
    already lead every table). Each row's edges keep their CSR order, renamed: the row sums run
    in the same order as over A."""
    o = g._plans.get(("_nodeorder",))
    if o is None:
        from .graph import degree_order
        o = degree_order(g, rows=True)
        o.graph.symmetric = True  # P A P^T of a symmetric A
        o.graph._plans["_degree_ordered"] = True
        g._plans[("_nodeorder",)] = o
    return o


# GCN_Model in training: a first layer over input features that need no gradient reads X in
# its original row order through P A (rows relabelled, column ids as in A) instead of
# permuting X onto P A P^T first (one [n, F] gather pass fewer; its SpMM stages the hub rows)
GCN_FIRST_ROWS = True


def row_order_graph(g: CsrGraph) -> CsrGraph:
    """P A for ``node_order(g)``'s P: row i is A's row perm[i] with its edges as in A (column ids
    not renamed), cached on g. A layer over it maps X in the original order to output rows in
    the degree order."""
    rg = g._plans.get(("_nodeorder_rows",))
    if rg is None:
        o = node_order(g)
        n = g.n_rows
        deg = g.rowptr[1:] - g.rowptr[:-1]
        nd = deg.index_select(0, o.perm)
        rp = torch.zeros(n + 1, dtype=torch.int64, device=g.rowptr.device)
        torch.cumsum(nd, 0, out=rp[1:])
        src = torch.repeat_interleave(g.rowptr[:-1].index_select(0, o.perm) - rp[:-1], nd,
                                      output_size=g.nnz)
        src += torch.arange(g.nnz, dtype=torch.int64, device=src.device)
        rg = CsrGraph(rp, g.col.index_select(0, src).contiguous(),
                      g.val.index_select(0, src).contiguous(), n, g.n_cols)
        del src
        g._plans[("_nodeorder_rows",)] = rg
    return rg


def _orderable(g: CsrGraph) -> bool:
    return (DEGREE_ORDER and g.nnz > 0 and g.symmetric and g.n_rows == g.n_cols
            and g.col.is_cuda and not g._plans.get("_degree_ordered"))


def gat_train_order(g: CsrGraph, heads: int, fh: int):
    """``node_order(g)`` when GAT training over it pays: a symmetric graph whose Wh / er table
    is large enough to stage hub rows (else None)."""
    if not (GAT_TRAIN_ORDER and _orderable(g)) or hub_rows_for(g.n_cols, heads * fh + heads) == 0:
        return None
    return node_order(g)


def gcn_train_order(g: CsrGraph, feat: int):
    """``node_order(g)`` when GCN training over it pays: a symmetric graph whose feat-wide
    SpMM takes the XCD-sliced hub path (else None)."""
    if not (GCN_TRAIN_ORDER and _orderable(g)) or column_order(g, feat) is None:
        return None
    return node_order(g)


def permute_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x[idx] for a 2-D fp32 device tensor and int64 row ids from a permutation, unchecked (no
    host read of the error flag: the training steps run it 2-4 times per step; the checked
    ``gather_rows`` below synced the host each time) (gnn_gather_rows_f32: 16-B row
    pieces per lane; torch's index_select moved the 1M x 128 permutation at ~1.7 TB/s,
    profiles/r06i_*); other inputs take index_select."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
            and idx.dtype == torch.int64 and idx.is_cuda and idx.dim() == 1):
        return x.index_select(0, idx)
    idx = idx.contiguous()
    out = torch.empty((idx.numel(), x.shape[1]), dtype=torch.float32, device=x.device)
    err = _err_flag(x.device, False)  # ids come from a permutation: the flag is never read
    _lib.check(_lib.load().gnn_gather_rows_f32(x.data_ptr(), x.stride(0), x.shape[0],
                                               idx.data_ptr(), idx.numel(), x.shape[1],
                                               out.data_ptr(), out.stride(0), err.data_ptr(),
                                               _lib.stream_handle(x.device)),
               "gnn_gather_rows_f32")
    return out


class PermuteRows(torch.autograd.Function):
    """y = x[perm] with the gradient gathered back through inv (a permutation: no index_add):
    the models' one relabelling on entry to and exit from the degree-ordered graph."""

    @staticmethod
    def forward(ctx, x, perm, inv):
        ctx.inv = inv
        return permute_rows(x, perm)

    @staticmethod
    def backward(ctx, gy):
        return permute_rows(gy.contiguous(), ctx.inv), None, None


# F.dropout (GAT/models/GAT.py:15,17) in training as gnn_dropout_rows_f32: a hashed element mask
# that is never stored, fused with the entry relabelling where there is one. torch's dropout
# wrote a byte mask beside its output and read it back in the backward (~0.1 ms forward +
# ~0.08 ms backward per [1M, 64] at cfg3, profiles/r06y_*).
HASHED_DROPOUT = True


def dropout_rows(x: torch.Tensor, p: float, seed: int, idx: torch.Tensor | None = None,
                 key_by_source: bool = False) -> torch.Tensor:
    """out[i] = x[r] with r = idx[i] (or i), element (i, c) kept iff the (seed, key, c) hash clears
    p (key = r when ``key_by_source``, else i), kept values scaled by 1 / (1 - p). Unchecked ids
    (they come from a permutation)."""
    n = idx.numel() if idx is not None else x.shape[0]
    out = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
    if idx is not None:
        idx = idx.contiguous()
    _lib.check(_lib.load().gnn_dropout_rows_f32(
        x.data_ptr(), x.stride(0), x.shape[0], idx.data_ptr() if idx is not None else None,
        int(key_by_source), n, x.shape[1], float(p), int(seed) & (2 ** 64 - 1), out.data_ptr(),
        out.stride(0), _err_flag(x.device, False).data_ptr(), _lib.stream_handle(x.device)),
        "gnn_dropout_rows_f32")
    return out


class DropoutRows(torch.autograd.Function):
    """y = dropout(x[perm]) (perm None: y = dropout(x)) with the hashed mask keyed by y's row; the
    gradient dx[j] = mask(inv[j]) dy[inv[j]] / (1 - p) re-derives the mask through inv."""

    @staticmethod
    def forward(ctx, x, p, seed, perm, inv):
        ctx.cfg = (p, seed, inv)
        return dropout_rows(x, p, seed, perm)

    @staticmethod
    def backward(ctx, gy):
        p, seed, inv = ctx.cfg
        gx = dropout_rows(gy.contiguous(), p, seed, inv, key_by_source=inv is not None)
        return gx, None, None, None, None


def hashed_dropout_ok(x: torch.Tensor, p: float) -> bool:
    """The hashed kernel takes F.dropout(x, p) in training: 2-D fp32 device rows with unit column
    stride, 0 < p < 1."""
    return (0.0 < p < 1.0 and HASHED_DROPOUT and x.dim() == 2 and x.is_cuda
            and x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) >= x.shape[1])


def model_dropout(x: torch.Tensor, p: float, training: bool, perm=None, inv=None):
    """F.dropout(x[perm] or x, p, training) on the hashed kernel where it applies
    (``hashed_dropout_ok``), else PermuteRows + torch's dropout."""
    ok = training and hashed_dropout_ok(x, p)
    if not ok:
        if perm is not None:
            x = PermuteRows.apply(x, perm, inv)
        return torch.nn.functional.dropout(x, p, training=training)
    return DropoutRows.apply(x, p, dropout_seed(), perm, inv)


def _spmm_items_call(items: CsrGraph, x, feat, part, stream) -> bool:
    """Pass 1 on gnn_spmm_items_f32. False (nothing launched) when the switch is off or the
    entry does not cover the call -- bf16 rows, another width, an odd pitch or alignment: the
    caller then runs the plain kernel."""
    if not SPMM_ITEMS_KERNEL or x.dtype != torch.float32:
        return False
    rc = _lib.invoke("gnn_spmm_items_f32", rowptr=items.rowptr.data_ptr(),
                     col=items.col.data_ptr(), val=items.val.data_ptr(), n_pos=items.n_rows,
                     x=x.data_ptr(), ldx=x.stride(0), feat=feat, part=part.data_ptr(),
                     ldp=part.stride(0), stream=stream)
    if rc == _lib.E_UNSUPPORTED:
        return False
    _lib.check(rc, "gnn_spmm_items_f32")
    return True


def _spmm_xcd_direct(xp, x, feat, bias, out, seg, skip_empty, flags, stream):
    """The XCD-sliced SpMM of a degree-ordered graph (graph.degree_order): the hub rows are
    X's first k rows, so there is no staging copy. Pass 1 (the items kernel, or the plain
    kernel where that does not apply) reads the items' hub rows from X into a partial-row
    buffer; pass 2 reads X and that buffer (c < 0 -> partial row -1-c). The partial rows are
    fp32 for a bf16 X too (the bf16 hub / tasks entries with an fp32 xh)."""
    items, rest = xp.direct()
    part = torch.empty((xp.n_pos, feat), dtype=torch.float32, device=x.device)
    p1 = items.plan(seg)
    if p1.n_seg or p1.n_small:
        raise RuntimeError("XCD hub plan: item rows outside the mid-row class")
    if not _spmm_items_call(items, x, feat, part, stream):
        _spmm_plain_call(items, p1, False, x, feat, None, part, feat, None, 0, stream)
    if _tasks_ok(feat, x, out, bias, part):
        tp = rest.task_plan(seg, TASK_MAX_DEG, _task_cost(feat))
        partial = None
        if tp.base.n_seg:
            partial = torch.empty((tp.base.n_seg, feat), dtype=torch.float32, device=x.device)
        _spmm_tasks_call(rest, rest.col, tp, x, part, feat, bias, out, out.stride(0), partial,
                         flags | (_lib.EPI_SKIP_EMPTY if skip_empty else 0), stream)
        return
    p2 = staged_plan(rest, seg)
    partial = None
    if p2.n_seg:
        partial = torch.empty((p2.n_seg, feat), dtype=torch.float32, device=x.device)
    _spmm_hub_call(rest, rest.col, p2, skip_empty, x, part, feat, bias, out, out.stride(0),
                   partial, flags, stream)


class _SpmmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, g):
        ctx.g = g
        ctx.has_bias = bias is not None
        return spmm_forward(g, x, bias)

    @staticmethod
    def backward(ctx, gy):
        g = ctx.g
        gx = gb = None
        if ctx.needs_input_grad[0]:
            gx = spmm_forward(g.transpose(), gy.contiguous())  # dX = A^T dY (same kernel)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            gb = gy.sum(0)
        return gx, gb, None


def spmm(g: CsrGraph, x: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Differentiable (w.r.t. X and bias) CSR SpMM on the device. bf16 rows are an inference
    storage type (``spmm_forward``): a bf16 tensor that requires grad raises TypeError."""
    if torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.requires_grad:
        raise TypeError("spmm: bfloat16 X is supported at inference only; training runs in "
                        "fp32 (gradients flow through float32 feature rows)")
    if torch.is_grad_enabled() and (x.requires_grad or (bias is not None and bias.requires_grad)):
        return _SpmmFn.apply(x, bias, g)
    return spmm_forward(g, x, bias)


def gemm_tn(a: torch.Tensor, b: torch.Tensor, d: torch.Tensor | None = None,
            trans: bool = False):
    """(A^T B, column sums of D) over the row axis (gnn_gemm_tn_f32): the weight / bias
    gradients of the training step. ``trans``: return (A^T B)^T = B^T A. None when the shape is
    not covered (the caller uses torch.mm)."""
    _require_device(a, b, d)
    if (a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or b.dim() != 2
            or a.shape[0] != b.shape[0] or (d is not None and d.shape != b.shape)):
        return None
    n, m = a.shape
    k = b.shape[1]
    lib = _lib.load()
    kind = lib.gnn_gemm_tn_supported(m, k)  # 1 wide, 2 narrow (k <= 16: classifier layers)
    if not kind:
        return None

    def fits(t):
        # rows that overlap (a row stride below the row length: an expanded row, an as_strided
        # window) are copied out; a single row has no second row to overlap
        if n > 1 and t.stride(0) < t.shape[1]:
            return False
        if kind == 2:  # narrow shapes: any row stride, unit column stride
            return (t.stride(1) == 1 or t.shape[1] == 1) and t.data_ptr() % 4 == 0
        return t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0

    # a copy for an operand the kernel cannot read in place: clone, not .contiguous(), which
    # hands back a contiguous view at a misaligned storage offset unchanged
    ts = [t if fits(t) else t.clone(memory_format=torch.contiguous_format)
          for t in [a, b] + ([d] if d is not None else [])]
    if not all(fits(t) for t in ts):  # rows of a length the 16-B loads cannot take
        return None
    a, b = ts[0], ts[1]
    d = ts[2] if d is not None else None
    c = torch.empty((k, m) if trans else (m, k), dtype=torch.float32, device=a.device)
    dsum = torch.empty(k, dtype=torch.float32, device=a.device) if d is not None else None
    ws = torch.empty(int(lib.gnn_gemm_tn_workspace_bytes(n, m, k)), dtype=torch.uint8,
                     device=a.device)

    def ld(t):  # the row stride; of a single row (whose stride is never used) the row length
        return t.stride(0) if n > 1 else t.shape[1]

    _lib.check(lib.gnn_gemm_tn_f32(a.data_ptr(), ld(a), b.data_ptr(), ld(b), n, m, k,
                                   c.data_ptr(), c.stride(0), 1 if trans else 0, _lib.ptr(d),
                                   ld(d) if d is not None else 0, _lib.ptr(dsum),
                                   ws.data_ptr(), ws.numel(), _lib.stream_handle(a.device)),
               "gnn_gemm_tn_f32")
    return c, dsum


def _masked_grad(gy: torch.Tensor, h: torch.Tensor, scale: float) -> torch.Tensor:
    """gy . [h > 0] * scale as a product (what the Dropout backward computes: dy * mask), so a
    NaN gradient stays NaN at a masked element; the masked gemm_tn kernel forms the same."""
    return gy * torch.where(h > 0, float(scale), 0.0).to(gy.dtype)


def gemm_tn_masked(a: torch.Tensor, b: torch.Tensor, h: torch.Tensor, scale: float,
                   want_dsum: bool, trans: bool = False):
    """(A^T B', column sums of B' if want_dsum) for B' = B . [H > 0] * scale
    (gnn_gemm_tn_masked_f32): the weight / bias gradients behind a fused ReLU + dropout epilogue
    whose output is H. Where the kernel does not take the shape, B' is formed with torch and
    handed to ``gemm_tn`` (None if that does not take it either)."""
    _require_device(a, b, h)
    lib = _lib.load()
    n, m = a.shape
    k = b.shape[1]
    ok = (a.dtype == b.dtype == h.dtype == torch.float32 and h.shape == b.shape
          and lib.gnn_gemm_tn_masked_supported(m, k)
          and all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
                  and t.stride(0) >= t.shape[1]  # no overlapping rows (expanded, as_strided)
                  for t in (a, b, h)))
    if not ok:
        bm = _masked_grad(b, h, scale)
        return gemm_tn(a, bm, bm if want_dsum else None, trans=trans)
    c = torch.empty((k, m) if trans else (m, k), dtype=torch.float32, device=a.device)
    dsum = torch.empty(k, dtype=torch.float32, device=a.device) if want_dsum else None
    ws = torch.empty(int(lib.gnn_gemm_tn_workspace_bytes(n, m, k)), dtype=torch.uint8,
                     device=a.device)
    _lib.check(lib.gnn_gemm_tn_masked_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                          h.data_ptr(), h.stride(0), float(scale), n, m, k,
                                          c.data_ptr(), c.stride(0), 1 if trans else 0,
                                          _lib.ptr(dsum), ws.data_ptr(), ws.numel(),
                                          _lib.stream_handle(a.device)), "gnn_gemm_tn_masked_f32")
    return c, dsum


LINEAR_SMALL_MAX_FOUT = 64  # widest output the k <= 16 kernel takes by default


def linear_small(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor | None:
    """x @ w^T with one narrow side (gnn_linear_small_f32: fout <= 16 on fp32 MFMA rows, or
    k <= 16 on a broadcast kernel) -- the classifier layer's support and its dX; None when the
    shape is not covered."""
    _require_device(x, w)
    if (x.dtype != torch.float32 or w.dtype != torch.float32 or x.dim() != 2 or w.dim() != 2
            or x.shape[1] != w.shape[1]):
        return None
    lib = _lib.load()
    fout, k = w.shape
    kind = lib.gnn_linear_small_supported(k, fout)
    # the broadcast kernel (k <= 16) beat hipBLASLt at fout 64 (GAT out_att dX: 0.055 vs 0.120
    # ms) but not at 128 inside the GCN_Model step (0.189 vs 0.146 ms,
    # profiles/r06y_gcn_model_train_step_kernel_stats.csv): 128 and 256 stay on torch.mm
    if not kind or (kind == 2 and fout > LINEAR_SMALL_MAX_FOUT):
        return None
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16 or x.stride(0) < k:
        # rows copied to a 16-B aligned pitch (a multiple of 4 floats >= k)
        xp = torch.empty((x.shape[0], k + (-k) % 4), dtype=torch.float32, device=x.device)
        xp[:, :k] = x
        x = xp[:, :k]
    w = w.contiguous()
    y = torch.empty((x.shape[0], fout + (-fout) % 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.gnn_linear_small_f32(x.data_ptr(), x.stride(0), x.shape[0], k, w.data_ptr(),
                                        fout, y.data_ptr(), y.stride(0),
                                        _lib.stream_handle(x.device)), "gnn_linear_small_f32")
    return y[:, :fout] if y.shape[1] != fout else y


def _transform_or_mm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x @ w^T: the MFMA transform where it covers the shape, the narrow kernels where one side
    is narrow (linear_small), else torch.mm (hipBLASLt)."""
    y = gcn_transform(x, w)
    if y is None:
        y = linear_small(x, w)
    return y if y is not None else torch.mm(x, w.t())


# A layer with in_features <= out_features trains as (A X) W^T + b: the same product as the
# reference's A (X W^T) + b (GCN/GCN.py:42-45), reassociated. The SpMM then gathers rows of X
# instead of the support (no wider), and the backward needs dY and Z = A X only: dW = dY^T Z
# and db = sum dY come out of ONE gemm_tn pass over (Z, dY) (dY read once, not next to dS and
# X), and where X needs no gradient -- a first layer over the input features -- the backward
# runs no SpMM at all (the A (X W^T) form needs dS = A^T dY for dW regardless).
GCN_REASSOC = True
# the A (X W^T) form zero-pads an output width below 64 to a multiple of 4 (see _GcnLayerFn)
GCN_PAD_NARROW = True


# The reassociated backward's dW / db pass (gemm_tn over Z and dY) and its dX chain (transform
# dZ = dY W, then the SpMM A^T dZ) read the same dY and nothing of each other: when X needs a
# gradient the weight pass runs on a side stream beside the chain (the SpMM is bound by gather
# latency and leaves the matrix cores and VALUs idle).
GCN_OVERLAP_DW = True  # tools/train_step_probe.py --set: 2.49-2.53 vs 2.51-2.64 ms at cfg2
_SIDE_STREAMS: dict = {}


def _side_stream(dev: torch.device) -> torch.cuda.Stream:
    s = _SIDE_STREAMS.get(dev.index)
    if s is None:
        s = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
    return s


def _reassociate(x, weight, g) -> bool:
    fout, fin = weight.shape
    return GCN_REASSOC and fin <= fout and x.shape[0] == g.n_cols


# GCN_Model's Graph_conv_layer -> ReLU -> Dropout run in training as ONE op when the layer takes
# the (A X) W^T + b form: ReLU and dropout in the transform's store epilogue, their backward
# folded into the weight-gradient pass (gemm_tn_masked) -- two elementwise passes forward and
# two backward fewer over the [n, hidden] activations
GCN_FUSE_RELU_DROPOUT = True


def fuses_relu_dropout(x, weight, g) -> bool:
    """Whether ``gcn_layer(..., relu_dropout=...)`` applies to this layer: the reassociated form
    (``_reassociate``) on a shape ``gcn_transform`` takes (its own conditions, restated)."""
    fout, fin = weight.shape
    return (GCN_FUSE_RELU_DROPOUT and _reassociate(x, weight, g)
            and x.dtype == torch.float32 and weight.dtype == torch.float32
            and bool(_lib.load().gnn_gcn_transform_supported(fin, fout))
            and not (fout == 256 and fin > 64 and not TRANSFORM_WIDE_MFMA))


def dropout_seed() -> int:
    """A 62-bit seed for the HIP kernels' hashed dropout, drawn from torch's CPU generator (so
    torch.manual_seed fixes it)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class _GcnLayerFn(torch.autograd.Function):
    """Graph_conv_layer (GCN/GCN.py:41-47) as one differentiable op, trained the way the
    reference's loop runs it (GCN/train_eval.py:43-48: forward, loss.backward()). Two forms:

    A (X W^T) + b (in_features > out_features: the narrower SpMM)
      forward   S = X W^T on the MFMA transform -- scattered into the column-degree order of
                A P^T when the graph takes that path (``column_order``), as at inference --
                then Y = A S + b (the forward SpMM path, bias in its epilogue);
      backward  dS = A^T dY (the same SpMM kernels; A itself when it is symmetric, as the GCN
                normalisation is: no transposed copy), dX = dS W on the MFMA transform,
                dW = dS^T X and db = the column sums of dY in one pass (gnn_gemm_tn_f32, a
                K = n_rows reduction: 1.81 ms on hipBLASLt at cfg2). S is not kept.
    (A X) W^T + b (in_features <= out_features, ``GCN_REASSOC``)
      forward   Z = A X (the SpMM over X), Y = Z W^T + b (the transform, bias in its store
                epilogue: gnn_gcn_transform_epi_f32); Z is kept for backward;
      backward  dW = dY^T Z and db = the column sums of dY in one gemm_tn pass that reads dY
                once (d = b), and only when X needs a gradient dZ = dY W (transform) and
                dX = A^T dZ (SpMM).
    The two forms agree to fp32 rounding (a sum of products regrouped).

    ``relu_dropout`` = (p, seed), reassociated form only (``fuses_relu_dropout``): the output
    is H = dropout_p(ReLU(Y)) -- GCN_Model's ReLU and Dropout after the layer (GCN/GCN.py:12-14)
    -- from the transform's epilogue (hashed dropout: element (i, c) kept iff the (seed, i, c)
    hash clears p); H is kept, and the backward's upstream gradient passes exactly where
    H > 0, scaled by 1 / (1 - p): folded into the dW / db pass (gemm_tn_masked), formed
    explicitly only when X needs a gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, g, relu_dropout=None):
        ctx.g = g
        ctx.has_bias = bias is not None
        ctx.reassoc = _reassociate(x, weight, g)
        ctx.relu_dropout = relu_dropout
        if relu_dropout is not None:
            if not fuses_relu_dropout(x, weight, g):
                raise ValueError("relu_dropout= needs the reassociated form on a transform shape")
            p, seed = relu_dropout
            z = spmm_forward(g, x)
            h = gcn_transform(z, weight, relu=True, bias=bias, dropout_p=p, seed=seed)
            ctx.save_for_backward(z, weight, h)
            return h
        if ctx.reassoc:
            z = spmm_forward(g, x)
            y = gcn_transform(z, weight, bias=bias)
            if y is None:
                y = torch.mm(z, weight.t()) if bias is None else torch.addmm(bias, z, weight.t())
            ctx.save_for_backward(z, weight)
            return y
        # an output width that is not a multiple of 4 (a classifier layer: 7 classes) is
        # zero-padded to one: the SpMMs then gather 16-B pieces of the support / dY rows in
        # packed row tasks (7 -> 8 at cfg2: 0.30 -> 0.27 ms per SpMM pass), the support and dX
        # products take the narrow kernels (linear_small)
        fout = weight.shape[0]
        ctx.pad = (-fout) % 4 if GCN_PAD_NARROW and fout < 64 else 0
        if ctx.pad:
            weight = torch.nn.functional.pad(weight, (0, 0, 0, ctx.pad))
            bias = torch.nn.functional.pad(bias, (0, ctx.pad)) if bias is not None else None
        order = column_order(g, weight.shape[0]) if x.shape[0] == g.n_cols else None
        s = None
        if order is not None:
            s = gcn_transform(x, weight, out_rows=order.inv, check_rows=False)
        if s is not None:
            y = spmm_forward(order.graph, s, bias)
        else:
            y = spmm_forward(g, _transform_or_mm(x, weight), bias)
        ctx.save_for_backward(x, weight)
        return y[:, :fout] if ctx.pad else y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        gx = gw = gb = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.relu_dropout is not None:
            z, weight, h = ctx.saved_tensors
            scale = 1.0 / (1.0 - ctx.relu_dropout[0])
            if ctx.needs_input_grad[1]:
                r = gemm_tn_masked(z, gy, h, scale, want_b, trans=True)
                if r is not None:
                    gw, gb = r
            dy = None
            if (ctx.needs_input_grad[1] and gw is None) or (want_b and gb is None) \
                    or ctx.needs_input_grad[0]:
                dy = _masked_grad(gy, h, scale)
            if ctx.needs_input_grad[1] and gw is None:
                gw = torch.mm(dy.t(), z)
            if want_b and gb is None:
                gb = dy.sum(0)
            if ctx.needs_input_grad[0]:
                gx = spmm_forward(ctx.g.transpose(), _transform_or_mm(dy, weight.t().contiguous()))
            return gx, gw, gb, None, None
        x, weight = ctx.saved_tensors  # Z = A X in the reassociated form
        if ctx.reassoc:
            main = side = None
            if GCN_OVERLAP_DW and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
                main = torch.cuda.current_stream(gy.device)
                side = _side_stream(gy.device)
                side.wait_stream(main)
            if ctx.needs_input_grad[1]:
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    # dW = dY^T Z as (Z^T dY)^T; db = the column sums of dY from the same loads
                    r = gemm_tn(x, gy, gy if want_b else None, trans=True)
                    if r is not None:
                        gw, gb = r
                    else:
                        gw = torch.mm(gy.t(), x)
                    if want_b and gb is None:
                        gb = gy.sum(0)
                if side is not None:  # read there: not recycled before the side work is done
                    x.record_stream(side)
                    gy.record_stream(side)
            if want_b and gb is None:
                gb = gy.sum(0)
            if ctx.needs_input_grad[0]:
                gx = spmm_forward(ctx.g.transpose(), _transform_or_mm(gy, weight.t().contiguous()))
            if side is not None:
                main.wait_stream(side)
                for t in (gw, gb):
                    if t is not None:
                        t.record_stream(main)
            return gx, gw, gb, None, None
        if ctx.pad:
            gy = torch.nn.functional.pad(gy, (0, ctx.pad))
        ds = spmm_forward(ctx.g.transpose(), gy)
        if ctx.needs_input_grad[0]:
            gx = _transform_or_mm(ds, weight.t().contiguous())
        if ctx.needs_input_grad[1]:
            # dW = dS^T X as (X^T dS)^T, with db = the column sums of dY read in the same pass
            r = gemm_tn(x, ds, gy if want_b else None, trans=True)
            if r is not None:
                gw, gb = r
            else:
                gw = torch.mm(ds.t(), x)
        if want_b and gb is None:
            gb = gy.sum(0)
        if ctx.pad:
            fout = weight.shape[0] - ctx.pad
            gw = gw[:fout] if gw is not None else None
            gb = gb[:fout] if gb is not None else None
        return gx, gw, gb, None, None


def gcn_layer(g: CsrGraph, x: torch.Tensor, weight: torch.Tensor,
              bias: torch.Tensor | None = None, relu_dropout=None) -> torch.Tensor:
    """A_hat (x W^T) + b, differentiable w.r.t. x, W and b (``_GcnLayerFn``); with
    ``relu_dropout`` = (p, seed): dropout_p(ReLU(A_hat x W^T + b)) as one op (see
    _GcnLayerFn; requires ``fuses_relu_dropout``)."""
    _require_device(g.rowptr, x, weight, bias)
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("gcn_layer runs in float32")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] \
            or x.shape[0] != g.n_cols:
        raise ValueError("x must be [n_cols, F_in] and weight [F_out, F_in]")
    return _GcnLayerFn.apply(x, weight, bias, g, relu_dropout)


# ---------------------------------------------------------------------- GAT
GAT_DENSE = 0   # GraphAttentionLayer   (GAT/models/layers.py:22-37)
GAT_SPARSE = 1  # SpGraphAttentionLayer (GAT/models/layers.py:94-131)


def gat_logits(wh: torch.Tensor, heads: int, fh: int, a_src: torch.Tensor,
               a_dst: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """el[n,h] = a_src[h].Wh[n,h], er[n,h] = a_dst[h].Wh[n,h] (one HIP launch)."""
    _require_device(wh, a_src, a_dst)
    wh = _rows_f32(wh, "Wh")
    n = wh.shape[0]
    if wh.shape[1] != heads * fh or a_src.numel() != heads * fh or a_dst.numel() != heads * fh:
        raise ValueError("Wh / attention vectors do not match heads * fh")
    el = torch.empty((n, heads), dtype=torch.float32, device=wh.device)
    er = torch.empty((n, heads), dtype=torch.float32, device=wh.device)
    lib = _lib.load()
    _lib.check(lib.gnn_gat_logits_f32(wh.data_ptr(), wh.stride(0), n, heads, fh,
                                      a_src.contiguous().data_ptr(), a_dst.contiguous().data_ptr(),
                                      el.data_ptr(), er.data_ptr(), heads,
                                      _lib.stream_handle(wh.device)), "gnn_gat_logits_f32")
    return el, er


def gat_project(x: torch.Tensor, w: torch.Tensor, heads: int, fh: int, a_src: torch.Tensor,
                a_dst: torch.Tensor, packed: bool = False, col_rows: torch.Tensor | None = None):
    """(Wh = x @ w, el, er) in one MFMA pass (inference; no autograd), or None when the
    shape is not covered by gnn_gat_project_f32 (the caller then uses torch.mm +
    gat_logits). ``packed``: the three are views of ONE [n, H*Fh + 2H] buffer, rows
    [Wh | er | el], so the aggregation's er gather lands next to the Wh row it also
    gathers. Same output bits; measured neutral at cfg3 on a slow box (1.297 vs 1.298 ms,
    profiles/r01i_gat_pack_ab_slow.log), so it is not the default.

    ``col_rows`` (int64 [n], a permutation): Wh and er of node i go to row col_rows[i], el
    stays at row i (gnn_gat_project_rows_f32) -- the operands of the aggregation over a
    column-degree-ordered graph (``gat_column_order``; col_rows = its ``inv``)."""
    _require_device(x, w, a_src, a_dst)
    if (x.dtype != torch.float32 or w.dtype != torch.float32 or x.dim() != 2 or w.dim() != 2
            or x.shape[1] != w.shape[0] or w.shape[1] != heads * fh):
        return None
    lib = _lib.load()
    k, fout = w.shape
    if not lib.gnn_gat_project_supported(k, fout, fh):
        return None
    if not _rows16(x) or x.stride(0) < k:  # rows the 16-B loads cannot take, or that overlap
        x = x.clone(memory_format=torch.contiguous_format)
    n = x.shape[0]
    if col_rows is not None:
        _require_device(col_rows)
        if packed:
            raise ValueError("col_rows= needs separate el / er buffers (packed=False)")
        if col_rows.dtype != torch.int64 or col_rows.shape != (n,):
            raise TypeError("col_rows must be int64 [rows of x]")
        col_rows = col_rows.contiguous()
    if packed:
        buf = torch.empty((n, fout + 2 * heads), dtype=torch.float32, device=x.device)
        wh, er, el = buf[:, :fout], buf[:, fout:fout + heads], buf[:, fout + heads:]
    else:
        wh = torch.empty((n, fout), dtype=torch.float32, device=x.device)
        el = torch.empty((n, heads), dtype=torch.float32, device=x.device)
        er = torch.empty((n, heads), dtype=torch.float32, device=x.device)
    if col_rows is not None:
        _lib.check(lib.gnn_gat_project_rows_f32(
            x.data_ptr(), x.stride(0), n, k, w.contiguous().data_ptr(), fout,
            a_src.contiguous().data_ptr(), a_dst.contiguous().data_ptr(), heads, fh,
            wh.data_ptr(), wh.stride(0), el.data_ptr(), er.data_ptr(), el.stride(0),
            col_rows.data_ptr(), None, _lib.stream_handle(x.device)),
            "gnn_gat_project_rows_f32")
        return wh, el, er
    _lib.check(lib.gnn_gat_project_f32(
        x.data_ptr(), x.stride(0), n, k, w.contiguous().data_ptr(), fout,
        a_src.contiguous().data_ptr(), a_dst.contiguous().data_ptr(), heads, fh, wh.data_ptr(),
        wh.stride(0), el.data_ptr(), er.data_ptr(), el.stride(0), None,
        _lib.stream_handle(x.device)), "gnn_gat_project_f32")
    return wh, el, er


# fout = 256 at k > 64 (cfg5's 256 -> 256 layer) runs as ONE 8-wave x 2-block launch, faster
# than hipBLASLt (10M x 256 -> 256: 9.63 vs 9.95 ms, profiles/r03o_transform_one256_ab.log; the
# round-3 two-launch form lost, 10.57 ms); False keeps those shapes on nn.Linear
TRANSFORM_WIDE_MFMA = True


TRANSFORM_PRECISIONS = ("split-bf16", "fp32-mfma")


def transform_precision() -> str:
    """The MFMA transforms' arithmetic at K >= 128 and of the GAT projection at K = 64 (see
    set_transform_precision), read back from the library (gnn_transform_get_precision), so a
    direct C call to gnn_transform_set_precision is seen too."""
    return TRANSFORM_PRECISIONS[0] if _lib.load().gnn_transform_get_precision() == 1 \
        else TRANSFORM_PRECISIONS[1]


def set_transform_precision(mode: str) -> str:
    """Arithmetic of the MFMA transforms at K >= 128 and of the GAT projection at K = 64
    (gnn_transform_set_precision, process-wide), returns the previous mode: 'split-bf16'
    (default: fp32 products from three-piece bf16 splits on v_mfma_f32_16x16x32_bf16, a few
    fp32 ulps per product) or 'fp32-mfma' (v_mfma_f32_16x16x4_f32, a k-ordered fp32 fmaf
    chain)."""
    if mode not in TRANSFORM_PRECISIONS:
        raise ValueError(f"transform precision must be one of {TRANSFORM_PRECISIONS}")
    prev = _lib.load().gnn_transform_set_precision(0 if mode == "fp32-mfma" else 1)
    return TRANSFORM_PRECISIONS[0] if prev == 1 else TRANSFORM_PRECISIONS[1]


def gcn_transform(x: torch.Tensor, weight: torch.Tensor, relu: bool = False,
                  out: torch.Tensor | None = None, out_rows: torch.Tensor | None = None,
                  check_rows: bool = True, live: torch.Tensor | None = None,
                  bias: torch.Tensor | None = None, dropout_p: float = 0.0,
                  seed: int = 0, out_dtype: torch.dtype = torch.float32) -> torch.Tensor | None:
    """support = x @ weight^T on fp32 MFMA (gnn_gcn_transform_f32), the dense half of
    Graph_conv_layer.forward (GCN/GCN.py:42); ``relu=True``: max(x @ weight^T, 0)
    (gnn_linear_relu_f32, the SageLayer at GraphSAGE/GraphSAGE.py:18-20). Inference only
    (no autograd). None when the shape is not covered (the caller then uses nn.Linear /
    hipBLASLt).

    ``out_rows`` (int64 [rows of x]): x row i goes to support row out_rows[i]
    (gnn_gcn_transform_rows_f32), e.g. a degree order's ``inv`` so that the support is in the
    degree-ordered graph's column order; ``out`` (or a new [rows of x, fout] tensor) receives
    it; the ids must not repeat (two rows stored to one support row leave either).
    ``check_rows=False`` skips the host read of the range-check flag (trusted ids, e.g. a
    ``DegreeOrder``'s; the kernel still skips the store of a bad id).

    ``live`` (with ``relu=True``): a device int64 scalar; only rows [0, min(live, rows of x))
    are computed (gnn_linear_relu_live_f32) -- a sampled batch's frontier whose size the host
    never read; the other output rows are left as they were.

    ``bias`` (fp32 [fout]) and ``dropout_p`` / ``seed`` (without out_rows / live):
    dropout(act(x @ weight^T + bias)) in the store epilogue (gnn_gcn_transform_epi_f32; act =
    ReLU if ``relu``; element (i, c) kept iff the (seed, i, c) hash clears p, kept values scaled
    by 1 / (1 - p)).

    ``out_dtype=torch.bfloat16`` (or a bfloat16 ``out``, whose dtype decides): the result is
    stored as bf16 by the kernel's store epilogue (gnn_gcn_transform_bf16out /
    _rows_bf16out; round to nearest even of exactly the fp32 value, NaN and +-inf kept) --
    the plain and ``out_rows`` forms only (no relu / live / bias / dropout)."""
    _require_device(x, weight)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"gcn_transform stores float32 or bfloat16 (got {out_dtype})")
    y16 = out_dtype == torch.bfloat16
    if (x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 2
            or weight.dim() != 2 or x.shape[1] != weight.shape[1]):
        return None
    lib = _lib.load()
    fout, k = weight.shape
    if not lib.gnn_gcn_transform_supported(k, fout):
        return None
    if fout == 256 and k > 64 and not TRANSFORM_WIDE_MFMA:
        return None
    if out_rows is not None and relu:
        raise ValueError("out_rows= is supported without the ReLU epilogue only")
    epi = bias is not None or dropout_p > 0
    if y16 and (relu or epi or live is not None):
        raise ValueError("a bfloat16 result is supported without relu / live / bias / dropout")
    if epi and (out_rows is not None or live is not None):
        raise ValueError("bias= / dropout_p= are supported without out_rows / live only")
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError("dropout_p must be in [0, 1)")
    if bias is not None:
        _require_device(bias)
        if bias.dtype != torch.float32 or bias.numel() != fout:
            raise ValueError("bias must be float32 [fout]")
        bias = bias.contiguous()
        if bias.data_ptr() % 16:
            bias = bias.clone()
    if live is not None:
        _require_device(live)
        if not relu or out_rows is not None:
            raise ValueError("live= is supported with the ReLU epilogue (the SageLayer) only")
        if live.dtype != torch.int64 or live.numel() != 1:
            raise TypeError("live must be a one-element int64 device tensor")
    if not _rows16(x) or x.stride(0) < k:  # rows the 16-B loads cannot take, or that overlap
        x = x.clone(memory_format=torch.contiguous_format)
    w = weight.contiguous()
    m = x.shape[0]
    if out is None:
        out = torch.empty((m, fout), dtype=out_dtype, device=x.device)
    elif (out.dim() != 2 or out.shape[1] != fout or (out_rows is None and out.shape[0] != m)
          or out.stride(1) != 1 or out.stride(0) % 4 or out.data_ptr() % 16):
        raise ValueError("out must be float32 or bfloat16 [rows, fout], 16-B aligned rows")
    if out_rows is not None:
        _require_device(out_rows)
        if out_rows.dtype != torch.int64 or out_rows.dim() != 1 or out_rows.numel() != m:
            raise TypeError("out_rows must be a 1-D int64 tensor with one id per row of x")
        out_rows = out_rows.contiguous()
        if m == 0:
            return out
        err = torch.zeros(1, dtype=torch.int32, device=x.device)
        fn, name = ((lib.gnn_gcn_transform_rows_bf16out, "gnn_gcn_transform_rows_bf16out")
                    if y16 else (lib.gnn_gcn_transform_rows_f32, "gnn_gcn_transform_rows_f32"))
        _lib.check(fn(
            x.data_ptr(), x.stride(0), m, k, w.data_ptr(), fout, out.data_ptr(), out.stride(0),
            out_rows.data_ptr(), out.shape[0], err.data_ptr(), _lib.stream_handle(x.device)),
            name)
        if check_rows and int(err.item()):
            raise IndexError("gcn_transform: an output row id is out of range")
        return out
    if live is not None:
        _lib.check(lib.gnn_linear_relu_live_f32(
            x.data_ptr(), x.stride(0), x.shape[0], live.data_ptr(), k, w.data_ptr(), fout,
            out.data_ptr(), out.stride(0), _lib.stream_handle(x.device)),
            "gnn_linear_relu_live_f32")
        return out
    if epi:
        _lib.check(lib.gnn_gcn_transform_epi_f32(
            x.data_ptr(), x.stride(0), x.shape[0], k, w.data_ptr(), fout, _lib.ptr(bias),
            1 if relu else 0, float(dropout_p), int(seed) & (2 ** 64 - 1), out.data_ptr(),
            out.stride(0), _lib.stream_handle(x.device)), "gnn_gcn_transform_epi_f32")
        return out
    fn, name = ((lib.gnn_linear_relu_f32, "gnn_linear_relu_f32") if relu else
                (lib.gnn_gcn_transform_bf16out, "gnn_gcn_transform_bf16out") if y16 else
                (lib.gnn_gcn_transform_f32, "gnn_gcn_transform_f32"))
    _lib.check(fn(x.data_ptr(), x.stride(0), x.shape[0], k, w.data_ptr(), fout, out.data_ptr(),
                  out.stride(0), _lib.stream_handle(x.device)), name)
    return out


def linear_relu_classify(x: torch.Tensor, weight: torch.Tensor, wd: torch.Tensor,
                         bd: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """(y, logits) = (relu(x @ weight^T), y @ wd^T + bd) in ONE launch
    (gnn_linear_relu_cls_f32): the last SageLayer (GraphSAGE/GraphSAGE.py:18-20) with the
    classifier ``self.dense`` (GraphSAGE.py:51-52) in its epilogue. Inference only; None when
    the shape is not covered (more than 4 classes, or a transform shape gcn_transform does not
    take), and the caller then runs the two layers separately."""
    _require_device(x, weight, wd)
    fout, k = weight.shape
    n_cls = wd.shape[0] if wd.dim() == 2 else 0
    if (x.dtype != torch.float32 or weight.dtype != torch.float32 or wd.dtype != torch.float32
            or x.dim() != 2 or x.shape[1] != k or wd.dim() != 2 or wd.shape[1] != fout
            or fout > 128
            or not 1 <= n_cls <= 4 or (bd is not None and (bd.dtype != torch.float32
                                                            or bd.numel() != n_cls))):
        return None
    lib = _lib.load()
    if not lib.gnn_gcn_transform_supported(k, fout) or (fout == 256 and k > 64
                                                         and not TRANSFORM_WIDE_MFMA):
        return None
    if bd is not None:
        _require_device(bd)
        bd = bd.contiguous()
    if not _rows16(x) or x.stride(0) < k:  # rows the 16-B loads cannot take, or that overlap
        x = x.clone(memory_format=torch.contiguous_format)
    w, wdc = weight.contiguous(), wd.contiguous()
    m = x.shape[0]
    if out is None:
        out = torch.empty((m, fout), dtype=torch.float32, device=x.device)
    elif (out.shape != (m, fout) or out.dtype != torch.float32 or out.device != x.device
          or out.stride(1) != 1 or out.stride(0) % 4 or out.data_ptr() % 16):
        raise ValueError("out must be float32 [rows, fout] on x's device, 16-B aligned rows")
    logits = torch.empty((m, n_cls), dtype=torch.float32, device=x.device)
    _lib.check(lib.gnn_linear_relu_cls_f32(
        x.data_ptr(), x.stride(0), m, k, w.data_ptr(), fout, out.data_ptr(), out.stride(0),
        wdc.data_ptr(), _lib.ptr(bd), n_cls, logits.data_ptr(), logits.stride(0),
        _lib.stream_handle(x.device)), "gnn_linear_relu_cls_f32")
    return out, logits


def col_mean(x: torch.Tensor) -> torch.Tensor:
    """Mean over rows (double accumulation) -- the dense GAT layer's edgeless-row output."""
    _require_device(x)
    x = _rows_f32(x, "x")
    lib = _lib.load()
    scratch = torch.empty(max(8, int(lib.gnn_col_mean_scratch_bytes(x.shape[0], x.shape[1]))),
                          dtype=torch.uint8, device=x.device)
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    _lib.check(lib.gnn_col_mean_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1],
                                    out.data_ptr(), scratch.data_ptr(),
                                    _lib.stream_handle(x.device)), "gnn_col_mean_f32")
    return out


GAT_SHORT_MAX_DEG = 16  # rows with 2..16 edges take the short-row path (A/B at cfg3: 16 best)
# Packed row tasks for the rows of degree <= GAT_SHORT_MAX_DEG (gnn_gat_csr_tasks_f32,
# gat.hip gat_packed_rows): runs of consecutive low-degree rows, edgeless and one-edge rows
# included, cut at GAT_TASK_COST edges + rows, one wave per task -- in place of the packed
# small rows and gat_short_kernel's four rows per wave. Built, tested, and slower at cfg3:
# aggregation 0.943-0.976 ms (cost 64-256) against 0.779 ms for the row classes
# (tools/gat_tasks_ab.py, profiles/r05b_gat_tasks_ab.log): the small-row path packs the 435K
# edgeless / one-edge rows far more cheaply than a task's per-row flush and per-edge softmax
# update. Opt-in.
GAT_TASKS = False
# er_j recomputed from the gathered Wh_j rows when gat_aggregate is given a_dst, instead of an
# er load per (edge, head group): 1.2 of the 4.1 GB the aggregation fetched at cfg3
# (profiles/r05r_*). In gat_csr_kernel's layouts the recomputation cost what the loads saved
# (0.793 vs 0.783 ms, r05p_gat_ab.log); in the edge-head layout (gat_eh_kernel: each lane holds
# its head's slice of the row) it is a lane-local dot product: 0.631 vs 0.772 ms
# (r05t_gat_ab.log). The backward row pass takes er_j the same way.
GAT_ER_RECOMPUTE = True
GAT_TASK_COST = 128


def _gat_tasks_ok(heads, fh, *ts) -> bool:
    # the task kernel's geometry: one 16-B vector per lane, one chunk of <= 64 lanes per row of a
    # head group (<= 8 heads x fh <= 256 features), a lane's features inside one head
    if not GAT_TASKS or fh % 4 or min(heads, 8) * fh > 256:
        return False
    return all(t is None or (t.data_ptr() % 16 == 0 and (t.dim() == 1 or t.stride(0) % 4 == 0))
               for t in ts)
# XCD-sliced hub staging for GAT (``_gat_xcd``) is built and tested but not the default: at
# cfg3 it loses or ties at every setting (tools/xcd_ab.py --op gat, profiles/r02z_xcd_ab_gat_*:
# single pass 0.79 ms; rows of >= 128 edges 0.88, >= 256 0.86, >= 1024 0.79). The edge
# softmax (8 exps per edge, phase A/B through LDS) hides the gathers that the SpMM waits on.
GAT_XCD = False


def _gat_operands(rowptr, n, wh, el, er, lde, heads, fh, slope, mode, fill, out, ldo, partial,
                  stats, flags, stream, dropout_p=0.0, seed=0) -> dict:
    """The arguments every gnn_gat_csr_* entry takes, but for its column array and plan."""
    return dict(rowptr=rowptr.data_ptr(), n_rows=n, wh=wh.data_ptr(), ldw=wh.stride(0),
                heads=heads, fh=fh, el=el.data_ptr(), er=er.data_ptr(), lde=lde,
                negative_slope=float(slope), mode=int(mode), empty_row_fill=_lib.ptr(fill),
                dropout_p=float(dropout_p), dropout_seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                out=out.data_ptr(), ldo=ldo, partial=_lib.ptr(partial), stats=_lib.ptr(stats),
                flags=flags, stream=stream)


def _gat_call(g_rowptr, col, n, wh, el, er, lde, heads, fh, slope, mode, fill, out, ldo, plan,
              mid, short, partial, stats, flags, stream, whh, erh):
    _lib.run("gnn_gat_csr_hub_f32", col_hub=col.data_ptr(),
             **_gat_operands(g_rowptr, n, wh, el, er, lde, heads, fh, slope, mode, fill, out, ldo,
                             partial, stats, flags, stream),
             **plan.segments(), **plan.gat_rows(mid, short), whh=whh.data_ptr(),
             ldwh=whh.stride(0), erh=erh.data_ptr(), ldeh=erh.stride(0))


def _gat_xcd(lib, g: CsrGraph, xp, wh, el, er, heads, fh, slope, mode, fill, out, seg, flags,
             stream):
    """GAT over the XCD-sliced hub plan (graph.XcdHubPlan), inference.

    Pass 1 runs each item (a row's hub edges in one XCD slice) as a row of its own, on XCD
    w % 8 like the SpMM, writing the item's softmax-weighted mean of Wh (no activation) and
    its per-head log-sum-exp L. Pass 2 runs every row's remaining edges plus one pseudo-edge
    per item whose Wh row is that mean and whose logit is L: an edge's logit is
    LeakyReLU(el_i + er_j) (dense; its negation for sparse), so the item's er entry is set
    to LeakyReLU^-1(+-L) - el_i. The online softmax then merges the items exactly as the
    fix-up merges segments (log-sum-exp rule). Both passes are gnn_gat_csr_hub_f32 over
    the staged buffers [hub rows | item rows]."""
    k, n_pos = xp.k, xp.n_pos
    feat = heads * fh
    dev = wh.device
    whb = torch.empty((k + n_pos, feat), dtype=torch.float32, device=dev)
    erb = torch.empty((k + n_pos, heads), dtype=torch.float32, device=dev)
    hp = xp.hub
    for src, dst, w in ((wh, whb, feat), (er, erb, heads)):
        _lib.check(lib.gnn_gather_rows_f32(src.data_ptr(), src.stride(0), src.shape[0],
                                           hp.hub_ids.data_ptr(), k, w, dst.data_ptr(), w,
                                           hp.err.data_ptr(), stream), "gnn_gather_rows_f32")
    el_items = el.index_select(0, xp.item_row)
    lse = torch.empty((n_pos, heads), dtype=torch.float32, device=dev)
    p1 = xp.items.plan(seg)
    if p1.n_seg or p1.n_small:
        raise RuntimeError("XCD hub plan: item rows outside the mid-row class")
    # er is never read in pass 1 (every column is staged): erb stands in with its stride
    _gat_call(xp.items.rowptr, xp.items.col, n_pos, wh, el_items, erb, heads, heads, fh, slope,
              mode, None, whb[k:], feat, p1, p1.mid_row, p1.mid_row[:0], None, lse, 0, stream,
              whb, erb)
    y = lse if mode == GAT_DENSE else -lse
    torch.sub(torch.where(y >= 0, y, y / slope), el_items, out=erb[k:])
    p2 = xp.rest_plan(seg)
    mid, short = p2.gat_split(xp.rest.rowptr, GAT_SHORT_MAX_DEG)
    partial = None
    if p2.n_seg:
        partial = torch.empty((p2.n_seg, feat + 2 * heads), dtype=torch.float32, device=dev)
    _gat_call(xp.rest.rowptr, xp.rest.col, g.n_rows, wh, el, er, el.stride(0), heads, fh, slope,
              mode, fill, out, out.stride(0), p2, mid, short, partial, None, flags, stream, whb,
              erb)


def gat_aggregate_staged(g: CsrGraph, wh: torch.Tensor, el: torch.Tensor, er: torch.Tensor,
                         whh: torch.Tensor, erh: torch.Tensor, heads: int, fh: int,
                         negative_slope: float, mode: int, activation: str | None = None,
                         out: torch.Tensor | None = None) -> torch.Tensor:
    """``gat_aggregate`` (inference: no dropout, no stats) over a graph whose column c >= 0
    reads Wh / er row c and c < 0 reads row -1-c of the staged tables ``whh`` / ``erh``
    (strided views allowed: e.g. the [Wh | er] rows an edge-cut rank received, used in
    place instead of concatenated). gnn_gat_csr_hub_f32; rows without edges are rejected
    (their dense-mode fill is a mean over every column, own and staged)."""
    _require_device(g.rowptr, wh, el, er, whh, erh, out)
    for t, name in ((wh, "Wh"), (el, "el"), (er, "er"), (whh, "whh"), (erh, "erh")):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32 (got {t.dtype})")
    feat = heads * fh
    # column range, checked once per graph (one host sync, cached): -1-c must name a row of
    # the staged tables, c a row of Wh -- the hub kernel does not bound-check its reads
    rng_ = g._plans.get("_col_range")
    if rng_ is None and g.nnz:
        rng_ = g._plans["_col_range"] = tuple(int(v) for v in
                                              torch.stack([g.col.min(), g.col.max()]).tolist())
    if rng_ is not None and (rng_[0] < -whh.shape[0] or rng_[1] >= g.n_cols):
        raise IndexError(f"gat_aggregate_staged: column ids span [{rng_[0]}, {rng_[1]}], the "
                         f"tables hold {whh.shape[0]} staged rows and {g.n_cols} rows")
    if wh.shape != (g.n_cols, feat) or wh.stride(1) != 1:
        raise ValueError("Wh must be [n_cols, heads * fh] with unit column stride")
    if whh.shape[1] != feat or erh.shape != (whh.shape[0], heads) or whh.stride(1) != 1 \
            or erh.stride(1) != 1:
        raise ValueError("whh [K, heads * fh] and erh [K, heads] with unit column stride")
    if el.shape != (g.n_rows, heads) or er.shape != (g.n_cols, heads):
        raise ValueError("el must be [n_rows, heads] and er [n_cols, heads]")
    el, er = el.contiguous(), er.contiguous()
    if el.stride(0) != er.stride(0):
        raise ValueError("el / er must share a row stride")
    if g.has_empty_rows():
        raise ValueError("gat_aggregate_staged: the graph has rows without edges")
    if out is None:
        out = torch.empty((g.n_rows, feat), dtype=torch.float32, device=wh.device)
    if g.n_rows == 0:
        return out
    from .graph import staged_plan
    seg = seg_len_for(feat, GAT_SEG_BYTES)
    plan = g.__dict__.setdefault("_staged_plans", {}).get(seg)
    if plan is None:
        plan = g.__dict__["_staged_plans"][seg] = staged_plan(g, seg)
    mid, short = plan.gat_split(g.rowptr, GAT_SHORT_MAX_DEG)
    partial = None
    if plan.n_seg:
        partial = torch.empty((plan.n_seg, feat + 2 * heads), dtype=torch.float32,
                              device=wh.device)
    _gat_call(g.rowptr, g.col, g.n_rows, wh, el, er, el.stride(0), heads, fh, negative_slope,
              mode, None, out, out.stride(0), plan, mid, short, partial, None,
              _ACT_FLAGS[activation], _lib.stream_handle(wh.device), whh, erh)
    return out


def gat_aggregate(g: CsrGraph, wh: torch.Tensor, el: torch.Tensor, er: torch.Tensor, heads: int,
                  fh: int, negative_slope: float, mode: int, activation: str | None = None,
                  dropout_p: float = 0.0, seed: int = 0, seg_len: int | None = None,
                  out: torch.Tensor | None = None,
                  stats: torch.Tensor | None = None, hubs: int | None = None,
                  xcd: bool | None = None, a_dst: torch.Tensor | None = None) -> torch.Tensor:
    """Fused edge-softmax + neighbour aggregation for all heads (one HIP launch + fix-up).

    ``a_dst`` ([heads * fh], the vector er = Wh . a_dst came from): the kernels recompute er_j
    from the Wh rows they gather instead of loading it (gnn_gat_csr_ex_f32; GAT_ER_RECOMPUTE);
    the same values up to the rounding of er's dot products.

    ``hubs``: Wh / er rows of the highest-degree columns staged into compact tables first
    (gnn_gat_csr_hub_f32; 0 = none, default ``hub_rows_for``); same output bits.

    ``xcd``: XCD-sliced hub staging (``_gat_xcd``; default GAT_XCD and the same size rule
    as the SpMM, inference only: no dropout, no stats, a positive LeakyReLU slope)."""
    _require_device(g.rowptr, wh, el, er, out)
    wh = _rows_f32(wh, "Wh")
    n = g.n_rows
    if wh.shape[0] != g.n_cols or wh.shape[1] != heads * fh:
        raise ValueError("Wh must be [n_cols, heads * fh]")
    if el.shape != (n, heads) or er.shape != (g.n_cols, heads):
        raise ValueError("el must be [n_rows, heads] and er [n_cols, heads]")
    # el / er share one row stride in the C-ABI: strided views of one buffer (gat_project
    # packed=True) pass as they are, anything else is made contiguous
    if not (el.stride(1) == 1 and er.stride(1) == 1 and el.stride(0) == er.stride(0)
            and el.stride(0) >= heads):
        el = el.contiguous()
        er = er.contiguous()
    lde = el.stride(0)
    feat = heads * fh
    if out is None:
        out = torch.empty((n, feat), dtype=torch.float32, device=wh.device)
    if n == 0:
        return out
    fill = None
    if mode == GAT_DENSE and g.has_empty_rows():
        fill = col_mean(wh)
    seg = seg_len if seg_len is not None else seg_len_for(feat, GAT_SEG_BYTES)
    lib = _lib.load()
    if xcd is None:
        xcd = (GAT_XCD and hubs is None and g.nnz >= XCD_MIN_NNZ
               and xcd_hub_rows_for(g.n_cols, feat + heads) > 0)
    if (xcd and g.nnz and dropout_p == 0 and stats is None and negative_slope > 0
            and mode in (GAT_DENSE, GAT_SPARSE)):
        kx = (xcd_hub_rows_for(g.n_cols, feat + heads) if hubs is None
              else min(int(hubs), g.n_cols))
        chunk = min(XCD_CHUNK, seg)
        xp = g.xcd_hub_plan(kx, XCD_MIN_DEG, chunk) if kx >= 8 and chunk >= 4 else None
        if xp is not None:
            _gat_xcd(lib, g, xp, wh, el, er, heads, fh, negative_slope, mode, fill, out, seg,
                     _ACT_FLAGS[activation], _lib.stream_handle(wh.device))
            return out
    plan = g.plan(seg)
    partial = None
    if plan.n_seg:
        partial = torch.empty((plan.n_seg, feat + 2 * heads), dtype=torch.float32,
                              device=wh.device)
    mid, short = plan.gat_split(g.rowptr, GAT_SHORT_MAX_DEG)
    stream = _lib.stream_handle(wh.device)
    kw = _gat_operands(g.rowptr, n, wh, el, er, lde, heads, fh, negative_slope, mode, fill, out,
                       out.stride(0), partial, stats, _ACT_FLAGS[activation], stream, dropout_p,
                       seed)
    kw.update(plan.segments())
    k = hub_rows_for(g.n_cols, feat + heads) if hubs is None else min(int(hubs), g.n_cols)
    hp = whh = erh = None
    ldwh = lderh = 0
    if k > 0 and g.nnz:
        hp = g.hub_plan(k)
        if XCD_DIRECT and hp.prefix:  # degree-ordered columns: hub rows read in place
            whh, ldwh, erh, lderh = wh, wh.stride(0), er, lde
        else:
            whh = torch.empty((hp.k, feat), dtype=torch.float32, device=wh.device)
            erh = torch.empty((hp.k, heads), dtype=torch.float32, device=wh.device)
            ldwh, lderh = feat, heads
            for src, dst, w in ((wh, whh, feat), (er, erh, heads)):
                _lib.check(lib.gnn_gather_rows_f32(src.data_ptr(), src.stride(0), src.shape[0],
                                                   hp.hub_ids.data_ptr(), hp.k, w,
                                                   dst.data_ptr(), w, hp.err.data_ptr(), stream),
                           "gnn_gather_rows_f32")
    col = hp.col_hub if hp is not None else g.col
    staged = dict(whh=_lib.ptr(whh), ldwh=ldwh, erh=_lib.ptr(erh), ldeh=lderh)
    if _gat_tasks_ok(heads, fh, wh, out, fill, whh):
        # the task plan's segments are ``plan``'s own (its base is the cached g.plan(seg))
        tp = g.task_plan(plan.seg_len, GAT_SHORT_MAX_DEG, GAT_TASK_COST)
        rc = _lib.invoke("gnn_gat_csr_tasks_f32", col=col.data_ptr(), **kw, **tp.task_rows(),
                         **staged)
        if rc != _lib.E_UNSUPPORTED:  # e.g. a 4-float vector path the row pitches do not allow
            _lib.check(rc, "gnn_gat_csr_tasks_f32")
            return out
        # the row-class launch below (same plan, same partial buffer) covers the shape
    kw.update(plan.gat_rows(mid, short))
    if a_dst is not None and GAT_ER_RECOMPUTE:
        a_dst = a_dst.detach().reshape(-1).contiguous().float()
        if a_dst.numel() != feat:
            raise ValueError("a_dst must hold heads * fh values")
        _require_device(a_dst)
        _lib.run("gnn_gat_csr_ex_f32", col=col.data_ptr(), **kw, **staged,
                 a_dst=a_dst.data_ptr())
    elif hp is not None:
        _lib.run("gnn_gat_csr_hub_f32", col_hub=col.data_ptr(), **kw, **staged)
    else:
        _lib.run("gnn_gat_csr_f32", col=col.data_ptr(), **kw)
    return out


# ---------------------------------------------------------------- GraphSAGE
# 'MEAN' / 'MAX' of GraphSAGE/graph_utils.py's Aggregator + NeighborAggregator 'sum'
# (GraphSAGE_Pytorch) and the value max-pool the north star names ("mean/max-pool";
# torch.max(dim=1).values, GraphSAGE_Pytorch/models/Aggregator.py:23-24)
SAGE_KINDS = {"MEAN": 0, "MAX": 1, "SUM": 2, "MAXPOOL": 3}


_EMPTY_FILL = {0: float("nan"), 2: 0.0}  # k == 0: torch.mean -> NaN, torch.sum -> 0


def _empty_reduction(mode: int) -> None:
    if mode == 1:  # torch.argmax over an empty dim raises
        raise IndexError("argmax(): Expected reduction dim 1 to have non-zero size.")
    if mode == 3:  # so does torch.max(dim=1)
        raise IndexError("max(): Expected reduction dim 1 to have non-zero size.")


def _sage_out(M, F, mode, dev):
    dt = torch.int64 if mode == 1 else torch.float32
    return torch.empty((M, F), dtype=dt, device=dev)


def sage_aggregate(neigh: torch.Tensor, agg_func: str = "MEAN") -> torch.Tensor:
    """Aggregator over a pre-gathered [M, k, F] tensor (GraphSAGE/graph_utils.py:4-11);
    'SUM' is NeighborAggregator's sum (GraphSAGE_Pytorch/models/Aggregator.py:21-22).
    ``neigh`` may be bfloat16 (gnn_sage_aggregate_bf16): the elements are widened exactly, the
    sums are fp32 and the result is fp32 (int64 for 'MAX') as for a float32 tensor."""
    if agg_func not in SAGE_KINDS:
        raise RuntimeError(f"unknown agg_func {agg_func!r}")
    _f32_or_bf16(neigh, "neigh_feat")
    _require_device(neigh)
    if neigh.dim() != 3:
        raise TypeError("neigh_feat must be float32 or bfloat16 [M, k, F]")
    _bf16_inference_only(neigh, "sage_aggregate")
    if neigh.stride(2) != 1:
        neigh = neigh.contiguous()
    M, k, F = neigh.shape
    mode = SAGE_KINDS[agg_func]
    if k == 0:
        _empty_reduction(mode)
        return torch.full((M, F), _EMPTY_FILL[mode], device=neigh.device)
    out = _sage_out(M, F, mode, neigh.device)
    fn, name = _twin(_lib.load(), "gnn_sage_aggregate", neigh)
    _lib.check(fn(neigh.data_ptr(), neigh.stride(1), neigh.stride(0), M, k, F, mode,
                  out.data_ptr(), F, _lib.stream_handle(neigh.device)), name)
    return out


_ERR_SINK: dict = {}


def _err_flag(dev, check: bool) -> torch.Tensor:
    """A zeroed device flag for a checked gather; unchecked (trusted-index) calls share a
    per-device sink that is never read, so they cost no memset and no host sync."""
    if check:
        return torch.zeros(1, dtype=torch.int32, device=dev)
    t = _ERR_SINK.get(dev)
    if t is None:
        t = _ERR_SINK[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def _check_err(err: torch.Tensor, what: str) -> None:
    if int(err.item()) != 0:
        raise IndexError(f"{what}: index out of range in self")


def _sage_table(t: torch.Tensor, name: str, what: str, *others) -> torch.Tensor:
    """The table operand of op ``what``: float32 or bfloat16 (checked before anything else looks
    at the tensor), on the device like ``others``, [rows, F] with unit column stride (copied
    where it is not), and not a bfloat16 table that asks for a gradient."""
    if t.dtype != torch.float32 and t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be float32 or bfloat16 (got {t.dtype})")
    _require_device(t, *others)
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D [rows, features]")
    if t.stride(1) != 1:
        t = t.contiguous()
    if t.dtype == torch.bfloat16:
        _bf16_inference_only(t, what)
    return t


def _sage_idx(idx: torch.Tensor) -> torch.Tensor:
    """The [M, k] neighbour index as int64 with unit column stride (any row stride)."""
    if idx.dim() != 2:
        raise ValueError("idx must be [M, k]")
    idx = idx.to(torch.int64)
    return idx if idx.stride(1) == 1 else idx.contiguous()


def _sage_self_idx(self_idx: torch.Tensor, M: int) -> torch.Tensor:
    """The centre index as a flat contiguous int64 tensor, one entry per output row."""
    self_idx = self_idx.to(torch.int64).contiguous().view(-1)
    if self_idx.numel() != M:
        raise ValueError("self_idx must hold one index per output row")
    return self_idx


def _sage_live(live: torch.Tensor) -> None:
    if live.dtype != torch.int64 or live.numel() != 1:
        raise TypeError("live must be a one-element int64 device tensor")


def _twin(lib, stem: str, t: torch.Tensor):
    """(entry, its name) of the pair ``stem`` + '_f32' / '_bf16', chosen by t's dtype."""
    name = stem + ("_bf16" if t.dtype == torch.bfloat16 else "_f32")
    return getattr(lib, name), name


def _sage_dst(out, M, F, mode, dev):
    """The caller's output view (any row stride, unit column stride) or a new tensor."""
    if out is None:
        return _sage_out(M, F, mode, dev)
    want = torch.int64 if mode == 1 else torch.float32
    if out.shape != (M, F) or out.dtype != want or out.stride(1) != 1 or not out.is_cuda:
        raise ValueError(f"out must be a {want} [{M}, {F}] device view with unit column stride")
    return out


def sage_gather_aggregate(table: torch.Tensor, idx: torch.Tensor, agg_func: str = "MEAN",
                          check: bool = True, out: torch.Tensor | None = None,
                          live: torch.Tensor | None = None) -> torch.Tensor:
    """Aggregator(torch.embedding(table, idx)) fused: [M, k] int64 indices into table [n, F].
    A bfloat16 ``table`` (the stored input features; gnn_sage_gather_aggregate_bf16) is read
    at 2 bytes per element, widened exactly and reduced in fp32: the result is fp32 (int64 for
    'MAX'), and 'MAX' / 'MAXPOOL' are exact functions of the stored values.
    ``live`` ('MEAN' / 'MAXPOOL' only): a device int64 scalar; rows [0, min(live, M)) only
    (gnn_sage_gather_aggregate_live_f32 / _bf16, M = the capacity of a sampled batch whose
    frontier size the host never read); the other rows of the result are left as they were."""
    if agg_func not in SAGE_KINDS:
        raise RuntimeError(f"unknown agg_func {agg_func!r}")
    if live is not None and agg_func not in ("MEAN", "MAXPOOL"):
        raise ValueError("live= is supported for 'MEAN' and 'MAXPOOL' only")
    table = _sage_table(table, "table", "sage_gather_aggregate", idx, live)
    idx = _sage_idx(idx)
    M, k = idx.shape
    F = table.shape[1]
    mode = SAGE_KINDS[agg_func]
    out = _sage_dst(out, M, F, mode, table.device)
    if k == 0:  # torch.mean over an empty dim is NaN, sum is 0; the caller's view is filled
        _empty_reduction(mode)
        return out.fill_(_EMPTY_FILL[mode])
    err = _err_flag(table.device, check)
    lib = _lib.load()
    if live is not None:
        _sage_live(live)
        fn, name = _twin(lib, "gnn_sage_gather_aggregate_live", table)
        rc = fn(table.data_ptr(), table.stride(0), table.shape[0], idx.data_ptr(), idx.stride(0),
                M, live.data_ptr(), k, F, mode, out.data_ptr(), out.stride(0), err.data_ptr(),
                _lib.stream_handle(table.device))
    else:
        fn, name = _twin(lib, "gnn_sage_gather_aggregate", table)
        rc = fn(table.data_ptr(), table.stride(0), table.shape[0], idx.data_ptr(), idx.stride(0),
                M, k, F, mode, out.data_ptr(), out.stride(0), err.data_ptr(),
                _lib.stream_handle(table.device))
    _lib.check(rc, name)
    if check:
        _check_err(err, "sage_gather_aggregate")
    return out


def sage_gather_concat(table: torch.Tensor, self_idx: torch.Tensor, idx: torch.Tensor,
                       agg_func: str = "MEAN", check: bool = True,
                       out: torch.Tensor | None = None,
                       live: torch.Tensor | None = None) -> torch.Tensor:
    """[M, 2F] = cat[table[self_idx], Aggregator(table[idx])] in one launch
    (gnn_sage_gather_concat_f32): the SageLayer input of GraphSAGE/GraphSAGE.py:17 with the
    gathers of :47-49. ``out`` may be any [M, 2F] float32 view with unit column stride.
    ``live``: a device int64 scalar; rows [0, min(live, M)) only (gnn_sage_gather_concat_live_f32,
    M = the capacity of a sampled batch whose frontier size the host never read).
    'MAX' (torch.argmax over the neighbours, graph_utils.py:8): the index written as fp32, the
    value torch.cat([self, argmax]) promotes it to (GNN_SAGE_ARGMAX_F32).
    A bfloat16 ``table`` (gnn_sage_gather_concat_live_bf16): both halves stay float32 -- the
    centre rows are stored widened, the aggregate is reduced in fp32."""
    if agg_func not in ("MEAN", "SUM", "MAXPOOL", "MAX"):
        raise RuntimeError(f"agg_func {agg_func!r} has no concat form")
    mode = 4 if agg_func == "MAX" else SAGE_KINDS[agg_func]
    table = _sage_table(table, "table", "sage_gather_concat", self_idx, idx, out)
    idx = _sage_idx(idx)
    M, k = idx.shape
    F = table.shape[1]
    self_idx = _sage_self_idx(self_idx, M)
    if out is None:
        out = torch.empty((M, 2 * F), dtype=torch.float32, device=table.device)
    elif out.shape != (M, 2 * F) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError(f"out must be a float32 [{M}, {2 * F}] view with unit column stride")
    if M == 0:
        return out
    if k == 0:
        _empty_reduction(SAGE_KINDS[agg_func])
        gather_rows(table, self_idx, out=out[:, :F], check=check)
        out[:, F:].fill_(_EMPTY_FILL[SAGE_KINDS[agg_func]])
        return out
    if live is not None:
        _require_device(live)
        _sage_live(live)
    err = _err_flag(table.device, check)
    fn, name = _twin(_lib.load(), "gnn_sage_gather_concat_live", table)
    _lib.check(fn(
        table.data_ptr(), table.stride(0), table.shape[0], self_idx.data_ptr(), idx.data_ptr(),
        idx.stride(0), M, _lib.ptr(live), k, F, mode, out.data_ptr(),
        out.stride(0), out[:, F:].data_ptr(), out.stride(0), err.data_ptr(),
        _lib.stream_handle(table.device)), name)
    if check:
        _check_err(err, "sage_gather_concat")
    return out


class SageMapsT(NamedTuple):
    """The transposed index maps of one SageLayer (``sage_maps_transpose``): the slots of
    target t are ``slot[ptr[t]:ptr[t + 1]]`` in ascending slot order; slot s < M is centre row
    s, slot s >= M the neighbour entry s - M (row (s - M) // k, column (s - M) % k)."""
    ptr: torch.Tensor    # int64 [n_prev + 1]
    slot: torch.Tensor   # int32 [M * (k + 1)]
    M: int
    k: int
    # False: the maps of the neighbour map alone (``sage_maps_transpose_nbr``, the gcn-mode
    # layer): M * k slots, slot e the entry (e // k, e % k), no centre slots
    centre: bool = True


def _maps_transpose(center_idx, neigh_idx, n_prev, check, centre):
    """The body of ``sage_maps_transpose`` (``centre``: the M centre slots come first) and
    ``sage_maps_transpose_nbr`` (``center_idx`` None: the neighbour map alone)."""
    what = "sage_maps_transpose" if centre else "sage_maps_transpose_nbr"
    _require_device(center_idx, neigh_idx)
    if neigh_idx.dim() != 2:
        raise ValueError("neigh_idx must be [M, k]")
    if neigh_idx.dtype != torch.int64 or (centre and center_idx.dtype != torch.int64):
        raise TypeError("the index maps must be int64")
    n_prev = int(n_prev)
    if n_prev < 0:
        raise ValueError("n_prev must not be negative")
    if ((neigh_idx.stride(1) != 1 and neigh_idx.shape[1] > 1)
            or (neigh_idx.shape[0] > 1 and neigh_idx.stride(0) < neigh_idx.shape[1])):
        neigh_idx = neigh_idx.contiguous()
    M, k = neigh_idx.shape
    if centre:
        center_idx = center_idx.contiguous().view(-1)
        if center_idx.numel() != M:
            raise ValueError("center_idx must hold one index per row of neigh_idx")
    dev = neigh_idx.device
    n_slots = M * (k + 1 if centre else k)
    if n_slots == 0:  # M = 0, or k = 0 without centre slots: every list is empty
        return SageMapsT(torch.zeros(n_prev + 1, dtype=torch.int64, device=dev),
                         torch.empty(0, dtype=torch.int32, device=dev), M, k, centre)
    lib = _lib.load()
    query = (lib.gnn_sage_maps_transpose_workspace_bytes if centre else
             lib.gnn_sage_maps_transpose_nbr_workspace_bytes)
    nbytes = int(query(M, k))
    if nbytes == _lib.E_UNSUPPORTED or n_prev >= 2 ** 31 - 1:
        return None
    ptr = torch.empty(n_prev + 1, dtype=torch.int64, device=dev)
    slot = torch.empty(n_slots, dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    err = _err_flag(dev, check)
    # a single row's stride is never used; k = 0 (centre slots alone) reads no neighbour map
    ldi = neigh_idx.stride(0) if M > 1 and k > 0 else k
    nbr = neigh_idx.data_ptr() if k > 0 else None
    tail = (ldi, M, k, n_prev, ptr.data_ptr(), slot.data_ptr(), err.data_ptr(), ws.data_ptr(),
            ws.numel(), _lib.stream_handle(dev))
    if centre:
        rc = lib.gnn_sage_maps_transpose(center_idx.data_ptr(), nbr, *tail)
    else:
        rc = lib.gnn_sage_maps_transpose_nbr(nbr, *tail)
    _lib.check(rc, "gnn_" + what)
    if check:
        _check_err(err, what)
    return SageMapsT(ptr, slot, M, k, centre)


def sage_maps_transpose(center_idx: torch.Tensor, neigh_idx: torch.Tensor, n_prev: int,
                        check: bool = True) -> SageMapsT | None:
    """The transposed maps of ``sage_gather_concat(table, center_idx, neigh_idx)`` over a table
    of ``n_prev`` rows, built on the device (gnn_sage_maps_transpose: a stable radix sort of
    the slots by target): exactly numpy's stable argsort of ``[center_idx, neigh_idx.ravel()]``
    with its bincount / cumsum. ``check``: an index outside [0, n_prev) raises IndexError (one
    host read). None where M (k + 1) does not fit an int32 slot id."""
    return _maps_transpose(center_idx, neigh_idx, n_prev, check, True)


def sage_maps_transpose_nbr(neigh_idx: torch.Tensor, n_prev: int,
                            check: bool = True) -> SageMapsT | None:
    """The transposed maps of ``sage_gather_aggregate(table, neigh_idx)`` over a table of
    ``n_prev`` rows (gnn_sage_maps_transpose_nbr): ``sage_maps_transpose`` without the centre
    slots -- slot e is the entry (e // k, e % k); exactly numpy's stable argsort of
    ``neigh_idx.ravel()`` with its bincount / cumsum. The result has ``centre=False``.
    ``check``: an index outside [0, n_prev) raises IndexError (one host read). None where M k
    does not fit an int32 slot id."""
    return _maps_transpose(None, neigh_idx, n_prev, check, False)


def _gather_arg(table, self_idx, idx, check, centre):
    """The body of ``sage_gather_concat_arg`` (``centre``: buf [M, 2F], the centre rows in its
    first half) and ``sage_gather_aggregate_arg`` (``self_idx`` None: buf [M, F])."""
    what = "sage_gather_concat_arg" if centre else "sage_gather_aggregate_arg"
    table = _sage_table(table, "table", what, self_idx, idx)
    idx = _sage_idx(idx)
    M, k = idx.shape
    F = table.shape[1]
    if centre:
        self_idx = _sage_self_idx(self_idx, M)
    lib = _lib.load()
    vec = 8 if _bf16(table) else 4
    supported = (lib.gnn_sage_gather_concat_arg_supported if centre else
                 lib.gnn_sage_gather_aggregate_arg_supported)
    if not supported(F, k) or F % vec or table.stride(0) % vec or table.data_ptr() % 16:
        return None
    ldb = 2 * F if centre else F
    buf = torch.empty((M, ldb), dtype=torch.float32, device=table.device)
    arg = torch.empty((M, F), dtype=torch.uint8, device=table.device)
    if M == 0:
        return buf, arg
    err = _err_flag(table.device, check)
    fn, name = _twin(lib, "gnn_" + what, table)
    tail = (arg.data_ptr(), F, err.data_ptr(), _lib.stream_handle(table.device))
    if centre:
        rc = fn(table.data_ptr(), table.stride(0), table.shape[0], self_idx.data_ptr(),
                idx.data_ptr(), idx.stride(0), M, k, F, buf.data_ptr(), ldb,
                buf[:, F:].data_ptr(), ldb, *tail)
    else:
        rc = fn(table.data_ptr(), table.stride(0), table.shape[0], idx.data_ptr(), idx.stride(0),
                M, k, F, buf.data_ptr(), ldb, *tail)
    _lib.check(rc, name)
    if check:
        _check_err(err, what)
    return buf, arg


def sage_gather_concat_arg(table: torch.Tensor, self_idx: torch.Tensor, idx: torch.Tensor,
                           check: bool = True):
    """``sage_gather_concat(table, self_idx, idx, 'MAXPOOL')`` that also records the winner
    (gnn_sage_gather_concat_arg_f32 / _bf16): returns ``(buf, arg)`` -- buf float32 [M, 2F] =
    cat[table[self_idx], max_j table[idx[:, j]]], arg uint8 [M, F] the neighbour column whose
    row holds that maximum under torch.argmax's order (a NaN first, then the larger value, then
    the smaller column: ``sage_gather_aggregate(table, idx, 'MAX')`` as bytes). buf[m, F + f]
    is the value AT arg[m, f]; it compares equal to MAXPOOL's (the sign of a zero and the
    payload of a NaN may differ). What the training layer saves for its backward: one byte per
    (row, feature) instead of an int64. None where the kernel does not take the shape (F not a
    power of two in [4, 256] -- [8, 256] for a bfloat16 table --, k outside [1, 255], a table
    view whose rows are not 16-B lanes)."""
    return _gather_arg(table, self_idx, idx, check, True)


def sage_gather_aggregate_arg(table: torch.Tensor, idx: torch.Tensor, check: bool = True):
    """``sage_gather_aggregate(table, idx, 'MAXPOOL')`` that also records the winner
    (gnn_sage_gather_aggregate_arg_f32 / _bf16): returns ``(out, arg)`` -- out float32 [M, F] =
    max_j table[idx[:, j]], arg uint8 [M, F] the winning neighbour column. The gcn-mode twin of
    ``sage_gather_concat_arg`` (no centre half), with its rules: the first maximum, a NaN first
    (``sage_gather_aggregate(table, idx, 'MAX')`` as bytes); out[m, f] is the value AT
    arg[m, f]. None where the kernel does not take the shape (F not a power of two in [4, 256]
    -- [8, 256] for a bfloat16 table --, k outside [1, 255], a table view whose rows are not
    16-B lanes)."""
    return _gather_arg(table, None, idx, check, False)


def sage_scatter_supported(F: int) -> bool:
    """Whether the scatters below take a table of width F: a power of two in [4, 256]
    (gnn_sage_scatter_concat_supported; F / 4 lanes of 16 B per row)."""
    return bool(_lib.load().gnn_sage_scatter_concat_supported(F))


def _sage_scatter(dbuf, arg, tr, n_prev, out, centre, scale=None):
    """The body of the four scatters. ``centre``: the concat layout (dbuf [M, 2F], the maps of
    ``sage_maps_transpose``), else the gcn-mode one (dbuf [M, F], ``sage_maps_transpose_nbr``).
    ``arg`` given: the MAXPOOL select; ``scale`` given (``sage_scatter_agg``): the scaled entry."""
    _require_device(dbuf, arg, tr.ptr, tr.slot, out)
    if dbuf.dtype != torch.float32:
        raise TypeError(f"dbuf must be float32 (got {dbuf.dtype})")
    if arg is not None and arg.dtype != torch.uint8:
        raise TypeError(f"arg must be uint8 (got {arg.dtype})")
    if dbuf.dim() != 2 or (centre and dbuf.shape[1] % 2):
        raise ValueError("dbuf must be [M, 2F]" if centre else "dbuf must be [M, F]")
    n_prev = int(n_prev)
    M, k = tr.M, tr.k
    width = dbuf.shape[1]  # of a row of dbuf: 2F with the centre half
    F = width // 2 if centre else width
    if (bool(tr.centre) != centre or dbuf.shape[0] != M or tr.ptr.numel() != n_prev + 1
            or tr.slot.numel() != M * (k + 1 if centre else k)
            or (arg is not None and tuple(arg.shape) != (M, F))):
        raise ValueError("dbuf, arg, the transposed maps (sage_maps_transpose"
                         f"{'' if centre else '_nbr'}) and n_prev do not belong together")
    if tr.ptr.dtype != torch.int64 or tr.slot.dtype != torch.int32:
        raise TypeError("the transposed maps must be (int64 ptr, int32 slot)")
    if out is not None and (out.shape != (n_prev, F) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError(f"out must be a contiguous float32 [{n_prev}, {F}] tensor")
    lib = _lib.load()
    if k < 1 or (arg is not None and k > 255) or not lib.gnn_sage_scatter_concat_supported(F):
        return None
    if M == 0:
        return (torch.zeros((n_prev, F), dtype=torch.float32, device=dbuf.device)
                if out is None else out.zero_())
    if (dbuf.stride(1) != 1 or (M > 1 and (dbuf.stride(0) % 4 or dbuf.stride(0) < width))
            or dbuf.data_ptr() % 16):
        return None
    if arg is not None and (arg.stride(1) != 1 or arg.data_ptr() % 4
                            or (M > 1 and (arg.stride(0) % 4 or arg.stride(0) < F))):
        return None
    stem = (("gnn_sage_scatter_concat" if centre else "gnn_sage_scatter_agg")
            + ("" if arg is None else "_maxpool"))
    nbytes = int(getattr(lib, stem + "_workspace_bytes")(M, k, F))
    if nbytes < 0:
        return None
    dx = out if out is not None else torch.empty((n_prev, F), dtype=torch.float32,
                                                 device=dbuf.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dbuf.device)
    ptr, slot = tr.ptr.contiguous(), tr.slot.contiguous()
    ldd = dbuf.stride(0) if M > 1 else width  # a single row's stride is never used
    if scale is not None:
        _lib.run("gnn_sage_scatter_agg_scaled_f32", dbuf=dbuf.data_ptr(), ldd=ldd,
                 ptr=ptr.data_ptr(), slot=slot.data_ptr(), M=M, k=k, feat=F, n_prev=n_prev,
                 dx=dx.data_ptr(), ldx=F, scale=float(scale), workspace=ws.data_ptr(),
                 workspace_bytes=ws.numel(), stream=_lib.stream_handle(dbuf.device))
        return dx
    mask = () if arg is None else (arg.data_ptr(), arg.stride(0) if M > 1 else F)
    _lib.check(getattr(lib, stem + "_f32")(
        dbuf.data_ptr(), ldd, *mask, ptr.data_ptr(), slot.data_ptr(), M, k, F, n_prev,
        dx.data_ptr(), F, ws.data_ptr(), ws.numel(), _lib.stream_handle(dbuf.device)),
        stem + "_f32")
    return dx


def sage_scatter_concat(dbuf: torch.Tensor, tr: SageMapsT, n_prev: int,
                        out: torch.Tensor | None = None) -> torch.Tensor | None:
    """The adjoint of ``sage_gather_concat`` in MEAN mode (gnn_sage_scatter_concat_f32):
    dX[t] = sum of dbuf[s, :F] over the centre slots s of t + sum of dbuf[m, F:] / k over the
    neighbour slots (m, j) of t, for the maps ``tr = sage_maps_transpose(...)``; float32
    [n_prev, F] with F = dbuf.shape[1] // 2. Rows nobody references are zeros. fp32 sums in
    slot order, no float atomics: bit-identical from run to run. ``dbuf``: any float32 [M, 2F]
    view with 16-B aligned rows; ``out``: a contiguous float32 [n_prev, F] tensor to write
    (every row is stored, whatever it held). None where the kernel does not take the shape
    (F not a power of two in [4, 256], k = 0, a misaligned view): the caller scatters another
    way."""
    return _sage_scatter(dbuf, None, tr, n_prev, out, True)


def sage_scatter_concat_maxpool(dbuf: torch.Tensor, arg: torch.Tensor, tr: SageMapsT,
                                n_prev: int, out: torch.Tensor | None = None
                                ) -> torch.Tensor | None:
    """The adjoint of ``sage_gather_concat_arg`` (gnn_sage_scatter_concat_maxpool_f32):
    dX[t, f] = sum of dbuf[s, f] over the centre slots s of t + sum over the neighbour slots
    (m, j) of t of (dbuf[m, F + f] if arg[m, f] == j else 0), for the maps
    ``tr = sage_maps_transpose(...)``. The mask selects (a non-finite gradient at a slot that
    did not win reaches nobody), as torch's index_put_ of the gradient does. Everything else is
    ``sage_scatter_concat``'s: fp32 sums in slot order, no float atomics, bit-identical from
    run to run, every row of the result stored. ``arg``: a uint8 [M, F] view with unit column
    stride and rows of whole 4-B words. None where the kernel does not take the shape (the
    widths of ``sage_scatter_concat``, k outside [1, 255], a misaligned view)."""
    if arg is None:
        raise TypeError("arg must be a uint8 [M, F] tensor")
    return _sage_scatter(dbuf, arg, tr, n_prev, out, True)


def sage_scatter_agg(dbuf: torch.Tensor, tr: SageMapsT, n_prev: int,
                     out: torch.Tensor | None = None,
                     scale: float | None = None) -> torch.Tensor | None:
    """The adjoint of ``sage_gather_aggregate(table, idx, 'MEAN')`` (gnn_sage_scatter_agg_f32):
    dX[t] = sum of dbuf[m] / k over the entries (m, j) with idx[m, j] == t, for the maps
    ``tr = sage_maps_transpose_nbr(idx, n_prev)``; float32 [n_prev, F] with F = dbuf.shape[1].
    The gcn-mode twin of ``sage_scatter_concat`` (no centre half) with its contract: rows
    nobody references are zeros, fp32 sums in slot order, no float atomics, bit-identical from
    run to run; ``dbuf`` any float32 [M, F] view with 16-B aligned rows, ``out`` a contiguous
    float32 [n_prev, F] tensor to write. None where the kernel does not take the shape (F not a
    power of two in [4, 256], k = 0, a misaligned view).
    ``scale``: the factor in place of 1 / k (gnn_sage_scatter_agg_scaled_f32): 1 for the adjoint
    of a SUM over the neighbours or of a row gather (k = 1); ``scale = 1 / k`` (in float32) gives
    the default's result bit for bit."""
    return _sage_scatter(dbuf, None, tr, n_prev, out, False, scale)


def sage_scatter_agg_maxpool(dbuf: torch.Tensor, arg: torch.Tensor, tr: SageMapsT, n_prev: int,
                             out: torch.Tensor | None = None) -> torch.Tensor | None:
    """The adjoint of ``sage_gather_aggregate_arg`` (gnn_sage_scatter_agg_maxpool_f32):
    dX[t, f] = sum over the entries (m, j) of t of (dbuf[m, f] if arg[m, f] == j else 0), for
    the maps ``tr = sage_maps_transpose_nbr(idx, n_prev)``. The mask selects (a non-finite
    gradient at a slot that did not win reaches nobody). Everything else is
    ``sage_scatter_agg``'s; ``arg``: a uint8 [M, F] view with unit column stride and rows of
    whole 4-B words. None where the kernel does not take the shape (the widths of
    ``sage_scatter_agg``, k outside [1, 255], a misaligned view)."""
    if arg is None:
        raise TypeError("arg must be a uint8 [M, F] tensor")
    return _sage_scatter(dbuf, arg, tr, n_prev, out, False)


def sage_train_layer_supported(table: torch.Tensor, weight: torch.Tensor, k: int,
                               agg: str = 'MEAN', gcn: bool = False) -> bool:
    """Whether the training SageLayer (graphsage._SageTrainLayerFn; ``agg`` 'MAXPOOL':
    graphsage._SageMaxPoolTrainLayerFn) runs on its own kernels for an [n, F] table, an [H, 2F]
    weight and k neighbours per row: ``gcn_transform`` takes (2F, H) and ``sage_scatter_concat``
    takes F; for 'MAXPOOL' also ``sage_gather_concat_arg`` takes (F, k) and the table's rows.
    ``gcn=True`` (graphsage._SageGcnTrainLayerFn): the weight is [H, F], ``gcn_transform`` takes
    (F, H), ``sage_scatter_agg`` takes F, and for 'MAXPOOL' ``sage_gather_aggregate_arg`` takes
    (F, k) and the table's rows."""
    if agg not in ('MEAN', 'MAXPOOL'):
        return False
    if (not table.is_cuda or not weight.is_cuda or table.dim() != 2 or weight.dim() != 2
            or table.dtype not in (torch.float32, torch.bfloat16)
            or weight.dtype != torch.float32 or k < 1):
        return False
    F, (H, K) = table.shape[1], weight.shape
    lib = _lib.load()
    ok = bool(K == (F if gcn else 2 * F) and lib.gnn_gcn_transform_supported(K, H)
              and (TRANSFORM_WIDE_MFMA or not (H == 256 and K > 64))
              and sage_scatter_supported(F))
    if ok and agg == 'MAXPOOL':
        vec = 8 if table.dtype == torch.bfloat16 else 4
        sup = (lib.gnn_sage_gather_aggregate_arg_supported if gcn else
               lib.gnn_sage_gather_concat_arg_supported)
        ok = bool(sup(F, k) and F % vec == 0
                  and table.stride(1) == 1 and table.stride(0) % vec == 0
                  and table.data_ptr() % 16 == 0)
    return ok


# ---------------------------------------------------------------- the unsupervised head
def _score_rows(t: torch.Tensor, H: int) -> bool:
    """An fp32 [rows, H] view the score kernels read or write with 16-B accesses."""
    return (t.stride(1) == 1 and t.data_ptr() % 16 == 0
            and (t.shape[0] <= 1 or (t.stride(0) % 4 == 0 and t.stride(0) >= H)))


def _score_operands(center: torch.Tensor, second: torch.Tensor, S: int):
    """(B, S, H) of a score call after the dtype and shape checks of ``sage_score``."""
    if center.dtype != torch.float32 or second.dtype != torch.float32:
        raise TypeError(f"center and second must be float32 (got {center.dtype}, {second.dtype})")
    if center.dim() != 2 or second.dim() != 2:
        raise ValueError("center must be [B, H] and second [B * S, H]")
    S = int(S)
    B, H = center.shape
    if S < 0 or second.shape != (B * S, H):
        raise ValueError(f"second must be [B * S, H] = [{B * S}, {H}] (got {tuple(second.shape)})")
    return B, S, H


def _score_takes(center: torch.Tensor, second: torch.Tensor) -> bool:
    """Whether the score kernels take center [B, H] and second [B S, H] (fp32 device tensors):
    the width, unit stride along H, 16-B aligned rows."""
    H = center.shape[1]
    return bool(_lib.load().gnn_sage_score_supported(H)) and (_score_rows(center, H)
                                                              and _score_rows(second, H))


def _bce_takes(z: torch.Tensor, y: torch.Tensor) -> bool:
    """Whether ``bce_logits`` takes the layouts of z and y (both [rows, cols])."""
    rows, cols = z.shape
    return (rows * cols > 0 and z.stride(1) == 1 and y.stride(1) == 1
            and (rows == 1 or (z.stride(0) >= cols and y.stride(0) >= cols)))


def _ld(t: torch.Tensor, width: int) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(width, 4)


def sage_score(center: torch.Tensor, second: torch.Tensor, S: int,
               out: torch.Tensor | None = None) -> torch.Tensor | None:
    """The unsupervised head's scores (gnn_sage_score_f32): z[b, s] = center[b] . second[b S + s],
    float32 [B, S] -- ``torch.bmm(center.unsqueeze(1), second.reshape(B, S, H).permute(0, 2, 1))``
    (GraphSAGE/GraphSAGE.py:61) without the permuted operand. fp32 sums in a fixed order:
    bit-identical from run to run. ``center`` [B, H], ``second`` [B S, H]: float32 views with
    unit stride along H and 16-B aligned rows; ``out``: a contiguous float32 [B, S] tensor to
    write. None where the kernel does not take the shape (H not a power of two in [4, 256], a
    stride along H that is not 1, a misaligned view, a pitch that is not a multiple of 4): the
    caller keeps torch's path."""
    _require_device(center, second, out)
    B, S, H = _score_operands(center, second, S)
    if out is not None and (out.shape != (B, S) or out.dtype != torch.float32
                            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 [{B}, {S}] tensor")
    lib = _lib.load()
    if not _score_takes(center, second):
        return None
    z = out if out is not None else torch.empty((B, S), dtype=torch.float32,
                                                device=center.device)
    if B and S:
        _lib.check(lib.gnn_sage_score_f32(
            center.data_ptr(), _ld(center, H), second.data_ptr(), _ld(second, H), B, S, H,
            z.data_ptr(), S, _lib.stream_handle(center.device)), "gnn_sage_score_f32")
    return z


def sage_score_backward(g: torch.Tensor, center: torch.Tensor, second: torch.Tensor,
                        need_center: bool = True, need_second: bool = True):
    """The adjoint of ``sage_score`` for g = dL/dz [B, S] (gnn_sage_score_bwd_f32):
    (d_center [B, H], d_second [B S, H]) with d_second[b S + s] = g[b, s] * center[b] (exactly
    torch's product, stored in the layout the second tower's last layer takes) and
    d_center[b] = sum_s g[b, s] second[b S + s], summed in an order fixed by (S, H): no float
    atomics, bit-identical from run to run. A half that is not needed is neither computed nor
    allocated (None in its place). None (alone) where the kernel does not take the shape, as
    ``sage_score``."""
    _require_device(g, center, second)
    if g.dtype != torch.float32:
        raise TypeError(f"g must be float32 (got {g.dtype})")
    if g.dim() != 2 or g.shape[0] != center.shape[0]:
        raise ValueError("g must be [B, S]")
    B, S, H = _score_operands(center, second, g.shape[1])
    lib = _lib.load()
    if not _score_takes(center, second):
        return None
    if g.stride(1) != 1 or (B > 1 and g.stride(0) < S):
        g = g.contiguous()
    f32 = dict(dtype=torch.float32, device=center.device)
    if need_center:  # at S = 0 (or B = 0) nothing is launched: the empty sums are these zeros
        dc = torch.empty((B, H), **f32) if B and S else torch.zeros((B, H), **f32)
    else:
        dc = None
    dx = torch.empty((B * S, H), **f32) if need_second else None
    if B and S and (need_center or need_second):
        _lib.check(lib.gnn_sage_score_bwd_f32(
            g.data_ptr(), g.stride(0) if B > 1 else S, center.data_ptr(), _ld(center, H),
            second.data_ptr(), _ld(second, H), B, S, H, _lib.ptr(dc), H, _lib.ptr(dx), H,
            _lib.stream_handle(center.device)), "gnn_sage_score_bwd_f32")
    return dc, dx


def bce_logits(z: torch.Tensor, y: torch.Tensor, want_grad: bool = True):
    """``F.binary_cross_entropy_with_logits(z, y.float())`` (mean) and its gradient in one pass
    (gnn_bce_logits_f32): (loss, g) with loss a 0-dim float32 tensor and
    g = (sigmoid(z) - y) / z.numel() shaped as z (None unless ``want_grad``). torch's expression
    (1 - y) z - logsigmoid(z), evaluated per element in double and summed in double in a fixed
    order: bit-identical from run to run, z = +-inf / NaN as in torch. ``z``: float32 [rows,
    cols]; ``y``: float32 or int64 of the same shape (soft labels as they are). None where the
    kernel does not take the layout (a stride along the columns that is not 1, no elements): the
    caller keeps torch's function."""
    _require_device(z, y)
    if z.dtype != torch.float32:
        raise TypeError(f"z must be float32 (got {z.dtype})")
    if y.dtype not in (torch.float32, torch.int64):
        raise TypeError(f"y must be float32 or int64 (got {y.dtype})")
    if z.dim() != 2 or y.shape != z.shape:
        raise ValueError("z and y must be [rows, cols] of one shape")
    rows, cols = z.shape
    if not _bce_takes(z, y):
        return None
    lib = _lib.load()
    dev = z.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    g = torch.empty((rows, cols), dtype=torch.float32, device=dev) if want_grad else None
    ws = torch.empty(int(lib.gnn_bce_logits_workspace_bytes(rows * cols)), dtype=torch.uint8,
                     device=dev)
    _lib.check(lib.gnn_bce_logits_f32(
        z.data_ptr(), z.stride(0) if rows > 1 else cols, y.data_ptr(),
        y.stride(0) if rows > 1 else cols, int(y.dtype == torch.int64), rows, cols,
        loss.data_ptr(), _lib.ptr(g), cols, ws.data_ptr(), ws.numel(),
        _lib.stream_handle(dev)), "gnn_bce_logits_f32")
    return loss.reshape(()), g


# ---------------------------------------------------------------- the supervised head
IGNORE_INDEX = -100  # nn.CrossEntropyLoss()'s


def _sup_head_operands(z: torch.Tensor, labels: torch.Tensor) -> bool:
    """The shape check of the supervised head's ops (z 2-D, labels given per row), then whether
    the kernels take the layout: fp32 logits with 2 <= C <= 64 and unit stride along C, int64
    labels [N]. Float labels (class probabilities) and everything else are torch's."""
    if z.dim() != 2:
        raise ValueError(f"logits must be [N, C] (got {tuple(z.shape)})")
    if labels.dim() < 1 or labels.shape[0] != z.shape[0]:
        raise ValueError(f"labels must have one entry per row of the logits "
                         f"(got {tuple(labels.shape)} for {tuple(z.shape)})")
    N, C = z.shape
    return bool(z.dtype == torch.float32 and labels.dtype == torch.int64 and labels.dim() == 1
                and _lib.load().gnn_sup_head_supported(C) and z.stride(1) == 1
                and (N <= 1 or z.stride(0) >= C))


def _new_status(dev) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=dev)


def sup_head_count(index: torch.Tensor, N: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The multiplicity of every row in a selection (gnn_sup_head_count_index / _mask):
    (count int32 [N], status int32 [1]). ``index``: int64 [n], entries in [-N, 0) wrapping as
    torch's indexing does, duplicates counted; or a bool mask [N] (converted on the device, no
    ``nonzero``). An entry outside [-N, N) addresses nothing and sets bit 0 of ``status``."""
    _require_device(index)
    if index.dtype not in (torch.int64, torch.bool):
        raise TypeError(f"index must be int64 or a bool mask (got {index.dtype})")
    if index.dim() != 1 or (index.dtype == torch.bool and index.shape[0] != N):
        raise ValueError(f"index must be int64 [n] or bool [{N}] (got {tuple(index.shape)})")
    lib = _lib.load()
    dev = index.device
    index = index.contiguous()
    count = torch.empty(N, dtype=torch.int32, device=dev)
    status = _new_status(dev)
    if index.dtype == torch.bool:
        _lib.check(lib.gnn_sup_head_count_mask(index.data_ptr(), N, count.data_ptr(),
                                               _lib.stream_handle(dev)),
                   "gnn_sup_head_count_mask")
    else:
        _lib.check(lib.gnn_sup_head_count_index(
            index.data_ptr(), index.shape[0], N, count.data_ptr(), status.data_ptr(),
            _lib.stream_handle(dev)), "gnn_sup_head_count_index")
    return count, status


def sup_head_forward(z: torch.Tensor, labels: torch.Tensor, index: torch.Tensor | None = None,
                     count: torch.Tensor | None = None, status: torch.Tensor | None = None,
                     want_correct: bool = True):
    """``F.cross_entropy(z[index], labels[index])`` (mean, ignore_index -100) and the count of
    correct predictions ``(argmax(z[index], 1) == labels[index]).sum()`` in one pass and a
    one-wavefront finish (gnn_sup_head_fwd_f32): (loss 0-dim float32, n_correct 0-dim int64 or
    None, inv_valid float64 [1] = 1 / the number of rows that are not ignored, status int32 [1]).
    The selection is ``index`` (int64 [n], duplicates and negative entries as torch's), or
    ``count`` (int32 [N] from ``sup_head_count``, for a mask), or every row. Rows evaluated in
    double, sums in double in a fixed order: bit-identical from run to run. Bad index entries /
    labels address nothing, set bits 0 / 1 of ``status`` and make the loss NaN. Nothing of size
    [N, C] is allocated. None where the kernels do not take the layout (``_sup_head_operands``):
    the caller keeps torch's path."""
    _require_device(z, labels, index, count, status)
    if not _sup_head_operands(z, labels):
        return None
    if index is not None and count is not None:
        raise ValueError("give the selection as index or as count, not both")
    if index is not None and index.dtype != torch.int64:
        raise TypeError(f"index must be int64 (got {index.dtype}); a mask goes through "
                        "sup_head_count")
    if index is not None and index.dim() != 1:
        raise ValueError("index must be 1-D")
    N, C = z.shape
    if count is not None and (count.dtype != torch.int32 or count.shape != (N,)
                              or not count.is_contiguous()):
        raise ValueError(f"count must be a contiguous int32 [{N}] tensor")
    lib = _lib.load()
    dev = z.device
    labels = labels.contiguous()
    if index is not None:
        index = index.contiguous()
    n = N if index is None else index.shape[0]
    if status is None:
        status = _new_status(dev)
    if n == 0:  # the mean of nothing
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        correct = torch.zeros(1, dtype=torch.int64, device=dev) if want_correct else None
        inv_valid = torch.full((1,), float("inf"), dtype=torch.float64, device=dev)
    else:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        correct = torch.empty(1, dtype=torch.int64, device=dev) if want_correct else None
        inv_valid = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.gnn_sup_head_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        _lib.check(lib.gnn_sup_head_fwd_f32(
            z.data_ptr(), z.stride(0) if N > 1 else C, labels.data_ptr(), _lib.ptr(index),
            _lib.ptr(count), n, N, C, IGNORE_INDEX, loss.data_ptr(), _lib.ptr(correct),
            inv_valid.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
            _lib.stream_handle(dev)), "gnn_sup_head_fwd_f32")
    return (loss.reshape(()), None if correct is None else correct.reshape(()), inv_valid,
            status)


def sup_head_backward(z: torch.Tensor, labels: torch.Tensor, count: torch.Tensor | None,
                      upstream: torch.Tensor, inv_valid: torch.Tensor,
                      status: torch.Tensor,
                      out: torch.Tensor | None = None) -> torch.Tensor | None:
    """The gradient of ``sup_head_forward``'s loss with respect to the whole z, contiguous
    float32 [N, C] (gnn_sup_head_bwd_f32): one pass that writes every element once,
    ``count[r] (softmax(z[r]) - onehot(labels[r])) upstream inv_valid`` recomputed from the
    logits row in double, zeros for rows with count 0 or an ignored label (``count`` None:
    every row once). ``upstream`` (float32, one element), ``inv_valid`` and ``status`` stay on
    the device; a status that is not zero makes the whole gradient NaN. No zero fill, no
    scatter, no [n, C] intermediate, no float atomics. ``out``: a float32 [N, C] view with unit
    stride along C to write instead of a new tensor. None as ``sup_head_forward``."""
    _require_device(z, labels, count, upstream, inv_valid, status, out)
    if not _sup_head_operands(z, labels):
        return None
    N, C = z.shape
    if out is not None and (out.shape != (N, C) or out.dtype != torch.float32
                            or out.stride(1) != 1 or (N > 1 and out.stride(0) < C)):
        raise ValueError(f"out must be a float32 [{N}, {C}] view with unit stride along C")
    if upstream.dtype != torch.float32 or upstream.numel() != 1:
        raise TypeError("upstream must be one float32 element")
    if inv_valid.dtype != torch.float64 or inv_valid.numel() != 1:
        raise TypeError("inv_valid must be one float64 element")
    if status.dtype != torch.int32 or status.numel() != 1:
        raise TypeError("status must be one int32 element")
    if count is not None and (count.dtype != torch.int32 or count.shape != (N,)
                              or not count.is_contiguous()):
        raise ValueError(f"count must be a contiguous int32 [{N}] tensor")
    lib = _lib.load()
    dev = z.device
    labels = labels.contiguous()
    dz = out if out is not None else torch.empty((N, C), dtype=torch.float32, device=dev)
    if N:
        _lib.check(lib.gnn_sup_head_bwd_f32(
            z.data_ptr(), z.stride(0) if N > 1 else C, labels.data_ptr(), _lib.ptr(count), N, C,
            IGNORE_INDEX, upstream.data_ptr(), inv_valid.data_ptr(), status.data_ptr(),
            dz.data_ptr(), dz.stride(0) if N > 1 else C, _lib.stream_handle(dev)),
            "gnn_sup_head_bwd_f32")
    return dz


def han_semantic_supported(D: int, S: int, M: int) -> bool:
    """Whether the semantic-attention kernels take z [N, M, D] with a hidden width S
    (gnn_han_semantic_supported, the one source of the set)."""
    return bool(_lib.load().gnn_han_semantic_supported(int(D), int(S), int(M)))


def _han_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """A float32 [N, M, D] (or [N, D]) tensor as the kernels read it: unit stride along D,
    16-B aligned rows, pitches that are multiples of 4 floats and do not overlap; anything else
    is copied."""
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    D = t.shape[-1]
    st = t.stride()
    ok = st[-1] == 1 and t.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in st[:-1])
    if ok and t.dim() == 3:
        ok = (t.shape[1] <= 1 or st[1] >= D) and \
            (t.shape[0] <= 1 or st[0] >= t.shape[1] * max(st[1], D))
    elif ok:
        ok = t.shape[0] <= 1 or st[0] >= D
    return t if ok else t.contiguous()


def _han_pitches(t: torch.Tensor) -> tuple[int, int]:
    """(ld_n, ld_m) of a [N, M, D] tensor from ``_han_rows`` (a size-1 axis has no pitch of its
    own)."""
    N, M, D = t.shape
    ld_m = t.stride(1) if M > 1 else D
    ld_n = t.stride(0) if N > 1 else M * ld_m
    return ld_n, ld_m


def _han_operands(z, w1, b1, w2):
    _require_device(z, w1, b1, w2)
    if z.dim() != 3:
        raise ValueError(f"z must be [N, M, D] (got {tuple(z.shape)})")
    N, M, D = z.shape
    S = w1.shape[0] if w1.dim() == 2 else -1
    if w1.shape != (S, D) or b1.shape != (S,) or w2.numel() != S:
        raise ValueError(f"project must be Linear({D}, S) -> Tanh -> Linear(S, 1): got weights "
                         f"{tuple(w1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)}")
    for name, t in (("w1", w1), ("b1", b1), ("w2", w2)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if not han_semantic_supported(D, S, M):
        raise ValueError(f"semantic attention kernels do not take D={D}, S={S}, M={M} "
                         "(han_semantic_supported)")
    return (_han_rows(z, "z"), w1.contiguous(), b1.contiguous(), w2.reshape(-1).contiguous(),
            N, M, D, S)


def _han_workspace(lib, N, M, D, S, dev) -> torch.Tensor:
    return torch.empty(int(lib.gnn_han_semantic_workspace_bytes(N, M, D, S)), dtype=torch.uint8,
                       device=dev)


def han_semantic_forward(z: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                         w2: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """HAN's semantic attention (HAN/models/SemanticAttention.py:15-20) over z [N, M, D] with
    ``project = Linear(D, S) -> Tanh -> Linear(S, 1, bias=False)`` given as w1 [S, D], b1 [S],
    w2 [1, S] or [S] (gnn_han_semantic_fwd_f32): (out [N, D], beta [M]) with
    ``beta = softmax(project(z).mean(0))`` and ``out = (beta * z).sum(1)``. The scores run on
    the matrix cores with the [N M, S] intermediate kept in registers; beta stays on the
    device. A pitched z (unit stride along D, 16-B aligned rows) is read in place."""
    z, w1, b1, w2, N, M, D, S = _han_operands(z, w1, b1, w2)
    lib = _lib.load()
    dev = z.device
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    beta = torch.empty(M, dtype=torch.float32, device=dev)
    if N == 0:  # the mean of nothing
        return out, beta.fill_(float("nan"))
    ld_n, ld_m = _han_pitches(z)
    ws = _han_workspace(lib, N, M, D, S, dev)
    _lib.run("gnn_han_semantic_fwd_f32", z=z.data_ptr(), ld_n=ld_n, ld_m=ld_m, N=N, M=M, D=D,
             S=S, w1=w1.data_ptr(), b1=b1.data_ptr(), w2=w2.data_ptr(), w=None,
             beta=beta.data_ptr(), out=out.data_ptr(), ldo=D, ws=ws.data_ptr(),
             ws_bytes=ws.numel(), stream=_lib.stream_handle(dev))
    return out, beta


def han_semantic_backward(g: torch.Tensor, z: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                          w2: torch.Tensor, beta: torch.Tensor, need_dz: bool = True,
                          need_params: bool = True, dz_out: torch.Tensor | None = None):
    """The adjoint of ``han_semantic_forward`` (gnn_han_semantic_bwd_f32) for g = d out [N, D]
    and the forward's beta: (dz [N, M, D], dw1 [S, D], db1 [S], dw2 [S]); ``need_dz`` False
    skips the input-side pass (dz None), ``need_params`` False the parameter-side pass (the
    three None). tanh(W1 z + b1) is recomputed on the matrix cores; no [N M, S] tensor, no float
    atomics, bit-identical from run to run. ``dz_out``: a float32 [N, M, D] tensor the kernels
    can write (``_han_rows`` layout) instead of a new one."""
    _require_device(g, beta, dz_out)
    z, w1, b1, w2, N, M, D, S = _han_operands(z, w1, b1, w2)
    if g.shape != (N, D):
        raise ValueError(f"g must be [{N}, {D}] (got {tuple(g.shape)})")
    if beta.dtype != torch.float32 or beta.shape != (M,) or not beta.is_contiguous():
        raise ValueError(f"beta must be a contiguous float32 [{M}] tensor")
    lib = _lib.load()
    dev = z.device
    g = _han_rows(g, "g")
    dz = None
    if need_dz:
        dz = dz_out if dz_out is not None else torch.empty((N, M, D), dtype=torch.float32,
                                                           device=dev)
        if dz.shape != (N, M, D) or _han_rows(dz, "dz_out") is not dz:
            raise ValueError(f"dz_out must be a float32 [{N}, {M}, {D}] tensor with unit stride "
                             "along D and 16-B aligned rows")
    dw1 = db1 = dw2 = None
    if need_params:
        dw1 = torch.empty((S, D), dtype=torch.float32, device=dev)
        db1 = torch.empty(S, dtype=torch.float32, device=dev)
        dw2 = torch.empty(S, dtype=torch.float32, device=dev)
        if N == 0:
            dw1.zero_(), db1.zero_(), dw2.zero_()
    if N == 0 or not (need_dz or need_params):
        return dz, dw1, db1, dw2
    ld_n, ld_m = _han_pitches(z)
    ldd_n, ldd_m = _han_pitches(dz) if dz is not None else (M * D, D)
    ws = _han_workspace(lib, N, M, D, S, dev)
    _lib.run("gnn_han_semantic_bwd_f32", g=g.data_ptr(), ldg=g.stride(0) if N > 1 else D,
             z=z.data_ptr(), ld_n=ld_n, ld_m=ld_m, N=N, M=M, D=D, S=S, w1=w1.data_ptr(),
             b1=b1.data_ptr(), w2=w2.data_ptr(), beta=beta.data_ptr(), dz=_lib.ptr(dz),
             lddz_n=ldd_n, lddz_m=ldd_m, dw1=_lib.ptr(dw1), db1=_lib.ptr(db1),
             dw2=_lib.ptr(dw2), ws=ws.data_ptr(), ws_bytes=ws.numel(),
             stream=_lib.stream_handle(dev))
    return dz, dw1, db1, dw2


def han_tanh(x: torch.Tensor) -> torch.Tensor:
    """The semantic-attention kernels' tanh of a float32 tensor (gnn_han_tanh_f32): what the
    tests measure against float64."""
    _require_device(x)
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32 (got {x.dtype})")
    x = x.contiguous()
    y = torch.empty_like(x)
    if x.numel():
        _lib.run("gnn_han_tanh_f32", x=x.data_ptr(), y=y.data_ptr(), n=x.numel(),
                 stream=_lib.stream_handle(x.device))
    return y


# The fused layer is opt-in (set SAGE_FUSED_MIN_ROWS to the smallest frontier to fuse): at
# cfg4 it gains 2-3 % on layer 0 (62,479 rows: 110 vs 112 us) and loses on the 8,192-row
# layer 1 (33 vs 25 us) -- its gathers and MFMAs do not overlap, so it costs about their
# sum, while the unfused gather-mean and hipBLASLt GEMM each run near their own roofline.
# A producer/consumer form (8 gather + 8 MFMA waves, double-buffered LDS tiles) was slower
# still (129 us). tools/sage_layer_ab.py, profiles/r02z_sage_layer_ab*.log.
SAGE_FUSED_MIN_ROWS = None


def _rows16(t: torch.Tensor) -> bool:
    return (t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
            and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)


def sage_layer(table: torch.Tensor, nbr_idx: torch.Tensor, weight: torch.Tensor,
               self_src: torch.Tensor, self_idx: torch.Tensor | None = None,
               check: bool = True) -> torch.Tensor | None:
    """relu(W . cat[self, mean_j table[nbr_idx[:, j]]]) in ONE launch (gnn_sage_layer_f32):
    the inference SageLayer (GraphSAGE/GraphSAGE.py:15-20) fused with its MEAN Aggregator and
    input gathers (graph_utils.py:6, GraphSAGE.py:47-49). self = self_src[self_idx] or, with
    no index, self_src itself. None when the shape is not covered (the caller then runs the
    gather-mean + GEMM launches)."""
    _require_device(table, nbr_idx, weight, self_src, self_idx)
    if nbr_idx.dim() != 2 or weight.dim() != 2 or not (_rows16(table) and _rows16(self_src)):
        return None
    M, k = nbr_idx.shape
    feat = table.shape[1]
    H = weight.shape[0]
    if (SAGE_FUSED_MIN_ROWS is None or M < SAGE_FUSED_MIN_ROWS or k == 0
            or self_src.shape[1] != feat or weight.shape[1] != 2 * feat):
        return None
    if self_idx is None and self_src.shape[0] != M:
        return None
    lib = _lib.load()
    if not lib.gnn_sage_layer_supported(feat, H):
        return None
    w = weight.detach().to(torch.float32).contiguous()
    nbr_idx = _sage_idx(nbr_idx)
    if self_idx is not None:
        self_idx = _sage_self_idx(self_idx, M)
    out = torch.empty((M, H), dtype=torch.float32, device=table.device)
    err = _err_flag(table.device, check)
    _lib.check(lib.gnn_sage_layer_f32(
        table.data_ptr(), table.stride(0), table.shape[0], self_src.data_ptr(),
        self_src.stride(0), self_src.shape[0], _lib.ptr(self_idx), nbr_idx.data_ptr(),
        nbr_idx.stride(0), M, k, feat, w.data_ptr(), H, out.data_ptr(), H, err.data_ptr(),
        _lib.stream_handle(table.device)), "gnn_sage_layer_f32")
    if check:
        _check_err(err, "sage_layer")
    return out


def gather_rows(x: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None,
                check: bool = True) -> torch.Tensor:
    """out[i] = x[idx[i]] (torch.embedding semantics, one HIP launch). The result has the
    table's dtype, as torch.embedding's: a bfloat16 table gives bfloat16 rows
    (gnn_gather_rows_bf16); a float32 ``out=`` view of a bfloat16 table selects the widening
    gather (gnn_gather_rows_bf16_f32: ``x[idx].float()`` in the same launch)."""
    x = _sage_table(x, "x", "gather_rows", idx, out)
    idx = idx.to(torch.int64).contiguous().view(-1)
    n, F = idx.numel(), x.shape[1]
    if out is None:
        out = torch.empty((n, F), dtype=x.dtype, device=x.device)
    elif _bf16(x) and out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out of a bfloat16 table must be bfloat16 or float32 (got {out.dtype})")
    err = _err_flag(x.device, check)
    lib = _lib.load()
    if not _bf16(x):
        fn, name = lib.gnn_gather_rows_f32, "gnn_gather_rows_f32"
    elif _bf16(out):
        fn, name = lib.gnn_gather_rows_bf16, "gnn_gather_rows_bf16"
    else:
        fn, name = lib.gnn_gather_rows_bf16_f32, "gnn_gather_rows_bf16_f32"
    _lib.check(fn(x.data_ptr(), x.stride(0), x.shape[0], idx.data_ptr(), n, F, out.data_ptr(),
                  out.stride(0), err.data_ptr(), _lib.stream_handle(x.device)), name)
    if check:
        _check_err(err, "gather_rows")
    return out


# ---------------------------------------------------------------- GAT backward
# The GAT backward as two passes (gnn_gat_backward_rows_f32: prep + del, per-row statistics;
# gnn_gat_backward_nodes_recompute_f32: the transposed aggregation recomputing the edge
# weights) instead of three (prep, edge pass writing w / ds per (edge, head), node pass reading
# them back); the three-pass path serves the shapes the two-pass kernels refuse.
GAT_BWD_RECOMPUTE = True
GAT_BWD_SHORT_DEG = 8   # rows with <= 8 edges: several per wave in both passes


def _short_split(plan, rowptr, max_deg):
    """(rows of more than max_deg edges, rows of at most max_deg edges incl. the plan's
    small rows) of a plan's non-segmented rows, cached on the plan."""
    cache = plan.__dict__.setdefault("_bwd_short", {})
    if max_deg not in cache:
        mid, short = plan.gat_split(rowptr, max_deg)
        cache[max_deg] = (mid, torch.cat([short, plan.small_row]).contiguous())
    return cache[max_deg]


def _bwd_recompute_ok(heads: int, fh: int, ldw: int) -> bool:
    """The shapes gnn_gat_backward_rows_f32 / _nodes_recompute_f32 take (16-B aligned tensors):
    the row pass's LDS (2 feat + heads <= 1152 floats) and the node pass's lane layout (fh / VW
    lanes per head a power of two, feat <= 256 VW; VW = 4 when fh and the Wh pitch are
    multiples of 4)."""
    feat = heads * fh
    vw = 4 if fh % 4 == 0 and ldw % 4 == 0 else 1
    lanes = fh // vw
    nv = -(-feat // vw)
    lpr = 0 if nv > 256 else (64 if nv > 64 else 1 << max(0, (nv - 1).bit_length()))
    return (2 * feat + heads <= 1152 and fh % vw == 0 and lanes & (lanes - 1) == 0
            and 0 < lanes <= lpr)


def _gat_backward_recompute(g, wh, el, er, stats, y, dy, a_src, a_dst, heads, fh,
                            negative_slope, mode, elu, dropout_p, seed, seg_len, mark,
                            dy_dropout=None):
    """The two-pass backward; None when the kernels refuse the shape (GNN_E_UNSUPPORTED)."""
    n = g.n_rows
    feat = heads * fh
    if not _bwd_recompute_ok(heads, fh, wh.stride(0)):
        return None
    dev = wh.device
    stream = _lib.stream_handle(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    sl = seg_len if seg_len is not None else seg_len_for(feat, GAT_SEG_BYTES)
    plan = g.plan(sl)
    short_ok = 8 * (2 * feat + heads) <= 1152
    rows, short = (_short_split(plan, g.rowptr, GAT_BWD_SHORT_DEG) if short_ok
                   else (plan.row_list(), plan.small_row[:0]))
    a_src = a_src.detach().reshape(-1).contiguous().float()
    a_dst = a_dst.detach().reshape(-1).contiguous().float()
    dout = torch.empty((n, feat), **f32)
    nstat = torch.empty((n, heads, 4), **f32)  # {el, lse, D, 0} per (row, head)
    dl = torch.empty((n, heads), **f32)
    del_part = torch.empty((max(plan.n_seg, 1), heads), **f32)
    seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF
    mark("rows")

    def rows_pass(dy, dp, ds):
        return _lib.invoke(
            "gnn_gat_backward_rows_ex_f32", rowptr=g.rowptr.data_ptr(), col=g.col.data_ptr(),
            n_rows=n, wh=wh.data_ptr(), ldw=wh.stride(0), heads=heads, fh=fh, el=el.data_ptr(),
            er=er.data_ptr(), lse=stats.data_ptr(), dy=dy.data_ptr(), y=y.data_ptr(), ldo=feat,
            elu=int(elu), negative_slope=float(negative_slope), mode=int(mode),
            dropout_p=float(dropout_p), dropout_seed=seed64, dout=dout.data_ptr(),
            nstat=nstat.data_ptr(), d_el=dl.data_ptr(), **plan.segments(), rows=rows.data_ptr(),
            n_rows_list=rows.numel(), short_rows=short.data_ptr(), n_short=short.numel(),
            del_part=del_part.data_ptr(), a_dst=a_dst.data_ptr() if GAT_ER_RECOMPUTE else None,
            dy_dropout_p=float(dp), dy_dropout_seed=int(ds) & 0xFFFFFFFFFFFFFFFF, stream=stream)

    if dy_dropout is not None:  # the upstream mask inside the prep where it takes the shape
        rc = rows_pass(dy, dy_dropout[0], dy_dropout[1])
        if rc == _lib.E_UNSUPPORTED:
            rc = rows_pass(dropout_rows(dy, dy_dropout[0], dy_dropout[1]), 0.0, 0)
    else:
        rc = rows_pass(dy, 0.0, 0)
    if rc == _lib.E_UNSUPPORTED:  # (_bwd_recompute_ok passed: an unaligned view)
        mark(None)
        return None
    _lib.check(rc, "gnn_gat_backward_rows_ex_f32")
    if g.symmetric and dropout_p == 0.0:
        # A^T = A: node j's in-edges are row j's (ascending sources); no edge ids needed
        rowptr_t, src_t, eid_t, gt = g.rowptr, g.col, None, g
    else:
        rowptr_t, src_t, eid_t, gt = g.transpose_eid()
    pt = gt.plan(sl)
    rows_t, short_t = _short_split(pt, rowptr_t, GAT_BWD_SHORT_DEG)
    dwh = torch.empty((n, feat), **f32)
    der = torch.empty((n, heads), **f32)
    part = torch.empty((max(pt.n_seg, 1), feat + heads), **f32)
    mark("nodes")
    rc = _lib.invoke(
        "gnn_gat_backward_nodes_recompute_f32", rowptr_t=rowptr_t.data_ptr(),
        src_t=src_t.data_ptr(), eid_t=_lib.ptr(eid_t), n_nodes=n, heads=heads, fh=fh,
        dout=dout.data_ptr(), nstat=nstat.data_ptr(), wh=wh.data_ptr(), ldw=wh.stride(0),
        er=er.data_ptr(), d_el=dl.data_ptr(), a_src=a_src.data_ptr(), a_dst=a_dst.data_ptr(),
        negative_slope=float(negative_slope), mode=int(mode), dropout_p=float(dropout_p),
        dropout_seed=seed64, dwh=dwh.data_ptr(), der=der.data_ptr(), **pt.segments(),
        rows=rows_t.data_ptr(), n_rows_list=rows_t.numel(), short_rows=short_t.data_ptr(),
        n_short=short_t.numel(), part=part.data_ptr(), stream=stream)
    if rc == _lib.E_UNSUPPORTED:
        # the row pass's outputs are the three-pass path's prep + edge outputs but for w / ds:
        # start over there (a shape both refuse is one the three-pass kernels also cover)
        mark(None)
        return None
    _lib.check(rc, "gnn_gat_backward_nodes_recompute_f32")
    mark(None)
    return dwh, dout, dl, der


def gat_backward(g: CsrGraph, wh: torch.Tensor, el: torch.Tensor, er: torch.Tensor,
                 stats: torch.Tensor, y: torch.Tensor, dy: torch.Tensor, a_src: torch.Tensor,
                 a_dst: torch.Tensor, heads: int, fh: int, negative_slope: float, mode: int,
                 elu: bool, dropout_p: float = 0.0, seed: int = 0,
                 seg_len: int | None = None, timings: list | None = None,
                 dy_dropout: tuple | None = None):
    """dWh (incl. the el/er terms), del, der for one GAT layer: two HIP passes (row pass,
    recomputing node pass; GAT_BWD_RECOMPUTE) or, for the shapes those refuse, three.

    Returns (dwh [N, H*fh], dout [N, H*fh], del [N, H], der [N, H]). ``timings`` (a list):
    (pass name, start event, end event) of each pass on the current stream is appended
    (bench.py's per-kernel backward times). ``dy_dropout`` = (p, seed): dy is the gradient of
    ``dropout_rows(y, p, seed)`` (the hidden dropout fused into the layer); its mask is applied
    to dy here -- inside the backward prep where the two-pass kernels take the shape."""
    _require_device(wh, dy)
    n = g.n_rows
    feat = heads * fh
    dev = wh.device
    lib = _lib.load()
    stream = _lib.stream_handle(dev)
    dy = dy.contiguous()
    y = y.contiguous()

    def mark(name):
        if timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(dev))
            if timings and timings[-1][2] is None:
                timings[-1] = (timings[-1][0], timings[-1][1], ev)
            if name:
                timings.append((name, ev, None))

    if GAT_BWD_RECOMPUTE:
        r = _gat_backward_recompute(g, wh, el, er, stats, y, dy, a_src, a_dst, heads, fh,
                                    negative_slope, mode, elu, dropout_p, seed, seg_len, mark,
                                    dy_dropout)
        if r is not None:
            return r
    if dy_dropout is not None:
        dy = dropout_rows(dy, dy_dropout[0], dy_dropout[1])
    dout = torch.empty((n, feat), dtype=torch.float32, device=dev)
    D = torch.empty((n, heads), dtype=torch.float32, device=dev)
    mark("prep")
    _lib.check(lib.gnn_gat_backward_prep_f32(dy.data_ptr(), y.data_ptr(), feat, n, heads, fh,
                                             int(elu), dout.data_ptr(), D.data_ptr(), stream),
               "gnn_gat_backward_prep_f32")
    sl = seg_len if seg_len is not None else seg_len_for(feat, GAT_SEG_BYTES)
    plan = g.plan(sl)
    E = g.nnz
    w_edge = torch.empty((max(E, 1), heads), dtype=torch.float32, device=dev)
    ds_edge = torch.empty((max(E, 1), heads), dtype=torch.float32, device=dev)
    dl = torch.zeros((n, heads), dtype=torch.float32, device=dev)
    del_part = torch.empty((max(plan.n_seg, 1), heads), dtype=torch.float32, device=dev)
    rows = plan.row_list()
    mark("edges")
    _lib.run(
        "gnn_gat_backward_edges_f32", rowptr=g.rowptr.data_ptr(), col=g.col.data_ptr(), n_rows=n,
        wh=wh.data_ptr(), ldw=wh.stride(0), heads=heads, fh=fh, el=el.data_ptr(),
        er=er.data_ptr(), lse=stats.data_ptr(), dout=dout.data_ptr(), D=D.data_ptr(),
        negative_slope=float(negative_slope), mode=int(mode), dropout_p=float(dropout_p),
        dropout_seed=int(seed) & 0xFFFFFFFFFFFFFFFF, w_edge=w_edge.data_ptr(),
        ds_edge=ds_edge.data_ptr(), d_el=dl.data_ptr(), **plan.segments(), rows=rows.data_ptr(),
        n_rows_list=rows.numel(), del_part=del_part.data_ptr(), stream=stream)
    rowptr_t, src_t, eid_t, gt = g.transpose_eid()
    pt = gt.plan(sl)
    rows_t = pt.row_list()
    dwh = torch.empty((n, feat), dtype=torch.float32, device=dev)
    der = torch.zeros((n, heads), dtype=torch.float32, device=dev)
    part = torch.empty((max(pt.n_seg, 1), feat + heads), dtype=torch.float32, device=dev)
    a_src = a_src.contiguous().float()
    a_dst = a_dst.contiguous().float()
    # one node pass for every head (the kernel sums der over groups of 8 heads itself)
    mark("nodes")
    _lib.run(
        "gnn_gat_backward_nodes_f32", rowptr_t=rowptr_t.data_ptr(), src_t=src_t.data_ptr(),
        eid_t=eid_t.data_ptr(), n_nodes=n, heads=heads, fh=fh, dout=dout.data_ptr(),
        w_edge=w_edge.data_ptr(), ds_edge=ds_edge.data_ptr(), d_el=dl.data_ptr(),
        a_src=a_src.data_ptr(), a_dst=a_dst.data_ptr(), dwh=dwh.data_ptr(), der=der.data_ptr(),
        **pt.segments(), rows=rows_t.data_ptr(), n_rows_list=rows_t.numel(),
        part=part.data_ptr(), stream=stream)
    mark(None)
    return dwh, dout, dl, der


# ------------------------------------------------- GTN: values over fixed CSR patterns (gtn.hip)
# A pattern is a CsrGraph whose values are not read; values travel beside it as [C, nnz]
# channel-major float32. The C entries take 1 <= C <= 8: more channels are looped here.
GTN_MAX_CHANNELS = 8


def masked_product_class_limits() -> tuple[int, int]:
    """(lane_max, wave_chunk) of gnn_masked_product_f32: the longest walked row summed by the P
    entry's own lane, and how many walked entries a wavefront takes at a time above it."""
    import ctypes
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().gnn_masked_product_class_limits(ctypes.byref(a), ctypes.byref(b)),
               "gnn_masked_product_class_limits")
    return int(a.value), int(b.value)


def _entry_rows(g: CsrGraph) -> torch.Tensor:
    """The row id of every stored entry (int64 [nnz], cached on the graph)."""
    r = g._plans.get("_entry_rows")
    if r is None:
        r = torch.repeat_interleave(
            torch.arange(g.n_rows, device=g.device, dtype=torch.int64),
            g.rowptr[1:] - g.rowptr[:-1])
        g._plans["_entry_rows"] = r
    return r


def _values(v: torch.Tensor, g: CsrGraph, name: str) -> torch.Tensor:
    if v.dim() != 2 or v.shape[1] != g.nnz or v.shape[0] < 1:
        raise ValueError(f"{name} must be [C, {g.nnz}] (got {tuple(v.shape)})")
    return v


def _product_shapes(mode, a, b, p):
    if mode not in (0, 1):
        raise ValueError("mode is 0 ((A . B) o P) or 1 ((A . B^T) o P)")
    n, k = a.n_rows, a.n_cols
    if mode == 0:
        ok, m = b.n_rows == k, b.n_cols
    else:
        ok, m = b.n_cols == k, b.n_rows
    if not ok or (p.n_rows, p.n_cols) != (n, m):
        raise ValueError(f"shapes do not chain in mode {mode}: A [{a.n_rows}, {a.n_cols}], "
                         f"B [{b.n_rows}, {b.n_cols}], P [{p.n_rows}, {p.n_cols}]")
    return n, k, m


def _segment_sum(terms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """Sums of consecutive runs of ``terms`` [T, ...] along axis 0 (an empty run gives 0)."""
    if lengths.numel() == 0 or terms.shape[0] == 0:
        return terms.new_zeros((lengths.numel(),) + tuple(terms.shape[1:]))
    return torch.segment_reduce(terms.contiguous(), "sum", lengths=lengths, axis=0, unsafe=True)


def masked_product_torch(mode: int, a: CsrGraph, av: torch.Tensor, b: CsrGraph,
                         bv: torch.Tensor, p: CsrGraph) -> torch.Tensor:
    """``masked_product`` restated in torch ops (any device, any float dtype): the walked row
    of every P entry expanded, each term's partner looked up with one ``searchsorted`` in the
    searched operand's row-major keys, and the terms of an entry summed as one run. The CPU
    path and the oracle of the kernel; its memory grows with the number of walked entries."""
    n, k, m = _product_shapes(mode, a, b, p)
    _values(av, a, "a values"), _values(bv, b, "b values")
    dev = p.device
    prow, pcol = _entry_rows(p), p.col.to(torch.int64)
    wg, wv, lg, lv = (a, av, b, bv) if mode == 0 else (b, bv, a, av)
    wrow = prow if mode == 0 else pcol
    lo = wg.rowptr[wrow]
    deg = wg.rowptr[wrow + 1] - lo
    total = int(deg.sum()) if deg.numel() else 0
    first = torch.cumsum(deg, 0) - deg
    ent = torch.repeat_interleave(torch.arange(p.nnz, device=dev, dtype=torch.int64), deg)
    q = torch.repeat_interleave(lo - first, deg) + torch.arange(total, device=dev,
                                                                dtype=torch.int64)
    wc = wg.col[q].to(torch.int64)
    key = wc * lg.n_cols + pcol[ent] if mode == 0 else prow[ent] * lg.n_cols + wc
    lkey = _entry_rows(lg) * lg.n_cols + lg.col.to(torch.int64)
    if lkey.numel() > 1 and bool((lkey[1:] <= lkey[:-1]).any()):
        raise IndexError("the searched operand's rows must ascend strictly")
    if lkey.numel() == 0 or total == 0:
        return av.new_zeros((av.shape[0], p.nnz))
    pos = torch.searchsorted(lkey, key).clamp_(max=lkey.numel() - 1)
    hit = lkey[pos] == key
    term = torch.where(hit, wv[:, q] * lv[:, pos], torch.zeros((), dtype=av.dtype, device=dev))
    return _segment_sum(term.t(), deg).t().contiguous()


def _ws_product(lib, n, k, m, a, b, p, C, dev):
    nbytes = int(lib.gnn_masked_product_workspace_bytes(n, k, m, a.nnz, b.nnz, p.nnz, C))
    if nbytes < 0:
        _lib.check(nbytes, "gnn_masked_product_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def masked_product(mode: int, a: CsrGraph, av: torch.Tensor, b: CsrGraph, bv: torch.Tensor,
                   p: CsrGraph, validate: bool = True) -> torch.Tensor:
    """The values [C, nnz_p] of a sparse product on the pattern P (gnn_masked_product_f32).
    mode 0: (A . B) o P with A [n, k] walked and B [k, m] searched; mode 1: (A . B^T) o P with
    A [n, k] searched and B [m, k] walked. The searched operand's rows ascend strictly.
    ``validate``: check the operands on the device first (one stream synchronisation); pass
    False for patterns checked before. CPU operands run ``masked_product_torch``."""
    n, k, m = _product_shapes(mode, a, b, p)
    av, bv = _values(av, a, "a values"), _values(bv, b, "b values")
    if av.shape[0] != bv.shape[0]:
        raise ValueError("A and B carry the same number of channels")
    if not av.is_cuda:
        return masked_product_torch(mode, a, av, b, bv, p)
    _require_device(av, bv, a.rowptr, b.rowptr, p.rowptr)
    if av.dtype != torch.float32 or bv.dtype != torch.float32:
        raise TypeError("masked_product takes float32 values")
    C, dev = av.shape[0], av.device
    if C > GTN_MAX_CHANNELS:
        return torch.cat([masked_product(mode, a, av[c:c + 8], b, bv[c:c + 8], p,
                                         validate and c == 0) for c in range(0, C, 8)])
    av, bv = av.contiguous(), bv.contiguous()
    out = torch.empty((C, p.nnz), dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = _ws_product(lib, n, k, m, a, b, p, C, dev)
    rc = _lib.invoke(
        "gnn_masked_product_f32", mode=mode, a_rowptr=a.rowptr.data_ptr(),
        a_col=_lib.ptr(a.col) if a.nnz else None, a_val=av.data_ptr() if a.nnz else None,
        nnz_a=a.nnz, b_rowptr=b.rowptr.data_ptr(), b_col=_lib.ptr(b.col) if b.nnz else None,
        b_val=bv.data_ptr() if b.nnz else None, nnz_b=b.nnz, p_rowptr=p.rowptr.data_ptr(),
        p_col=_lib.ptr(p.col) if p.nnz else None, nnz_p=p.nnz, n=n, k=k, m=m, C=C,
        out=out.data_ptr() if p.nnz else None, validate=int(bool(validate)),
        workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=_lib.stream_handle(dev))
    if rc == _lib.E_ARG:
        raise IndexError("masked_product: a column id out of range, a malformed rowptr or a "
                         "searched row that does not ascend strictly")
    _lib.check(rc, "gnn_masked_product_f32")
    return out


def _edge_rows_ok(F: int, *ts) -> bool:
    """Whether the edge kernels take these feature rows: F % 4 == 0, 4 <= F <= 256, float32 on
    the device (contiguous rows of such an F are 16-B aligned)."""
    return F % 4 == 0 and 4 <= F <= 256 and all(t.is_cuda and t.dtype == torch.float32
                                                for t in ts)


def _offdiag(g: CsrGraph) -> torch.Tensor:
    """bool [nnz]: the entries with row != col (cached on the graph)."""
    mk = g._plans.get("_offdiag")
    if mk is None:
        mk = _entry_rows(g) != g.col.to(torch.int64)
        g._plans["_offdiag"] = mk
    return mk


def edge_aggregate_torch(g: CsrGraph, v: torch.Tensor, x: torch.Tensor,
                         skip_diag: bool = False) -> torch.Tensor:
    """``edge_aggregate`` restated in torch ops: the terms v[c, e] x[.., col_e, :] of a row
    summed as one run (any device, any float dtype)."""
    _values(v, g, "v")
    C = v.shape[0]
    col = g.col.to(torch.int64)
    rows = x[col][None] if x.dim() == 2 else x[:, col]                 # [1 | C, nnz, F]
    vv = v * _offdiag(g) if skip_diag else v
    term = (vv[:, :, None] * rows).permute(1, 0, 2)                     # [nnz, C, F]
    out = _segment_sum(term, g.rowptr[1:] - g.rowptr[:-1])              # [n_rows, C, F]
    return out.permute(1, 0, 2).contiguous().reshape(C, g.n_rows, x.shape[-1])


def edge_aggregate(g: CsrGraph, v: torch.Tensor, x: torch.Tensor,
                   skip_diag: bool = False) -> torch.Tensor:
    """Y[c, r, :] = sum over e in row r, in CSR order, of v[c, e] X[col_e, :]
    (gnn_edge_aggregate_f32): v [C, nnz]; x [n_cols, F] shared by the channels (each row
    gathered once for all C outputs) or [C, n_cols, F] per channel. ``skip_diag`` leaves out
    the entries with row == col. Shapes outside F % 4 == 0, 4 <= F <= 256 and CPU tensors run
    ``edge_aggregate_torch``."""
    _values(v, g, "v")
    C, F = v.shape[0], x.shape[-1]
    if x.shape[-2] != g.n_cols or (x.dim() == 3 and x.shape[0] != C) or x.dim() not in (2, 3):
        raise ValueError(f"x must be [{g.n_cols}, F] or [{C}, {g.n_cols}, F] "
                         f"(got {tuple(x.shape)})")
    if not _edge_rows_ok(F, v, x):
        return edge_aggregate_torch(g, v, x, skip_diag)
    if C > GTN_MAX_CHANNELS:
        return torch.cat([edge_aggregate(g, v[c:c + 8], x if x.dim() == 2 else x[c:c + 8],
                                         skip_diag) for c in range(0, C, 8)])
    v, x = v.contiguous(), x.contiguous()
    y = torch.empty((C, g.n_rows, F), dtype=torch.float32, device=v.device)
    _lib.run("gnn_edge_aggregate_f32", rowptr=g.rowptr.data_ptr(),
             col=_lib.ptr(g.col) if g.nnz else None, val=v.data_ptr() if g.nnz else None,
             nnz=g.nnz, n_rows=g.n_rows, n_cols=g.n_cols, X=x.data_ptr() if g.nnz else None,
             ldx=F, x_stride=0 if x.dim() == 2 else g.n_cols, Y=y.data_ptr(), ldy=F, F=F, C=C,
             skip_diag=int(bool(skip_diag)), stream=_lib.stream_handle(v.device))
    return y


def edge_dot_torch(g: CsrGraph, grad: torch.Tensor, x: torch.Tensor,
                   skip_diag: bool = False) -> torch.Tensor:
    """``edge_dot`` restated in torch ops (any device, any float dtype)."""
    dv = (grad[:, _entry_rows(g)] * x[g.col.to(torch.int64)][None]).sum(-1)
    return dv * _offdiag(g) if skip_diag else dv


def edge_dot(g: CsrGraph, grad: torch.Tensor, x: torch.Tensor,
             skip_diag: bool = False) -> torch.Tensor:
    """dv[c, e] = <grad[c, row_e, :], x[col_e, :]> (gnn_edge_dot_f32), the edge-value adjoint
    of ``edge_aggregate`` over a shared input: grad [C, n_rows, F], x [n_cols, F]; with
    ``skip_diag`` the entries with row == col get 0. Other shapes and CPU tensors run
    ``edge_dot_torch``."""
    if grad.dim() != 3 or grad.shape[1] != g.n_rows or x.shape != (g.n_cols, grad.shape[2]):
        raise ValueError(f"grad must be [C, {g.n_rows}, F] and x [{g.n_cols}, F] (got "
                         f"{tuple(grad.shape)}, {tuple(x.shape)})")
    C, F = grad.shape[0], grad.shape[2]
    if not _edge_rows_ok(F, grad, x):
        return edge_dot_torch(g, grad, x, skip_diag)
    if C > GTN_MAX_CHANNELS:
        return torch.cat([edge_dot(g, grad[c:c + 8], x, skip_diag) for c in range(0, C, 8)])
    grad, x = grad.contiguous(), x.contiguous()
    dv = torch.empty((C, g.nnz), dtype=torch.float32, device=grad.device)
    if g.nnz:
        _lib.run("gnn_edge_dot_f32", rowptr=g.rowptr.data_ptr(), col=g.col.data_ptr(), nnz=g.nnz,
                 n_rows=g.n_rows, n_cols=g.n_cols, G=grad.data_ptr(), ldg=F, X=x.data_ptr(),
                 ldx=F, dv=dv.data_ptr(), F=F, C=C, skip_diag=int(bool(skip_diag)),
                 stream=_lib.stream_handle(grad.device))
    return dv


def edge_rowsum_torch(g: CsrGraph, v: torch.Tensor, skip_diag: bool = False) -> torch.Tensor:
    """``edge_rowsum`` restated in torch ops (any device, any float dtype)."""
    vv = v * _offdiag(g) if skip_diag else v
    return _segment_sum(vv.t(), g.rowptr[1:] - g.rowptr[:-1]).t().contiguous()


def edge_rowsum(g: CsrGraph, v: torch.Tensor, skip_diag: bool = False) -> torch.Tensor:
    """d[c, r] = sum over e in row r, in CSR order, of v[c, e] (gnn_edge_rowsum_f32); over the
    column view of a pattern these are the column sums of the reference's ``norm``."""
    _values(v, g, "v")
    if not (v.is_cuda and v.dtype == torch.float32):
        return edge_rowsum_torch(g, v, skip_diag)
    v = v.contiguous()
    y = torch.empty((v.shape[0], g.n_rows), dtype=torch.float32, device=v.device)
    _lib.run("gnn_edge_rowsum_f32", rowptr=g.rowptr.data_ptr(),
             col=_lib.ptr(g.col) if g.nnz else None, val=v.data_ptr() if g.nnz else None,
             nnz=g.nnz, n_rows=g.n_rows, C=v.shape[0], skip_diag=int(bool(skip_diag)),
             y=y.data_ptr(), stream=_lib.stream_handle(v.device))
    return y


# ---------------------------------------------------------------- GATNE (csrc/gatne.hip)
def gatne_supported(E: int, U: int, A: int, T: int) -> bool:
    """Whether the GATNE attention kernels take the widths (gnn_gatne_supported, the one source
    of the set): U, A in {16, 32, 64, 128}, E a power of two in [16, 256], 1 <= T <= 8."""
    return bool(_lib.load().gnn_gatne_supported(int(E), int(U), int(A), int(T)))


def typed_gather_sum(table: torch.Tensor, nbr: torch.Tensor, agg_func: str = "SUM",
                     check: bool = True) -> torch.Tensor:
    """u[b, t] = sum (``'SUM'``) or mean (``'MEAN'``) over k of the rows ``nbr[b, t, k]`` of
    ``table`` (gnn_typed_gather_sum_f32): ``table`` [N, T, W] is read at type t (GATNE's
    ``node_type_embeddings``), ``table`` [N, W] the same row for every type (a feature table).
    nbr: int64 [B, T, K]; W a multiple of 4; float32 [B, T, W], fp32 sums in k order. An id
    outside [0, N) is skipped: ``check`` raises IndexError for it (one host read)."""
    if agg_func not in ("SUM", "MEAN"):
        raise ValueError("please choice else aggregator!")
    _require_device(table, nbr)
    if table.dtype != torch.float32:
        raise TypeError(f"table must be float32 (got {table.dtype})")
    if nbr.dim() != 3 or table.dim() not in (2, 3):
        raise ValueError("nbr must be [B, T, K] and table [N, T, W] or [N, W]")
    B, T, K = nbr.shape
    if table.dim() == 3 and table.shape[1] != T:
        raise ValueError(f"table holds {table.shape[1]} types, nbr {T}")
    W = table.shape[-1]
    if W % 4:
        raise ValueError(f"the row width must be a multiple of 4 (got {W})")
    if not table.is_contiguous() or table.data_ptr() % 16:
        table = table.clone(memory_format=torch.contiguous_format)
    nbr = nbr.to(torch.int64).contiguous()
    u = torch.empty((B, T, W), dtype=torch.float32, device=table.device)
    if B == 0 or T == 0 or W == 0:
        return u
    if K == 0:
        if agg_func == "MEAN":
            _empty_reduction(0)
        return u.fill_(float("nan") if agg_func == "MEAN" else 0.0)
    err = _err_flag(table.device, check)
    ld_n, ld_t = (T * W, W) if table.dim() == 3 else (W, 0)
    _lib.run("gnn_typed_gather_sum_f32", table=table.data_ptr(), ld_n=ld_n, ld_t=ld_t,
             n_table=table.shape[0], nbr=nbr.data_ptr(), B=B, T=T, K=K, W=W,
             scale=1.0 if agg_func == "SUM" else 1.0 / K, u=u.data_ptr(), ldu=W,
             err_flag=err.data_ptr(), stream=_lib.stream_handle(table.device))
    if check:
        _check_err(err, "typed_gather_sum")
    return u


class GatneOrder(NamedTuple):
    """Rows sorted by edge type (``gatne_order``): ``perm`` int32 [B] (the batch row at every
    sorted position), ``seg`` int32 [T + 2] (seg[t] = the first position of a type >= t;
    seg[T] .. seg[T + 1] = B are the rows of no type)."""
    perm: torch.Tensor
    seg: torch.Tensor
    T: int


def gatne_order(types: torch.Tensor, T: int, check: bool = True) -> GatneOrder:
    """The stable order of the batch rows by edge type (gnn_gatne_order): ``perm`` is exactly
    numpy's stable argsort of ``types`` and ``seg[:T + 1]`` its bincount / cumsum. A type outside
    [0, T) sorts last; ``check`` raises IndexError for it (one host read), unchecked such rows
    come out of the attention stage as NaN."""
    _require_device(types)
    if types.dim() != 1:
        raise ValueError("types must be [B]")
    T = int(T)
    types = types.to(torch.int64).contiguous()
    B = types.numel()
    dev = types.device
    lib = _lib.load()
    nbytes = int(lib.gnn_gatne_order_workspace_bytes(B, T))
    if nbytes < 0:
        raise ValueError(f"gatne_order does not take B={B}, T={T} (1 <= T <= 8)")
    perm = torch.empty(B, dtype=torch.int32, device=dev)
    seg = torch.empty(T + 2, dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = _err_flag(dev, check)
    _lib.run("gnn_gatne_order", types=types.data_ptr(), B=B, T=T, perm=perm.data_ptr(),
             seg=seg.data_ptr(), status=status.data_ptr(), workspace=ws.data_ptr(),
             workspace_bytes=ws.numel(), stream=_lib.stream_handle(dev))
    if check and int(status.item()) != 0:
        raise IndexError(f"gatne_order: edge type outside [0, {T})")
    return GatneOrder(perm, seg, T)


def _gatne_operands(c, u, w1, w2, m, order):
    _require_device(c, u, w1, w2, m, order.perm, order.seg)
    if c.dim() != 2 or u.dim() != 3 or w1.dim() != 3 or m.dim() != 3:
        raise ValueError("c must be [B, E], u [B, T, U], w1 [T, U, A], m [T, U, E]")
    B, E = c.shape
    T, U, A = w1.shape
    if (u.shape != (B, T, U) or m.shape != (T, U, E) or w2.numel() != T * A
            or order.perm.numel() != B or order.seg.numel() != T + 2 or order.T != T):
        raise ValueError("the GATNE operands do not belong together")
    for name, t in (("c", c), ("u", u), ("w1", w1), ("w2", w2), ("m", m)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if not gatne_supported(E, U, A, T):
        raise ValueError(f"the GATNE kernels do not take E={E}, U={U}, A={A}, T={T} "
                         "(gatne_supported)")
    if c.stride(1) != 1 or c.data_ptr() % 16 or (B > 1 and (c.stride(0) % 4 or c.stride(0) < E)):
        c = c.clone(memory_format=torch.contiguous_format)

    def dense(t):
        return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else \
            t.clone(memory_format=torch.contiguous_format)

    return c, dense(u), dense(w1), dense(w2), dense(m), B, T, E, U, A


def gatne_attend_forward(c: torch.Tensor, u: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
                         m: torch.Tensor, order: GatneOrder):
    """GATNE's edge-type attention (GATNE_Pytorch/models/GATNE.py:80-95) for centre rows c
    [B, E], neighbour sums u [B, T, U] and the rows' types given as ``order = gatne_order(types,
    T)`` (gnn_gatne_attend_fwd_f32): with r the type of row b, ``alpha = softmax_t(tanh(u_t
    w1[r]) . w2[r])``, ``e = c + (sum_t alpha_t u_t) m[r]``, ``out = e / max(|e|, 1e-12)``.
    Returns (out [B, E], alpha [B, T], inv [B] = 1 / max(|e|, 1e-12)). The per-row weight
    tensors of the reference are never formed."""
    c, u, w1, w2, m, B, T, E, U, A = _gatne_operands(c, u, w1, w2, m, order)
    dev = c.device
    out = torch.empty((B, E), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, T), dtype=torch.float32, device=dev)
    inv = torch.empty(B, dtype=torch.float32, device=dev)
    if B:
        _lib.run("gnn_gatne_attend_fwd_f32", c=c.data_ptr(), ldc=c.stride(0) if B > 1 else E,
                 u=u.data_ptr(), perm=order.perm.data_ptr(), seg=order.seg.data_ptr(), B=B, T=T,
                 E=E, U=U, A=A, w1=w1.data_ptr(), w2=w2.data_ptr(), m=m.data_ptr(),
                 out=out.data_ptr(), ldo=E, alpha=alpha.data_ptr(), inv=inv.data_ptr(),
                 stream=_lib.stream_handle(dev))
    return out, alpha, inv


def gatne_attend_backward(g: torch.Tensor, out: torch.Tensor, u: torch.Tensor,
                          alpha: torch.Tensor, inv: torch.Tensor, w1: torch.Tensor,
                          w2: torch.Tensor, m: torch.Tensor, order: GatneOrder,
                          need_du: bool = True, need_params: bool = True):
    """The adjoint of ``gatne_attend_forward`` for g = d out [B, E] and the forward's out, alpha
    and inv (gnn_gatne_attend_bwd_f32): (dc [B, E], du [B, T, U], dw1 [T, U, A], dw2 [T, A],
    dm [T, U, E]); ``need_du`` / ``need_params`` False leave None in their places. The tanh is
    recomputed; a type absent from the batch gets exact zeros; sums in a fixed order, no float
    atomics, bit-identical from run to run."""
    _require_device(g, out, alpha, inv)
    g, u, w1, w2, m, B, T, E, U, A = _gatne_operands(g, u, w1, w2, m, order)
    if (out.shape != (B, E) or alpha.shape != (B, T) or inv.shape != (B,)
            or not (out.is_contiguous() and alpha.is_contiguous() and inv.is_contiguous())):
        raise ValueError("out, alpha and inv must be the forward's tensors")
    dev = g.device
    f32 = dict(dtype=torch.float32, device=dev)
    dc = torch.empty((B, E), **f32)
    du = torch.empty((B, T, U), **f32) if need_du else None
    dw1 = dw2 = dm = None
    if need_params:
        dw1, dw2, dm = (torch.empty(s, **f32) for s in ((T, U, A), (T, A), (T, U, E)))
    lib = _lib.load()
    ws = torch.empty(max(int(lib.gnn_gatne_attend_workspace_bytes(B, T, E, U, A)), 16),
                     dtype=torch.uint8, device=dev)
    _lib.run("gnn_gatne_attend_bwd_f32", g=g.data_ptr(), ldg=g.stride(0) if B > 1 else E,
             out=out.data_ptr(), ldo=E, u=u.data_ptr(), alpha=alpha.data_ptr(),
             inv=inv.data_ptr(), perm=order.perm.data_ptr(), seg=order.seg.data_ptr(), B=B, T=T,
             E=E, U=U, A=A, w1=w1.data_ptr(), w2=w2.data_ptr(), m=m.data_ptr(),
             dc=dc.data_ptr(), du=_lib.ptr(du), dw1=_lib.ptr(dw1), dw2=_lib.ptr(dw2),
             dm=_lib.ptr(dm), ws=ws.data_ptr(), ws_bytes=ws.numel(),
             stream=_lib.stream_handle(dev))
    return dc, du, dw1, dw2, dm
