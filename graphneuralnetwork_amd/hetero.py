"""Metapath graphs of a heterogeneous graph, built on the device.

The reference's HAN loader turns a relation (paper x author, paper x field) into a metapath
graph on the host (``HeteroGraph.get_mate_path_graph``, HAN/utils/data_utils.py:85-89):

    mate_path_adj = HGraphs[key] * HGraphs[key].T     # scipy sparse product
    mate_path_adj[mate_path_adj > 0] = 1
    return mate_path_adj.toarray()                    # dense N x N

Here the same structure is a boolean sparse x sparse product written straight into a
``CsrGraph`` (csrc/relation_product.hip: ``gnn_relation_product_count`` / ``_fill``), which
``han.GATConv`` / ``HANLayer`` take as they take the dense array: row i holds the set union
of the B-rows named by row i of A, ascending, without duplicates -- the edge order
``graph.from_dense(reference_output, "positive")`` gives. No dense N x N array and nothing
sized by the number of partial products exists at any point.

The loader's mini-batch path slices those dense arrays, ``HG_adj[idx][:, idx]`` once per step and
metapath (``collect_f.__call__``, HAN/utils/data_utils.py:92-101). Here the slice is the induced
subgraph of a ``CsrGraph`` written as a ``CsrGraph`` [b, b] (csrc/induced_subgraph.hip:
``gnn_induced_subgraph_map`` / ``_count`` / ``_fill``; ``induced_subgraphs``), rows ascending by
position, values carried, and ``collect_f`` is the reference's class over it.

The reference's GTN takes its T edge types as one dense ``[N, N, T]`` tensor (GTN/run.py). Here
``edge_type_graph`` turns the relations into an ``EdgeTypeGraph``: the union pattern U, each
relation's values over it, and the cached product patterns S_{l+1} = (S_l . U) > 0 that
``gtn.GTN_Model`` computes values on (csrc/gtn.hip).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .graph import CsrGraph, from_coo, from_torch_sparse


def _operand(x, device=None) -> CsrGraph:
    """A relation operand as a CsrGraph: a CsrGraph, a torch sparse COO / CSR tensor (every
    stored entry an edge) or a ``(row, col, (n_rows, n_cols))`` triple."""
    if isinstance(x, CsrGraph):
        g = x
    elif isinstance(x, torch.Tensor):
        if x.layout == torch.strided:
            raise TypeError("a relation is sparse: pass a torch sparse tensor, a CsrGraph or a "
                            "(row, col, shape) triple")
        g = from_torch_sparse(x, "all")
    elif isinstance(x, (tuple, list)) and len(x) == 3:
        row, col, shape = x
        row = torch.as_tensor(row, dtype=torch.int64)
        col = torch.as_tensor(col, dtype=torch.int64, device=row.device)
        if row.shape != col.shape or row.dim() != 1:
            raise ValueError("row and col must be 1-D and of the same length")
        n_rows, n_cols = (int(v) for v in shape)
        if row.numel() and (int(row.min()) < 0 or int(row.max()) >= n_rows):
            raise IndexError("relation row index out of range")
        g = from_coo(row, col, torch.ones(row.numel(), device=row.device), n_rows, n_cols,
                     check=False)  # the product checks the column ids
    else:
        raise TypeError("a relation operand is a CsrGraph, a torch sparse tensor or a "
                        "(row, col, shape) triple")
    return g if device is None else g.to(device)


def class_limits() -> tuple[int, int]:
    """(short_max, mid_max): the largest row upper bound ub = sum of the named B-rows' lengths
    built by one wavefront in registers, and the largest built in an LDS table; rows above
    are built in a bitmap (gnn_relation_product_class_limits)."""
    s, m = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().gnn_relation_product_class_limits(ctypes.byref(s), ctypes.byref(m)),
               "gnn_relation_product_class_limits")
    return int(s.value), int(m.value)


def relation_product(a, b) -> CsrGraph:
    """C = (A . B) > 0 as a CsrGraph with unit values: A [n, k], B [k, m]. Device operands run
    the HIP kernels; CPU operands run ``relation_product_torch``."""
    a = _operand(a)
    b = _operand(b, a.device)
    if a.n_cols != b.n_rows:
        raise ValueError(f"shapes do not chain: A is [{a.n_rows}, {a.n_cols}], "
                         f"B is [{b.n_rows}, {b.n_cols}]")
    if not a.rowptr.is_cuda:
        return relation_product_torch(a, b)
    dev = a.device
    n, k, m = a.n_rows, a.n_cols, b.n_cols
    lib = _lib.load()
    nbytes = int(lib.gnn_relation_product_workspace_bytes(n, k, m, a.nnz, b.nnz))
    if nbytes < 0:
        _lib.check(nbytes, "gnn_relation_product_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nnz = ctypes.c_int64(0)
    stream = _lib.stream_handle(dev)
    operands = dict(a_rowptr=a.rowptr.data_ptr(), a_col=_lib.ptr(a.col) if a.nnz else None,
                    nnz_a=a.nnz, b_rowptr=b.rowptr.data_ptr(),
                    b_col=_lib.ptr(b.col) if b.nnz else None, nnz_b=b.nnz, n=n, k=k, m=m,
                    workspace=ws.data_ptr(), workspace_bytes=nbytes, stream=stream)
    rc = _lib.invoke("gnn_relation_product_count", c_rowptr=rowptr.data_ptr(),
                     nnz_out=ctypes.addressof(nnz), **operands)
    if rc == _lib.E_ARG:
        raise IndexError("relation column id out of range (or a malformed rowptr)")
    _lib.check(rc, "gnn_relation_product_count")
    col = torch.empty(int(nnz.value), dtype=torch.int32, device=dev)
    _lib.run("gnn_relation_product_fill", c_rowptr=rowptr.data_ptr(),
             c_col=col.data_ptr() if col.numel() else None, nnz_c=col.numel(), **operands)
    return CsrGraph(rowptr, col, torch.ones(col.numel(), dtype=torch.float32, device=dev), n, m)


def relation_product_torch(a, b) -> CsrGraph:
    """``relation_product`` restated in torch ops (any device): every partial product expanded,
    key = row * m + col, ``torch.unique``. The CPU path and the oracle of the kernels; its
    memory grows with the number of partial products, which the kernels' does not."""
    a = _operand(a)
    b = _operand(b, a.device)
    if a.n_cols != b.n_rows:
        raise ValueError(f"shapes do not chain: A is [{a.n_rows}, {a.n_cols}], "
                         f"B is [{b.n_rows}, {b.n_cols}]")
    dev = a.device
    n, k, m = a.n_rows, a.n_cols, b.n_cols
    ac, bc = a.col.to(torch.int64), b.col.to(torch.int64)
    if (ac.numel() and (int(ac.min()) < 0 or int(ac.max()) >= k)) or \
            (bc.numel() and (int(bc.min()) < 0 or int(bc.max()) >= m)):
        raise IndexError("relation column id out of range")
    a_row = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64),
                                    a.rowptr[1:] - a.rowptr[:-1])
    deg = (b.rowptr[1:] - b.rowptr[:-1])[ac]           # products of each entry of A
    first = torch.cumsum(deg, 0) - deg
    total = int(deg.sum()) if deg.numel() else 0
    src = torch.repeat_interleave(b.rowptr[:-1][ac] - first, deg) + \
        torch.arange(total, device=dev, dtype=torch.int64)
    key = torch.unique(torch.repeat_interleave(a_row, deg) * m + bc[src])
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if key.numel():
        torch.cumsum(torch.bincount(key // m, minlength=n), 0, out=rowptr[1:])
    col = (key % m).to(torch.int32).contiguous() if key.numel() else \
        torch.zeros(0, dtype=torch.int32, device=dev)
    return CsrGraph(rowptr, col, torch.ones(col.numel(), dtype=torch.float32, device=dev), n, m)


def metapath_graph(b) -> CsrGraph:
    """The metapath graph of a relation B [n, k]: (B . B^T) > 0, [n, n], symmetric. B^T is
    built on the operand's device (``CsrGraph.transpose``)."""
    b = _operand(b)
    bt = b.transpose()
    if bt is b:  # a square relation marked symmetric is its own transpose
        bt = CsrGraph(b.rowptr, b.col, b.val, b.n_rows, b.n_cols)
    g = relation_product(b, bt)
    g.symmetric = True
    return g


def _positive_entries(rel, device) -> CsrGraph:
    """The entries > 0 of a valued relation as a CsrGraph on ``device`` (None: the operand's
    own device; scipy matrices go to the ROCm device when there is one). A negative entry
    raises: under the reference's ``adj[adj > 0] = 1`` it would leave non-unit values behind,
    and this builder carries no values."""
    if isinstance(rel, CsrGraph):
        row = torch.repeat_interleave(
            torch.arange(rel.n_rows, device=rel.device, dtype=torch.int64),
            rel.rowptr[1:] - rel.rowptr[:-1])
        col, val, shape = rel.col.to(torch.int64), rel.val, (rel.n_rows, rel.n_cols)
    elif isinstance(rel, torch.Tensor):
        if rel.layout == torch.strided:
            if rel.dim() != 2:
                raise TypeError("a relation is a 2-D matrix")
            idx = (rel != 0).nonzero()
            row, col, val, shape = idx[:, 0], idx[:, 1], rel[rel != 0], tuple(rel.shape)
        else:
            coo = rel.to_sparse_coo() if rel.layout != torch.sparse_coo else rel
            row, col = coo._indices()[0], coo._indices()[1]
            val, shape = coo._values(), tuple(rel.shape)
    elif hasattr(rel, "tocoo"):  # a scipy sparse matrix: never imported here, only recognised
        coo = rel.tocoo()
        row = torch.from_numpy(coo.row.astype("int64"))
        col = torch.from_numpy(coo.col.astype("int64"))
        val = torch.from_numpy(coo.data.astype("float64"))
        shape = tuple(int(v) for v in coo.shape)
        if device is None and torch.cuda.is_available():
            device = "cuda"
    else:
        raise TypeError("a relation is a scipy sparse matrix, a torch tensor or a CsrGraph")
    if val.numel() and bool((val < 0).any()):
        raise ValueError("a relation with negative entries has no metapath graph here: the "
                         "reference's adj[adj > 0] = 1 would keep non-unit values")
    keep = val > 0
    row, col = row[keep], col[keep]
    if device is not None:
        row, col = row.to(device), col.to(device)
    return from_coo(row, col, torch.ones(row.numel(), device=row.device), shape[0], shape[1])


class HeteroGraph:
    """The reference's ``HeteroGraph`` (HAN/utils/data_utils.py:74-89) over the device builder:
    same constructor argument, ``__iter__``, ``__len__`` and ``get_mate_path_graph(key)``, but
    each metapath graph is a ``CsrGraph`` (what ``han.HANLayer`` takes) instead of a dense
    array. Relations may be scipy sparse matrices (when scipy is installed; it is never
    imported here), torch sparse or dense tensors, or ``CsrGraph``s; entries > 0 are edges and a
    negative entry raises ``ValueError``. ``device``: where the graphs are built (default: the
    relation's own device; the ROCm device for scipy matrices when there is one)."""

    def __init__(self, HGraphs: dict, device=None):
        self.HGraphs = HGraphs
        self.device = device

    def __iter__(self):
        for key in self.HGraphs.keys():
            yield self.get_mate_path_graph(key)

    def __len__(self):
        return len(self.HGraphs)

    def get_mate_path_graph(self, mate_path) -> CsrGraph:
        return metapath_graph(_positive_entries(self.HGraphs[mate_path], self.device))


# ------------------------------------------------------------------ mini-batches: A[idx][:, idx]
STATUS_BAD_IDX, STATUS_BAD_GRAPH, STATUS_REPEAT = 1, 2, 4   # bits of the kernels' status word


def subgraph_class_limits() -> tuple[int, int, int]:
    """(short_max, mid_max, lds_bits) of the induced-subgraph fill: the largest kept count of a
    row sorted by one wavefront, the largest sorted in LDS, and the largest batch whose rank
    bitmap lives in LDS (gnn_induced_subgraph_class_limits)."""
    s, m, b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().gnn_induced_subgraph_class_limits(
        ctypes.byref(s), ctypes.byref(m), ctypes.byref(b)), "gnn_induced_subgraph_class_limits")
    return int(s.value), int(m.value), int(b.value)


def _batch_index(idx, device) -> torch.Tensor:
    """A batch as an int64 [b] tensor on ``device``: a 1-D tensor or array, or what a DataLoader
    over an index array hands a collate_fn (a list of 0-d tensors, numpy integers or ints)."""
    if isinstance(idx, torch.Tensor):
        t = idx
    else:
        idx = list(idx)
        if idx and isinstance(idx[0], torch.Tensor):
            t = torch.stack([torch.as_tensor(v) for v in idx])
        else:
            t = torch.tensor([int(v) for v in idx], dtype=torch.int64)
    if t.dim() != 1:
        raise ValueError("a batch is a 1-D list of node ids")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("node ids are integers")
    return t.to(device=device, dtype=torch.int64).contiguous()


def _raise_status(status: int) -> None:
    if status & STATUS_BAD_IDX:
        raise IndexError("batch id out of range for the graph")
    if status & STATUS_BAD_GRAPH:
        raise IndexError("graph column id out of range (or a malformed rowptr) in a selected row")
    if status & STATUS_REPEAT:
        raise ValueError("a selected row repeats a selected column: coalesce the graph first")


def _square(gs) -> int:
    n = gs[0].n_rows
    for g in gs:
        if g.n_rows != g.n_cols:
            raise ValueError(f"an induced subgraph needs a square graph, got [{g.n_rows}, "
                             f"{g.n_cols}]")
        if g.n_rows != n:
            raise ValueError("the graphs of one batch share their node set")
    return n


def induced_subgraph_torch(g: CsrGraph, idx) -> CsrGraph:
    """``induced_subgraph`` restated in torch ops (any device): the selected rows expanded, each
    column looked up in the stably sorted ``idx`` with two ``searchsorted`` calls, the runs
    expanded, and a stable argsort of ``row * b + position``. The CPU path and the oracle of the
    kernels; its memory grows with the selected rows' full lengths, which the kernels' does not."""
    n = _square([g])
    dev = g.device
    idx = _batch_index(idx, dev)
    b = idx.numel()
    if b and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError("batch id out of range for the graph")
    lo_e, hi_e = g.rowptr[idx], g.rowptr[idx + 1]
    if b and (int(lo_e.min()) < 0 or int((hi_e - lo_e).min()) < 0 or int(hi_e.max()) > g.nnz):
        raise IndexError("malformed rowptr in a selected row")
    deg = hi_e - lo_e
    total = int(deg.sum()) if b else 0
    first = torch.cumsum(deg, 0) - deg
    row = torch.repeat_interleave(torch.arange(b, device=dev, dtype=torch.int64), deg)
    src = torch.repeat_interleave(lo_e - first, deg) + \
        torch.arange(total, device=dev, dtype=torch.int64)
    c = g.col[src].to(torch.int64)
    if total and (int(c.min()) < 0 or int(c.max()) >= n):
        raise IndexError("graph column id out of range in a selected row")
    sorted_idx, perm = torch.sort(idx, stable=True)
    lo = torch.searchsorted(sorted_idx, c, right=False)
    run = torch.searchsorted(sorted_idx, c, right=True) - lo   # positions that hold the column
    kept = int(run.sum()) if total else 0
    ent = torch.repeat_interleave(torch.arange(total, device=dev, dtype=torch.int64), run)
    off = torch.arange(kept, device=dev, dtype=torch.int64) - \
        torch.repeat_interleave(torch.cumsum(run, 0) - run, run)
    pos = perm[lo[ent] + off] if kept else torch.zeros(0, dtype=torch.int64, device=dev)
    key = row[ent] * b + pos
    order = torch.argsort(key, stable=True)
    key = key[order]
    if kept > 1 and bool((key[1:] == key[:-1]).any()):
        raise ValueError("a selected row repeats a selected column: coalesce the graph first")
    rowptr = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    if kept:
        torch.cumsum(torch.bincount(key // b, minlength=b), 0, out=rowptr[1:])
    out = CsrGraph(rowptr, pos[order].to(torch.int32).contiguous(),
                   g.val[src[ent][order]].contiguous(), b, b)
    out.symmetric = g.symmetric
    return out


def induced_subgraphs(gs, idx) -> list[CsrGraph]:
    """``[A[idx][:, idx] for A in gs]`` as CsrGraphs [b, b], values carried, each row in ascending
    position order. ``gs``: square CsrGraphs over one node set, on one device; ``idx``: the
    batch's node ids, in any order, repeats allowed. Device operands run csrc/
    induced_subgraph.hip: one map of the batch, a count per graph, ONE host read of the totals
    and the status word, a fill per graph and a second read of the status word (a repeated
    (row, position) pair shows in the fill). CPU operands run ``induced_subgraph_torch``."""
    gs = list(gs)
    if not gs:
        return []
    n = _square(gs)
    dev = gs[0].device
    if not gs[0].rowptr.is_cuda:
        return [induced_subgraph_torch(g, idx) for g in gs]
    idx = _batch_index(idx, dev)
    b, M = idx.numel(), len(gs)
    lib = _lib.load()
    nbytes = int(lib.gnn_induced_subgraph_workspace_bytes(n, b))
    if nbytes < 0:
        _lib.check(nbytes, "gnn_induced_subgraph_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = _lib.stream_handle(dev)
    batch = dict(idx=idx.data_ptr() if b else None, b=b, n=n, status=status.data_ptr(),
                 workspace=ws.data_ptr(), workspace_bytes=nbytes, stream=stream)
    _lib.run("gnn_induced_subgraph_map", **batch)
    rowptrs = torch.empty((M, b + 1), dtype=torch.int64, device=dev)
    for m, g in enumerate(gs):
        _lib.run("gnn_induced_subgraph_count", rowptr=g.rowptr.data_ptr(),
                 col=_lib.ptr(g.col) if g.nnz else None, nnz=g.nnz,
                 c_rowptr=rowptrs[m].data_ptr(), **batch)
    host = torch.cat([rowptrs[:, b], status.to(torch.int64)]).cpu()  # the one read before the fills
    _raise_status(int(host[M]))
    out = []
    for m, g in enumerate(gs):
        nnz_c = int(host[m])
        col = torch.empty(nnz_c, dtype=torch.int32, device=dev)
        val = torch.empty(nnz_c, dtype=torch.float32, device=dev)
        _lib.run("gnn_induced_subgraph_fill", rowptr=g.rowptr.data_ptr(),
                 col=_lib.ptr(g.col) if g.nnz else None, val=_lib.ptr(g.val) if g.nnz else None,
                 nnz=g.nnz, c_rowptr=rowptrs[m].data_ptr(), c_col=col.data_ptr() if nnz_c else None,
                 c_val=val.data_ptr() if nnz_c else None, nnz_c=nnz_c, **batch)
        c = CsrGraph(rowptrs[m], col, val, b, b)
        c.symmetric = g.symmetric
        out.append(c)
    _raise_status(int(status))
    return out


def induced_subgraph(g: CsrGraph, idx) -> CsrGraph:
    """``A[idx][:, idx]`` of one square CsrGraph (see ``induced_subgraphs``)."""
    return induced_subgraphs([g], idx)[0]


class collect_f:
    """The reference's ``collect_f`` (HAN/utils/data_utils.py:92-101), the ``collate_fn`` of its
    mini-batch loaders: same three constructor arguments, ``HGs_adj``, ``features`` (fp32) and
    ``labels`` (int64), and ``__call__(data)`` returns ``([A[idx][:, idx] for A in HGs_adj],
    features[idx], labels[idx])``. ``HGs`` is a ``HeteroGraph`` (iterated once, as the reference
    does) or a list of ``CsrGraph``s, and then each slice is a ``CsrGraph`` [b, b] built by
    ``induced_subgraphs``; a list of dense arrays keeps the reference's own line. ``device``:
    where the graphs, features and labels live (default: where the graphs are)."""

    def __init__(self, HGs, features, labels, device=None):
        graphs = list(HGs)
        if all(isinstance(g, CsrGraph) for g in graphs):
            if device is None and graphs:
                device = graphs[0].device
            self.HGs_adj = [g if device is None or g.device == torch.device(device)
                            else g.to(device) for g in graphs]
            self._csr = True
        else:
            self.HGs_adj = [torch.as_tensor(g).to(device) if device is not None
                            else torch.as_tensor(g) for g in graphs]
            self._csr = False
        self.features = torch.as_tensor(features).to(torch.float32)
        self.labels = torch.as_tensor(labels).to(torch.int64)
        if device is not None:
            self.features, self.labels = self.features.to(device), self.labels.to(device)

    def __call__(self, data):
        idx = _batch_index(data, self.features.device)
        if self._csr:
            adj = induced_subgraphs(self.HGs_adj, idx)
        else:
            adj = [a[idx.to(a.device)][:, idx.to(a.device)] for a in self.HGs_adj]
        return adj, self.features[idx], self.labels[idx]


# ------------------------------------------------- edge-type graphs: the GTN input on CSR patterns
class Pattern:
    """A CSR pattern (rows ascending, no duplicates; a CsrGraph whose values are not read) with
    its cached column view: ``T`` is the pattern of the transpose, and values [C, nnz] over this
    pattern become values over ``T`` as ``v[:, perm]`` (``T.perm`` is the inverse, so every
    move between the two layouts is a gather)."""

    def __init__(self, g: CsrGraph):
        self.g = g
        self._t: "Pattern | None" = None
        self._perm = None
        self.next: "Pattern | None" = None       # (this . U) > 0, set by EdgeTypeGraph
        self.checked: set = set()                # operand sets the product kernel has validated

    @property
    def nnz(self) -> int:
        return self.g.nnz

    @property
    def T(self) -> "Pattern":
        if self._t is None:
            _, _, eid, gt = self.g.transpose_eid()
            t = Pattern(gt)
            inv = torch.empty_like(eid)
            inv[eid] = torch.arange(eid.numel(), device=eid.device, dtype=eid.dtype)
            self._perm, t._perm = eid, inv
            self._t, t._t = t, self
        return self._t

    @property
    def perm(self) -> torch.Tensor:
        self.T
        return self._perm


class EdgeTypeGraph:
    """The T relations of a heterogeneous graph over one node set, as the sparse GTN reads
    them: ``U`` the union pattern (CsrGraph [n, n], columns ascending, no duplicates) and
    ``tval`` [T, nnz_U] each relation's value at each union entry (0 where it has none). The
    product patterns S_1 = U, S_{l+1} = (S_l . U) > 0 are built once (``relation_product``) and
    cached here with their column views."""

    def __init__(self, U: CsrGraph, tval: torch.Tensor):
        self.U, self.tval = U, tval
        self.n, self.T = U.n_rows, int(tval.shape[0])
        self._pattern = Pattern(U)
        self._tval_t = None

    @property
    def device(self) -> torch.device:
        return self.U.device

    @property
    def pattern(self) -> Pattern:
        return self._pattern

    @property
    def tval_t(self) -> torch.Tensor:
        """``tval`` over the column view of U (the values of the transposed relations)."""
        if self._tval_t is None:
            self._tval_t = self.tval[:, self._pattern.perm].contiguous()
        return self._tval_t

    def product_pattern(self, p: Pattern) -> Pattern:
        """(p . U) > 0 as a Pattern, built once per p."""
        if p.next is None:
            p.next = Pattern(relation_product(p.g, self.U))
        return p.next

    def S(self, l: int) -> Pattern:
        """S_1 = U and S_{l+1} = (S_l . U) > 0."""
        p = self._pattern
        for _ in range(l - 1):
            p = self.product_pattern(p)
        return p

    def to(self, device) -> "EdgeTypeGraph":
        return EdgeTypeGraph(self.U.to(device), self.tval.to(device))


def _relation_coo(rel):
    """(row, col, val, n_rows, n_cols) of one relation, every stored entry kept."""
    if isinstance(rel, CsrGraph):
        row = torch.repeat_interleave(
            torch.arange(rel.n_rows, device=rel.device, dtype=torch.int64),
            rel.rowptr[1:] - rel.rowptr[:-1])
        return row, rel.col.to(torch.int64), rel.val, rel.n_rows, rel.n_cols
    if isinstance(rel, torch.Tensor):
        if rel.dim() != 2:
            raise TypeError("a relation is a 2-D matrix")
        if rel.layout == torch.strided:
            idx = (rel != 0).nonzero()
            return idx[:, 0], idx[:, 1], rel[rel != 0], rel.shape[0], rel.shape[1]
        coo = rel.to_sparse_coo() if rel.layout != torch.sparse_coo else rel
        return coo._indices()[0], coo._indices()[1], coo._values(), rel.shape[0], rel.shape[1]
    if hasattr(rel, "tocoo"):  # a scipy sparse matrix: never imported here, only recognised
        coo = rel.tocoo()
        return (torch.from_numpy(coo.row.astype("int64")), torch.from_numpy(coo.col.astype("int64")),
                torch.from_numpy(coo.data.astype("float64")), int(coo.shape[0]), int(coo.shape[1]))
    raise TypeError("a relation is a scipy sparse matrix, a torch tensor or a CsrGraph")


def edge_type_graph(relations, device=None) -> EdgeTypeGraph:
    """The ``EdgeTypeGraph`` of T square relations over one node set: a list of ``CsrGraph``s,
    torch sparse or dense 2-D tensors or scipy sparse matrices (recognised, never imported), or
    the reference's dense ``[N, N, T]`` tensor (GTN/run.py builds it from the edge lists).
    Duplicates within one relation are summed, as scipy's constructor does; entries equal to 0
    are not edges; a negative value raises ``ValueError`` (the reference's ``deg_inv == inf``
    test only catches a degree of +0). ``device``: where the graph lives (default: the
    relations' own)."""
    if isinstance(relations, torch.Tensor) or hasattr(relations, "ndim") and \
            not hasattr(relations, "tocoo"):
        stack = torch.as_tensor(relations)
        if stack.dim() != 3 or stack.shape[0] != stack.shape[1]:
            raise ValueError(f"a dense edge-type tensor is [N, N, T] (got {tuple(stack.shape)})")
        relations = [stack[:, :, t] for t in range(stack.shape[2])]
    relations = list(relations)
    if not relations:
        raise ValueError("an edge-type graph needs at least one relation")
    keys, vals, n = [], [], None
    for rel in relations:
        row, col, val, nr, nc = _relation_coo(rel)
        if nr != nc or (n is not None and nr != n):
            raise ValueError("the relations are square and share one node set")
        n = nr
        if device is not None:
            row, col, val = row.to(device), col.to(device), val.to(device)
        if val.numel() and bool((val < 0).any()):
            raise ValueError("a relation with negative entries has no GTN normalisation here: "
                             "the reference's deg_inv == inf test only catches a degree of +0")
        if row.numel() and (int(row.min()) < 0 or int(row.max()) >= n or int(col.min()) < 0
                            or int(col.max()) >= n):
            raise IndexError("relation index out of range")
        key, inverse = torch.unique(row.to(torch.int64) * n + col.to(torch.int64),
                                    return_inverse=True)
        total = torch.zeros(key.numel(), dtype=torch.float64, device=key.device)
        total.index_add_(0, inverse, val.to(torch.float64))     # duplicates summed
        keep = total != 0
        keys.append(key[keep])
        vals.append(total[keep])
    dev = keys[0].device
    union = torch.unique(torch.cat(keys))
    tval = torch.zeros((len(relations), union.numel()), dtype=torch.float32, device=dev)
    for t, (key, val) in enumerate(zip(keys, vals)):
        tval[t, torch.searchsorted(union, key)] = val.to(torch.float32)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if union.numel():
        torch.cumsum(torch.bincount(union // n, minlength=n), 0, out=rowptr[1:])
    U = CsrGraph(rowptr, (union % n).to(torch.int32).contiguous(),
                 torch.ones(union.numel(), dtype=torch.float32, device=dev), n, n)
    return EdgeTypeGraph(U, tval)
