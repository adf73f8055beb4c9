"""Every C-ABI entry with a multi-piece workspace refuses a buffer one byte short of its own
query with GNN_E_ARG, before anything reaches the device: the size it checks is the size the
query states. Smallest legal dimensions; host buffers stand in for the device pointers, which
are never dereferenced. gnn_cover_build is left out: it reads two row offsets from the device
before it can size its workspace."""
import ctypes

import pytest

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from graphneuralnetwork_amd import _lib
    return _lib.load(build_if_missing=True)


class _Host:
    """A zeroed host buffer passed wherever an entry takes a pointer, and the small host arrays
    the entries read themselves (per-peer counts, fan-outs, capacities, pointer tables)."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(4096)
        self.p = ctypes.addressof(self.buf)
        self.i64 = (ctypes.c_int64 * 8)()
        self.out = ctypes.addressof(self.i64)
        self.zero = (ctypes.c_int64 * 1)(0)                              # recv_edges, world 1
        self.ones = (ctypes.c_int64 * 1)(1)                              # fanouts, caps
        self.seed = (ctypes.c_uint64 * 1)(7)
        self.table = (ctypes.c_void_p * 1)(self.p)                       # nbrs[0]


# name of the entry -> (its query, the query's arguments, the entry's arguments with
# "WS" where (workspace, workspace_bytes) go)
def _cases(h):
    p, out = h.p, h.out
    a = ctypes.addressof
    return {
        "gnn_spmm_tasks_build": ("gnn_spmm_tasks_workspace_bytes", (1,),
                                 (p, 1, 64, 1, p, 0, out, "WS", None)),
        "gnn_column_order": ("gnn_column_order_workspace_bytes", (1,),
                             (None, 0, 1, -1, p, p, None, "WS", None)),
        "gnn_xcd_hub_plan_build": ("gnn_xcd_hub_plan_workspace_bytes", (1, 0),
                                   (p, None, 1, 0, 8, 1, 4, 1, 0, 0, out, "WS", None)),
        "gnn_cover_send_partials": ("gnn_cover_send_workspace_bytes", (0,),
                                    (None, None, None, a(h.zero), 1, 0, 1, 0, p, None, None, "WS",
                                     None)),
        "gnn_gcn_adjacency_build": ("gnn_gcn_adjacency_workspace_bytes", (0, 1),
                                    (None, None, 0, 1, "WS", out, None)),
        "gnn_hub_plan_build": ("gnn_hub_plan_workspace_bytes", (1,),
                               (None, 0, 1, 1, p, None, p, "WS", None)),
        "gnn_frontier_build": ("gnn_frontier_workspace_bytes", (1,),
                               (None, 0, None, 0, 1, "WS", p, p, None)),
        "gnn_sample_layers": ("gnn_sample_layers_workspace_bytes", (1,),
                              (p, p, 1, p, 1, 1, a(h.ones), a(h.seed), 0, None, a(h.ones),
                               a(h.table), None, None, p, "WS", None)),
        "gnn_sage_maps_transpose": ("gnn_sage_maps_transpose_workspace_bytes", (0, 0),
                                    (None, None, 0, 0, 0, 0, p, None, p, "WS", None)),
        "gnn_sage_maps_transpose_nbr": ("gnn_sage_maps_transpose_nbr_workspace_bytes", (0, 0),
                                        (None, 0, 0, 0, 0, p, None, p, "WS", None)),
        "gnn_sage_scatter_concat_f32": ("gnn_sage_scatter_concat_workspace_bytes", (0, 0, 4),
                                        (None, 8, p, None, 0, 0, 4, 0, None, 4, "WS", None)),
        "gnn_sage_scatter_concat_maxpool_f32": (
            "gnn_sage_scatter_concat_maxpool_workspace_bytes", (0, 1, 4),
            (None, 8, None, 4, p, None, 0, 1, 4, 0, None, 4, "WS", None)),
        "gnn_sage_scatter_agg_f32": ("gnn_sage_scatter_agg_workspace_bytes", (0, 0, 4),
                                     (None, 4, p, None, 0, 0, 4, 0, None, 4, "WS", None)),
        "gnn_sage_scatter_agg_maxpool_f32": (
            "gnn_sage_scatter_agg_maxpool_workspace_bytes", (0, 1, 4),
            (None, 4, None, 4, p, None, 0, 1, 4, 0, None, 4, "WS", None)),
        "gnn_relation_product_count": ("gnn_relation_product_workspace_bytes", (0, 0, 0, 0, 0),
                                       (p, None, 0, p, None, 0, 0, 0, 0, p, out, "WS", None)),
        "gnn_relation_product_fill": ("gnn_relation_product_workspace_bytes", (0, 0, 0, 0, 0),
                                      (p, None, 0, p, None, 0, 0, 0, 0, p, None, 0, "WS", None)),
        "gnn_induced_subgraph_map": ("gnn_induced_subgraph_workspace_bytes", (0, 0),
                                     (None, 0, 0, p, "WS", None)),
        "gnn_induced_subgraph_count": ("gnn_induced_subgraph_workspace_bytes", (0, 0),
                                       (p, None, 0, 0, None, 0, p, p, "WS", None)),
        "gnn_induced_subgraph_fill": ("gnn_induced_subgraph_workspace_bytes", (0, 0),
                                      (p, None, None, 0, 0, None, 0, p, None, None, 0, p, "WS",
                                       None)),
    }


ENTRIES = sorted(_cases(_Host()))


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_byte_short_is_refused(lib, entry):
    h = _Host()
    query, dims, args = _cases(h)[entry]
    need = getattr(lib, query)(*dims)
    assert need > 0, (query, dims, need)
    call = []
    for v in args:
        call.extend((h.p, need - 1) if v == "WS" else (v,))
    assert getattr(lib, entry)(*call) == E_ARG
    assert bytes(h.buf) == bytes(4096)                   # the stand-in buffer was never written
