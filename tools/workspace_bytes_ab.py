"""Workspace queries of two builds of the library side by side (no device needed).

    python tools/workspace_bytes_ab.py PARENT_LIB RESULT_LIB > profiles/<name>_bytes.txt

Loads both with plain ctypes.CDLL, calls every gnn_*_workspace_bytes of the multi-piece
layouts on the dimensions below and prints one line per call: both values and whether they are
equal (negative codes included). Exit status 1 if any differ. The rocPRIM terms depend on the
ROCm release, so only two libraries on one machine compare.
"""
import ctypes
import sys

I31 = 2 ** 31 - 1
M1, M10 = 10 ** 6, 10 ** 7                 # nodes of cfg2 / cfg3 and of cfg4 / the north star
E10, E20, E100 = 10 ** 7, 2 * 10 ** 7, 10 ** 8
EDGE = [0, 1, 32, 33, 64, 65]              # both sides of a 256-byte piece: 8- and 4-byte items
B, F1, F2 = 8192, 25, 10                   # cfg4's batch and fan-outs
SLOTS = [(B, F2), (B * (F2 + 1), F1)]      # (M, k) of the two SAGE layers of a cfg4 batch


def one(vals):
    return [(v,) for v in vals]


def negatives(arity, ok=1):
    return [tuple(-1 if i == j else ok for i in range(arity)) for j in range(arity)]


COUNTS = [-1] + EDGE + [M1, M10, I31 - 1, I31]
NODES = [-1, 0, 1, 33, 64 * 32, 64 * 32 + 1, M1, M10, I31 - 1, I31]   # 32 ids per 4-byte word
CASES = {
    "gnn_hub_plan_workspace_bytes": one(COUNTS),
    "gnn_spmm_tasks_workspace_bytes": one(COUNTS),
    "gnn_column_order_workspace_bytes": one(COUNTS),
    "gnn_xcd_hub_plan_workspace_bytes": negatives(2) + [(0, 0), (1, 0), (1, 1), (32, 33), (33, 32),
                                                        (64, 65), (65, 64), (M1, E10), (M1, E20),
                                                        (M10, E100), (I31 - 1, 1), (I31, 1)],
    # (n_rows, nnz_local, n_own, world)
    "gnn_cover_workspace_bytes": negatives(4) + [(0, 0, 0, 1), (1, 0, 0, 1), (1, 1, 1, 1),
                                                 (1, 0, 0, 0), (1, 0, 0, 64), (1, 0, 0, 65),
                                                 (33, 32, 33, 1), (32, 33, 32, 1), (65, 64, 65, 2),
                                                 (64, 65, 32, 2)]
    + [(n, e // w, n // w, w) for n, e in ((M1, E10), (M1, E20), (M10, E100)) for w in (2, 8)]
    + [(I31 - 1, 1, 1, 2), (I31, 1, 1, 2)],
    "gnn_cover_send_workspace_bytes": one([-1] + EDGE + [E10 // 8, E100 // 8, E100 // 2]),
    # (n_edges, n_nodes)
    "gnn_gcn_adjacency_workspace_bytes": negatives(2) + [(0, 0), (0, 1), (1, 1), (16, 1), (16, 0),
                                                         (32, 33), (33, 32), (E10, M1), (E20, M1),
                                                         (E100, M10), (1, I31 - 1), (1, I31)],
    "gnn_frontier_workspace_bytes": one(NODES),
    "gnn_sample_layers_workspace_bytes": one(NODES),
    "gnn_sage_maps_transpose_workspace_bytes": negatives(2) + [(0, 0), (1, 0), (1, 1), (64, 0),
                                                               (65, 0), (8192, 25)] + SLOTS
    + [(I31 - 1, 0), (I31, 0), (I31, 1), (2 ** 30, 1)],
    "gnn_sage_maps_transpose_nbr_workspace_bytes": negatives(2) + [(0, 0), (1, 0), (1, 1), (64, 1),
                                                                   (65, 1), (8192, 25)] + SLOTS
    + [(I31 - 1, 1), (I31, 1), (2 ** 30, 2), (2 ** 30, 3)],
}
SCATTER = negatives(3, ok=4) + [(0, 0, 4), (1, 1, 4), (1, 0, 4), (1, 256, 4)] + \
    [(m, k, f) for m, k in SLOTS for f in (3, 4, 128, 256)] + [(I31, 1, 4), (I31 - 1, 0, 4)]
for name in ("concat", "concat_maxpool", "agg", "agg_maxpool"):
    CASES[f"gnn_sage_scatter_{name}_workspace_bytes"] = SCATTER
# (n, k, m, nnz_a, nnz_b)
CASES["gnn_relation_product_workspace_bytes"] = negatives(5) + [
    (0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (32, 1, 1, 0, 0), (33, 1, 1, 0, 0), (64, 1, 1, 0, 0),
    (65, 1, 1, 0, 0), (1, 1, 64 * 256, 0, 0), (1, 1, 64 * 256 + 1, 0, 0),
    (M1, M1, M1, 5 * M1, 5 * M1), (M10, M1, M10, E100, E100),
    (I31 - 1, 1, 1, 0, 0), (I31, 1, 1, 0, 0), (1, I31 - 1, 1, 0, 0), (1, I31, 1, 0, 0),
    (1, 1, I31 - 1, 0, 0), (1, 1, I31, 0, 0)]
# (n, b)
CASES["gnn_induced_subgraph_workspace_bytes"] = negatives(2) + [
    (0, 0), (1, 1), (64, 64), (65, 65), (32, 33), (33, 32), (M1, 32), (M1, 1024), (M1, 131072),
    (M1, 131073), (M10, M1), (I31 - 1, 1), (I31, 1), (1, I31 - 1), (1, I31)]


def main():
    parent, result = (ctypes.CDLL(p) for p in sys.argv[1:3])
    print(f"# {'query':48s} {'arguments':44s} {'parent':>14s} {'result':>14s}")
    differ = calls = 0
    for name, cases in CASES.items():
        for args in cases:
            got = []
            for lib in (parent, result):
                fn = getattr(lib, name)
                fn.restype = ctypes.c_int64
                fn.argtypes = [ctypes.c_int64] * len(args)
                if name == "gnn_cover_workspace_bytes":
                    fn.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int32]
                got.append(fn(*args))
            calls += 1
            differ += got[0] != got[1]
            mark = "equal" if got[0] == got[1] else "DIFFERENT"
            print(f"{name:50s} {str(args):44s} {got[0]:14d} {got[1]:14d}  {mark}")
    print(f"# {calls} calls, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
