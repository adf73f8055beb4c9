"""The ctypes binding is read from include/gnn_mi355x.h (``_lib.parse_header``), the wide entries
are called by parameter name (``_lib.invoke``) and the plans hand out their arguments under the
header's names. No GPU needed."""
import ctypes
import keyword
import random

import pytest
import torch

from graphneuralnetwork_amd import _lib
from graphneuralnetwork_amd.graph import RowSplitPlan, TaskPlan

INT, I32, I64 = ctypes.c_int, ctypes.c_int32, ctypes.c_int64
U32, U64, F32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
VP, CP = ctypes.c_void_p, ctypes.c_char_p

SEGMENTS = [(I64, "seg_len"), (VP, "seg_row"), (VP, "seg_begin"), (I64, "n_seg"),
            (VP, "long_row"), (VP, "long_seg_ptr"), (I64, "n_long")]

# written by hand from the header: name -> (restype, [(argtype, parameter name), ...])
PINNED = {
    "gnn_version": (INT, []),
    "gnn_error_string": (CP, [(INT, "code")]),
    "gnn_halo_rccl_path": (INT, [(CP, "buf"), (I64, "len")]),
    "gnn_py_layer_result_free": (None, [(VP, "result")]),
    "gnn_sup_head_workspace_bytes": (I64, [(I64, "n")]),
    "gnn_gcn_transform_epi_f32": (INT, [
        (VP, "x"), (I64, "ldx"), (I64, "n_rows"), (I64, "k"), (VP, "w"), (I64, "fout"),
        (VP, "bias"), (I32, "relu"), (F32, "drop_p"), (U64, "drop_seed"), (VP, "y"),
        (I64, "ldy"), (VP, "stream")]),
    "gnn_py_layer_sample": (INT, [
        (VP, "rowptr"), (VP, "nbr"), (I64, "n_nodes"), (VP, "nodes"), (I64, "n_batch"),
        (I32, "num_layers"), (I64, "num_neighs"), (I32, "is_gcn"), (VP, "mt_state"),
        (VP, "result")]),
    "gnn_spmm_csr_f32": (INT, [
        (VP, "rowptr"), (VP, "col"), (VP, "val"), (I64, "n_rows"), (VP, "x"), (I64, "ldx"),
        (I64, "feat"), (VP, "bias"), (VP, "y"), (I64, "ldy"), *SEGMENTS,
        (VP, "small_row"), (VP, "small_col"), (VP, "small_val"), (I64, "n_small"),
        (VP, "mid_row"), (I64, "n_mid"), (VP, "partial"), (U32, "flags"), (VP, "stream")]),
    "gnn_gat_csr_ex_f32": (INT, [
        (VP, "rowptr"), (VP, "col"), (I64, "n_rows"), (VP, "wh"), (I64, "ldw"), (I64, "heads"),
        (I64, "fh"), (VP, "el"), (VP, "er"), (I64, "lde"), (F32, "negative_slope"),
        (I32, "mode"), (VP, "empty_row_fill"), (F32, "dropout_p"), (U64, "dropout_seed"),
        (VP, "out"), (I64, "ldo"), *SEGMENTS,
        (VP, "small_row"), (VP, "small_col"), (I64, "n_small"), (VP, "mid_row"), (I64, "n_mid"),
        (VP, "short_row"), (I64, "n_short"), (VP, "partial"), (VP, "stats"), (U32, "flags"),
        (VP, "stream"), (VP, "whh"), (I64, "ldwh"), (VP, "erh"), (I64, "ldeh"), (VP, "a_dst")]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    res, params = PINNED[name]
    assert _lib.SIGNATURES[name] == (res, [t for t, _ in params])
    assert _lib.PARAMS[name] == tuple(n for _, n in params)


def test_pinned_widths():
    assert len(PINNED["gnn_spmm_csr_f32"][1]) == 26
    assert len(PINNED["gnn_gat_csr_ex_f32"][1]) == 40
    # every parameter name can be a Python keyword argument
    assert not [n for names in _lib.PARAMS.values() for n in names
                if keyword.iskeyword(n) or not n.isidentifier()]


# ---------------------------------------------------------------- the parser
def test_parser_refuses_unknown_type():
    with pytest.raises(ValueError, match=r"gnn_a.*size_t"):
        _lib.parse_header("int gnn_a(const float* x, size_t n);")
    with pytest.raises(ValueError, match=r"gnn_b.*double"):
        _lib.parse_header("double gnn_b(void);")
    with pytest.raises(ValueError, match="gnn_c"):  # void is a return type only
        _lib.parse_header("int gnn_c(void x);")
    with pytest.raises(ValueError, match="gnn_d"):  # a parameter without a name
        _lib.parse_header("int gnn_d(int64_t);")


def test_parser_reads_split_and_commented_prototypes():
    text = """
    #include <stdint.h>
    #define GNN_X(a) \\
        gnn_not_a_function(a);
    extern "C" {
    /* int gnn_in_a_comment(int a); */
    // int gnn_in_a_line_comment(int a);
    int64_t gnn_split(const int32_t* col,
                      int64_t nnz,   /* edges */
                      uint32_t
                          flags, // trailing
                      void** out);
    const char* gnn_text(char* buf, const char* name, float p, uint64_t seed);
    void gnn_nothing(void);
    int helper_fn(int a);
    static int other(size_t gnn_like);
    }
    """
    got = _lib.parse_header(text)
    assert got == {
        "gnn_split": (I64, [VP, I64, U32, VP], ("col", "nnz", "flags", "out")),
        "gnn_text": (CP, [CP, CP, F32, U64], ("buf", "name", "p", "seed")),
        "gnn_nothing": (None, [], ()),
    }


def test_parser_refuses_a_second_declaration():
    with pytest.raises(ValueError, match="gnn_a"):
        _lib.parse_header("int gnn_a(void); int gnn_a(int x);")


# ---------------------------------------------------------------- the binder
class _Stub:
    """Stands in for the loaded library: every entry records its positional arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_invoke_orders_keywords_as_the_header(monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(_lib, "_lib", stub)
    names = _lib.PARAMS["gnn_spmm_csr_tasks_bf16"]
    assert len(names) == 27 and "xh_f32" in names
    kw = {n: i for i, n in enumerate(names)}
    keys = list(kw)
    random.Random(0).shuffle(keys)
    assert keys != list(names)
    assert _lib.invoke("gnn_spmm_csr_tasks_bf16", **{k: kw[k] for k in keys}) == 0
    assert stub.calls == [("gnn_spmm_csr_tasks_bf16", tuple(range(len(names))))]
    _lib.run("gnn_version")
    assert stub.calls[-1] == ("gnn_version", ())


def test_invoke_refuses_missing_and_unknown_keywords(monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(_lib, "_lib", stub)
    kw = dict.fromkeys(_lib.PARAMS["gnn_spmm_csr_tasks_bf16"], 0)
    missing = {k: v for k, v in kw.items() if k != "xh_f32"}
    with pytest.raises(TypeError, match="xh_f32"):
        _lib.invoke("gnn_spmm_csr_tasks_bf16", **missing)
    with pytest.raises(TypeError, match="col_hub"):
        _lib.invoke("gnn_spmm_csr_tasks_bf16", col_hub=0, **kw)
    with pytest.raises(TypeError, match="col_hub"):  # one swapped for another: the count fits
        _lib.invoke("gnn_spmm_csr_tasks_bf16", col_hub=0, **missing)
    assert stub.calls == []


def test_invoke_follows_the_loaded_library(monkeypatch):
    first, second = _Stub(), _Stub()
    monkeypatch.setattr(_lib, "_lib", first)
    _lib.invoke("gnn_error_string", code=1)
    monkeypatch.setattr(_lib, "_lib", second)  # what use_variant does
    _lib.invoke("gnn_error_string", code=2)
    assert first.calls == [("gnn_error_string", (1,))]
    assert second.calls == [("gnn_error_string", (2,))]


# ---------------------------------------------------------------- the plans
def _block(entry, first, last):
    names = _lib.PARAMS[entry]
    return set(names[names.index(first):names.index(last) + 1])


def _plan(mid=(3, 5)):
    i32 = torch.int32
    return RowSplitPlan(
        seg_len=8, seg_row=torch.tensor([7, 7], dtype=i32),
        seg_begin=torch.tensor([20, 28], dtype=torch.int64),
        long_row=torch.tensor([7], dtype=i32), long_seg_ptr=torch.tensor([0, 2], dtype=i32),
        small_row=torch.tensor([0, 1, 2, 4], dtype=i32),
        small_col=torch.tensor([-1, 6, -1, 3], dtype=i32),
        small_val=torch.tensor([0.0, 0.5, 0.0, 2.0]), mid_row=torch.tensor(mid, dtype=i32))


def test_plan_fields_carry_the_header_names():
    p = _plan()
    seg = p.segments()
    assert set(seg) == _block("gnn_spmm_csr_f32", "seg_len", "n_long") == {n for _, n in SEGMENTS}
    assert (seg["seg_len"], seg["n_seg"], seg["n_long"]) == (8, 2, 1)
    assert seg["seg_row"] == p.seg_row.data_ptr() and seg["seg_begin"] == p.seg_begin.data_ptr()
    assert seg["long_row"] == p.long_row.data_ptr()
    assert seg["long_seg_ptr"] == p.long_seg_ptr.data_ptr()
    rows = p.spmm_rows()
    assert set(rows) == _block("gnn_spmm_csr_f32", "small_row", "n_mid")
    assert set(rows) == _block("gnn_spmm_csr_hub_bf16", "small_row", "n_mid")
    assert (rows["small_row"], rows["small_col"], rows["small_val"], rows["n_small"]) == (
        p.small_row.data_ptr(), p.small_col.data_ptr(), p.small_val.data_ptr(), 4)
    assert (rows["mid_row"], rows["n_mid"]) == (p.mid_row.data_ptr(), 2)
    mid, short = p.mid_row[:1], p.mid_row[1:]
    gat = p.gat_rows(mid, short)
    for entry in ("gnn_gat_csr_f32", "gnn_gat_csr_hub_f32", "gnn_gat_csr_ex_f32"):
        assert set(gat) == _block(entry, "small_row", "n_short")
    assert gat == dict(small_row=p.small_row.data_ptr(), small_col=p.small_col.data_ptr(),
                       n_small=4, mid_row=mid.data_ptr(), n_mid=1, short_row=short.data_ptr(),
                       n_short=1)
    assert p.gat_rows(mid, short[:0])["short_row"] is None
    tp = TaskPlan(8, p, torch.tensor([5], dtype=torch.int32),
                  torch.tensor([0, 5], dtype=torch.int32), 4, 128)
    assert tp.segments() == seg
    for entry in ("gnn_spmm_csr_tasks_f32", "gnn_spmm_csr_tasks_bf16", "gnn_gat_csr_tasks_f32"):
        assert set(tp.task_rows()) == _block(entry, "mid_row", "n_task")
    assert tp.task_rows() == dict(mid_row=tp.mid_row.data_ptr(), n_mid=1,
                                  task_row=tp.task_row.data_ptr(), n_task=1)
    # each wide entry's keywords are exactly what ops.py puts together from these blocks
    for entry, blocks in (("gnn_spmm_csr_f32", (seg, rows)), ("gnn_gat_csr_ex_f32", (seg, gat)),
                          ("gnn_spmm_csr_tasks_f32", (seg, tp.task_rows()))):
        for b in blocks:
            assert set(b) <= set(_lib.PARAMS[entry])


def test_empty_mid_class_passes_long_seg_ptr():
    """mid_row == NULL means "no plan" to the kernels: an empty class is never None."""
    p = _plan(mid=())
    lsp = p.long_seg_ptr.data_ptr()
    assert lsp not in (None, 0)
    rows = p.spmm_rows()
    assert (rows["mid_row"], rows["n_mid"]) == (lsp, 0)
    full = _plan()
    gat = full.gat_rows(full.mid_row[:0], full.mid_row)  # every mid row went to the short class
    assert (gat["mid_row"], gat["n_mid"], gat["n_short"]) == (full.long_seg_ptr.data_ptr(), 0, 2)
    tp = TaskPlan(8, p, p.mid_row, torch.tensor([0, 5], dtype=torch.int32), 4, 128)
    assert (tp.task_rows()["mid_row"], tp.task_rows()["n_mid"]) == (lsp, 0)
    empty = TaskPlan(8, p, p.mid_row, torch.zeros(0, dtype=torch.int32), 4, 128)
    assert (empty.task_rows()["task_row"], empty.task_rows()["n_task"]) == (None, 0)


def test_skip_empty_drops_exactly_the_edgeless_rows():
    p = _plan()
    rows = p.spmm_rows(skip_empty=True)
    small_row, small_col, small_val = p.nonempty_small()
    assert small_row.tolist() == [1, 4] and small_col.tolist() == [6, 3]
    assert small_val.tolist() == [0.5, 2.0]
    assert (rows["small_row"], rows["small_col"], rows["small_val"], rows["n_small"]) == (
        small_row.data_ptr(), small_col.data_ptr(), small_val.data_ptr(), 2)
    assert (rows["mid_row"], rows["n_mid"]) == (p.mid_row.data_ptr(), 2)
    assert p.spmm_rows()["n_small"] == 4  # the full class is still there
