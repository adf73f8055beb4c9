"""``probe_rows`` of tests/test_wide_addressing_gpu.py, on the CPU: for every operand layout the
GPU module uses, the probes straddle B1 = 2^31 bytes, B2 = 2^32 bytes and B3 = 2^31 elements,
and every row a wrapped index would reach instead of a probe holds other content than the probe
(zeros, or another probe's row). So a kernel that wraps fails the GPU tests."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "test_wide_addressing_gpu", Path(__file__).with_name("test_wide_addressing_gpu.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

LAYOUTS = sorted(W.LAYOUTS.items())
# out_rows of a bf16 result: rows of 128 two-byte elements
LAYOUTS.append(("bf16 transform result", (W.N32, 128, 2)))


@pytest.mark.parametrize("name,layout", LAYOUTS, ids=[n for n, _ in LAYOUTS])
def test_probes_straddle_every_threshold(name, layout):
    n, ld, es = layout
    rows = W.probe_rows(n, ld, es)
    assert rows.dtype == np.int64 and np.array_equal(rows, np.unique(rows))
    assert {0, 1, n - 2, n - 1} <= set(rows.tolist())
    byte_of = rows * ld * es          # the first byte of a row
    elem_of = rows * ld               # its first element
    last_byte = byte_of + ld * es - 1
    for rb, first, last, limit in zip(W.threshold_rows(ld, es), (byte_of, byte_of, elem_of),
                                      (last_byte, last_byte, elem_of + ld - 1),
                                      (W.B1_BYTES, W.B2_BYTES, W.B3_ELEMS)):
        assert {rb - 1, rb, rb + 1} <= set(rows.tolist())
        i = int(np.searchsorted(rows, rb))
        assert last[i - 1] < limit <= first[i]  # rB - 1 ends below it, rB starts at or past it
    # the smallest operand: 64 rows past the last threshold
    assert n == max(W.threshold_rows(ld, es)) + W.SPARE


@pytest.mark.parametrize("name,layout", LAYOUTS, ids=[n for n, _ in LAYOUTS])
def test_a_wrapped_address_reads_other_content(name, layout):
    n, ld, es = layout
    rows = W.probe_rows(n, ld, es)
    for width in (ld, 8):
        vals = W.probe_values(rows.size, width)
        assert np.array_equal(vals, vals.astype(np.float32))
        assert (np.abs(vals * 4 - np.round(vals * 4)) == 0).all() and np.abs(vals).max() < 32
        content = {int(r): vals[i] for i, r in enumerate(rows)}
        zero = np.zeros(width, np.float32)
        seen = 0
        for r in rows.tolist():
            assert (content[r] != 0).any()  # a probe differs from the zero rows around it
            for a in W.aliases(r, ld, es):
                assert 0 <= a < r
                other = content.get(a, zero)
                assert not np.array_equal(other, content[r]), (name, r, a)
                assert (other != content[r]).all() or a not in content
                seen += 1
        assert seen >= 9  # 3 probes past each threshold, at least one alias each


def test_the_row_at_b2_aliases_row_0():
    for n, ld, es in W.LAYOUTS.values():
        _, rb2, _ = W.threshold_rows(ld, es)
        assert 0 in W.aliases(rb2, ld, es) and 1 in W.aliases(rb2 + 1, ld, es)
