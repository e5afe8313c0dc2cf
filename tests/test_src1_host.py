"""CPU-only: the numpy statement of the single-source walk's out-list (tests/src1_ref.py) on the walk's test graph - each head's edges
ordered by (tail, position in the CSR-by-tail) - and the checker the GPU test applies to the library's exported arrays
(tests/test_layer_src1_gpu.py::test_out_list_order_host_and_device_build: the export copies device arrays, so that half needs the GPU)."""
import numpy as np
import pytest

from tests import src1_ref as sr


def test_numpy_out_list_is_ordered_by_tail_then_csr_position():
    trip = sr.make_triples()
    assert 2800 <= len(trip) <= 3200
    out_ptr, rt, pos, in_ptr, in_hr = sr.out_by_tail(trip)
    sr.check_out_by_tail(out_ptr, rt, pos, in_ptr, in_hr)
    # the graph's special entities
    assert out_ptr[sr.HUB + 1] - out_ptr[sr.HUB] > 256 and in_ptr[sr.HUB + 1] - in_ptr[sr.HUB] > 128
    assert out_ptr[sr.ISOLATED + 1] - out_ptr[sr.ISOLATED] == 1
    row = slice(out_ptr[sr.MULTI_HEAD], out_ptr[sr.MULTI_HEAD + 1])
    run = rt[row][rt[row][:, 1] == sr.MULTI_TAIL]
    assert run[:, 0].tolist() == [2, 0, 1]            # fact order (the CSR-by-tail's), not relation order
    span = pos[out_ptr[sr.SPAN_HEAD]:out_ptr[sr.SPAN_HEAD + 1]][rt[out_ptr[sr.SPAN_HEAD]:out_ptr[sr.SPAN_HEAD + 1], 1] == sr.HUB]
    assert len(span) >= 3 and len(set((span - in_ptr[sr.HUB]) // 128)) >= 2      # one run, several segments of the hub's row
    sub, rel = sr.subjects()
    assert len(sub) == 33 and sub[4] == sub[5] and rel[4] != rel[5]


def test_checker_rejects_a_run_in_relation_order():
    trip = sr.make_triples()
    out_ptr, rt, pos, in_ptr, in_hr = sr.out_by_tail(trip)
    lo = out_ptr[sr.MULTI_HEAD] + int(np.flatnonzero(rt[out_ptr[sr.MULTI_HEAD]:out_ptr[sr.MULTI_HEAD + 1], 1] == sr.MULTI_TAIL)[0])
    order = np.argsort(rt[lo:lo + 3, 0])              # the run sorted by relation instead
    rt2, pos2 = rt.copy(), pos.copy()
    rt2[lo:lo + 3], pos2[lo:lo + 3] = rt[lo:lo + 3][order], pos[lo:lo + 3][order]
    with pytest.raises(AssertionError):
        sr.check_out_by_tail(out_ptr, rt2, pos2, in_ptr, in_hr)
