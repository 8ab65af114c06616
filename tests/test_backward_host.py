"""The lookup's backward without a GPU: the chunk constant, the refusals that need no device, and the numpy statement of the
contract (tests/backward_fixture.py) against a float64 evaluation.

The bound of the last test is derived, not measured: every contribution c = g * w carries at most two roundings (the
reciprocal w and the product), a row of len references is summed with len - 1 + (chunks - 1) < len additions whatever the
chunking, so |fixture - exact| <= (len + 2) * 2^-24 * sum|c| per element to first order (standard normal data: no underflow).
"""

import ctypes as C
import os
import sys

import numpy as np

from scone_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches and their per-sequence id lists)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: N_ROWS)


def test_chunk_is_a_power_of_two_in_range():
    c = _lib.lib().scone_backward_chunk()
    assert 64 <= c <= 512 and c & (c - 1) == 0
    from scone_amd.hip_backend import backward_chunk
    assert backward_chunk() == c


def test_null_refusals_need_no_device():
    lib = _lib.lib()
    plan, n_rows, n_refs = C.c_void_p(), C.c_uint64(7), C.c_uint64(7)
    assert lib.scone_backward_plan(None, None, 1, 1, C.byref(plan), C.byref(n_rows), C.byref(n_refs), None) == _lib.EINVAL
    assert lib.scone_backward_plan_varlen(None, None, None, 1, 1, C.byref(plan), C.byref(n_rows), C.byref(n_refs), None) == _lib.EINVAL
    assert lib.scone_backward_plan_csr(None, None, None, 1, C.byref(plan), C.byref(n_rows), C.byref(n_refs), None) == _lib.EINVAL
    assert lib.scone_backward_rows(None, None, None, _lib.DT_F32, _lib.REDUCE_MEAN, None, None, 0, None) == _lib.EINVAL
    assert lib.scone_backward_counts(None, None, None, None) == _lib.EINVAL
    assert plan.value is None and n_rows.value == 7 and n_refs.value == 7       # nothing was written


def test_destroying_a_null_plan_is_a_no_op():
    _lib.lib().scone_backward_plan_destroy(None)


def test_fixture_agrees_with_float64_within_the_derived_bound():
    C_ = _lib.lib().scone_backward_chunk()
    for max_n in (3, 4):
        off, ids = VL._lists("small", max_n)
        ntok = len(off) - 1
        g = np.random.default_rng(5 + max_n).standard_normal((ntok, 24)).astype(np.float16)
        for reduce in ("mean", "sum"):
            rid, rows = BW.backward_rows(off, ids, g, reduce, C_)
            rid64, sums, mags, lens = BW.backward_rows_f64(off, ids, g, reduce)
            assert np.array_equal(rid, rid64) and (np.diff(rid) > 0).all() and len(rid) < WS.N_ROWS[max_n]
            assert lens.max() > C_, "no row has more than one chunk"
            bound = (lens[:, None] + 2) * 2.0 ** -24 * mags
            err = np.abs(rows.astype(np.float64) - sums)
            assert (err <= bound).all(), (max_n, reduce, float((err / np.maximum(bound, 1e-300)).max()))
            assert rows.dtype == np.float32 and err.max() > 0          # the bound is not vacuous: fp32 sums do round
