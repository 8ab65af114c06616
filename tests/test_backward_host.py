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


# ------------------------------------------------------------------ what tests/test_gpu_backward_edges.py rests on
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scone_amd", "csrc")


def _edges():
    import test_gpu_backward_edges as GE  # (its case tables and list builders only: nothing here touches a GPU)
    return GE


def test_the_instance_matrix_reaches_all_18_instances():
    """NT as launch_chunks_nt picks it: pieces = d / E with E = 4 (fp32) or 8 (fp16, bf16); <= 64 -> 1, <= 128 -> 2, else 4."""
    src = open(os.path.join(CSRC, "scone_backward.hip")).read()
    assert "if (pieces <= 64)" in src and "else if (pieces <= 128)" in src and "static constexpr int E = DT == SCONE_DT_F32 ? 4 : 8;" in src
    reached = set()
    for dtype, d, reduce in _edges().INSTANCE_CASES:
        assert d % 8 == 0
        pieces = d // (4 if dtype == "fp32" else 8)
        nt = 1 if pieces <= 64 else 2 if pieces <= 128 else 4
        reached.add((dtype, nt, reduce))
        assert d == 16384 or pieces % (nt * 64) != 0, "the last column tile is not ragged"     # (16384: whole tiles, several of them)
    assert reached == {(t, nt, r) for t in ("fp32", "fp16", "bf16") for nt in (1, 2, 4) for r in ("mean", "sum")}
    assert any(d // 4 > 256 for t, d, _ in _edges().INSTANCE_CASES if t == "fp32"), "no fp32 case has several column tiles"
    assert any(d // 8 > 256 for t, d, _ in _edges().INSTANCE_CASES if t != "fp32"), "no half-precision case has several column tiles"


def test_the_grid_cap_and_the_block_size_are_what_the_grid_case_assumes():
    import re
    common = open(os.path.join(CSRC, "scone_common.h")).read()
    src = open(os.path.join(CSRC, "scone_backward.hip")).read()
    assert re.search(r"^#define SCONE_MAX_BLOCKS \(1u << 20\)$", common, flags=re.M)
    assert re.search(r"^constexpr int BWD_THREADS = 256;$", src, flags=re.M)
    assert "scone_capped_blocks(((unsigned long long)pl->m.n_chunks + 3) / 4)" in src          # 4 waves of 64 per block
    GE = _edges()
    assert GE.GRID_WAVES == (1 << 20) * (256 // 64) and GE.GRID_ROWS == GE.GRID_WAVES + 2048


def test_the_short_form_equals_the_row_loop():
    GE = _edges()
    rng = np.random.default_rng(8)
    n = 20000
    off, ids = GE.grid_lists(n, 700, rng)
    g = rng.standard_normal((n, 8)).astype(np.float16)
    assert (np.diff(off) == 2).sum() == 700
    for reduce in ("mean", "sum"):
        rid, rows = BW.backward_rows(off, ids, g, reduce, 128, 0, n, n)
        sid, short = BW.backward_rows_short(off, ids, g, reduce, 0, n, n)
        lens = BW.row_lengths(off, ids)[1]
        assert len(rid) == n and (lens == 2).sum() >= 600 and lens.max() == 2
        assert np.array_equal(rid, sid) and np.array_equal(rows.view(np.uint32), short.view(np.uint32))
    own = BW.backward_rows_short(off, ids, g, "mean", 100, 5000, n)
    ref = BW.backward_rows(off, ids, g, "mean", 128, 100, 5000, n)
    assert np.array_equal(own[0], ref[0]) and np.array_equal(own[1].view(np.uint32), ref[1].view(np.uint32))


def test_the_clamp_is_the_identity_on_well_formed_offsets_and_the_headers_rule_elsewhere():
    off, ids = VL._lists("small", 3)
    lo, hi = BW.clamp_offsets(off)
    assert np.array_equal(lo, off[:-1]) and np.array_equal(hi, off[1:])
    rows, pos, K = BW.references(off, ids)
    assert np.array_equal(rows, ids) and np.array_equal(K, np.diff(off))
    bent = np.asarray([0, 4, 2, -3, 9, 6, 6])                    # total = 6 of 8 ids
    lo, hi = BW.clamp_offsets(bent)
    assert lo.tolist() == [0, 4, 2, 0, 6, 6] and hi.tolist() == [4, 4, 2, 6, 6, 6]
    rows, pos, K = BW.references(bent, np.arange(10, 18))
    assert K.tolist() == [4, 0, 0, 6, 0, 0] and rows.tolist() == [10, 11, 12, 13] + [10, 11, 12, 13, 14, 15]
    assert pos.tolist() == [0] * 4 + [3] * 6


def test_the_wrong_models_are_wrong_where_they_should_be():
    C_ = 4
    off = np.arange(7)                                                     # six positions, one id each
    ids = np.asarray([0, 0, 1, 2, 2, 2])
    g = np.zeros((6, 2), dtype=np.float32)
    g[0:3] = -0.0                                                          # rows 0 and 1: only -0
    g[3:6, 0] = np.float32(2.0 ** -149)                                   # row 2: three denormals; column 1 stays +0
    want = BW.backward_rows(off, ids, g, "sum", C_)[1]
    assert want.view(np.uint32).tolist() == [[0, 0], [0, 0], [3, 0]]
    start = BW.backward_rows(off, ids, g, "sum", C_, neg_zero_start=True)[1]
    assert start.view(np.uint32).tolist() == [[0x80000000] * 2, [0x80000000] * 2, [3, 0]]
    ftz = BW.backward_rows(off, ids, g, "sum", C_, flush_denormals=True)[1]
    assert ftz.view(np.uint32).tolist() == [[0, 0], [0, 0], [0, 0]]
    tiny = np.full((6, 2), 1.5 * 2.0 ** -126, dtype=np.float32)            # normal; a third of it is not
    mean = BW.backward_rows(np.asarray([0, 3]), np.asarray([0, 1, 2]), tiny[:1], "mean", C_)[1]
    assert (mean != 0).all() and (np.abs(mean) < np.finfo(np.float32).tiny).all()
    assert (BW.backward_rows(np.asarray([0, 3]), np.asarray([0, 1, 2]), tiny[:1], "mean", C_, flush_denormals=True)[1] == 0).all()
    assert np.array_equal(BW.flush(np.asarray([-2.0 ** -130, 2.0 ** -126, 0.0], dtype=np.float32)).view(np.uint32),
                          np.asarray([-0.0, 2.0 ** -126, 0.0], dtype=np.float32).view(np.uint32))
