"""CPU: the preconditions of tests/test_gpu_dense_backward.py (include/scone_hip.h, "backward of the dense side"), checked on the
host with C = 128, and the bindings of the section.

An index plan is the backward plan of one-element lists, so its expectation is tests/backward_fixture.py's `backward_rows` with
`off = arange(ntok + 1)`.  The GPU tests compare bits with it; that only says something if the batches they use can tell the
contract's summation order from the obvious wrong ones.  Here: with fp32 standard-normal `grad_out` at d = 64, a model that walks
a row's references backwards and a model that sums a row in one chain (no chunks) both give other bits than the contract -- on
the token rows of the packed batch "small" of tests/test_gpu_varlen.py (867 / 903 / 988 / 203 references: every row has several
chunks) and on the position rows of the rectangle B = 2C + 5, T = 3 with default positions (three chunks each).

The precondition uses fp32 gradients.  fp16 gradients summed with weight 1 have few significant bits, so many partial sums are
exact and the order shows less: in the probe made when this file was written the walk order still showed on the long token
rows, but not on the short position rows.  The GPU tests run all three gradient types against the fixture anyway; the fp32
cases are the ones that pin the order.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches)

CHUNK = 128
D = 64


def index_rows(idx, g, n_ids, skip=None, reduce="sum", C_=CHUNK, **wrong):
    """The contract of an index plan + scone_backward_rows, through the fixture only: positions with an id outside [0, n_ids) or
    with skip != 0 have no reference.  Returns (ids [U] int64 ascending, rows [U, d] fp32, K [ntok])."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    keep = (idx >= 0) & (idx < n_ids)
    if skip is not None:
        keep &= np.asarray(skip).reshape(-1) == 0
    off = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(keep, out=off[1:])
    ids, rows = BW.backward_rows(off, idx[keep], g, reduce, C_, n_rows=n_ids, **wrong)
    return ids, rows, keep.astype(np.int32)


def _g(ntok, seed):
    return np.random.default_rng(seed).standard_normal((ntok, D)).astype(np.float32)


def test_small_batch_token_rows():
    tok, cu, _ = VL._batch("small")
    assert len(tok) == 2961 and int(cu[-1]) == 2961
    assert np.bincount(tok, minlength=VL.VOCAB + 1).tolist() == [867, 903, 988, 203]
    lens = np.diff(cu)
    assert lens[0] == 0 and lens[-1] == 0 and ((lens[:-1] == 0) & (lens[1:] == 0)).any()     # empty: front, a run, the end


@pytest.mark.parametrize("space", ["small_tokens", "rectangle_positions"])
def test_the_batches_tell_the_summation_order(space):
    if space == "small_tokens":
        idx, n_ids = VL._batch("small")[0], VL.VOCAB + 1
    else:
        B, T = 2 * CHUNK + 5, 3
        idx, n_ids = np.arange(B * T) % T, T
    g = _g(len(idx), 5)
    ids, want, K = index_rows(idx, g, n_ids)
    assert np.array_equal(ids, np.arange(n_ids)) and K.all()
    assert (np.bincount(idx) > CHUNK).all()                          # every row has several chunks
    for wrong in (dict(reverse=True), dict(chunked=False)):
        _, other, _ = index_rows(idx, g, n_ids, **wrong)
        assert not E.same_bits(other, want), f"{wrong} gives the contract's bits: the batch pins nothing"
    _, mean, _ = index_rows(idx, g, n_ids, reduce="mean")
    assert E.same_bits(mean, want)                                   # K_p = 1: the weight is 1.0f


def test_skip_and_range_rules_of_the_fixture():
    idx = np.array([2, -1, 0, 5, 2, 4, 2, 0])
    g = _g(len(idx), 6)
    skip = np.array([0, 0, 1, 0, 0, 0, 1, 0])
    ids, rows, K = index_rows(idx, g, 5, skip)
    assert ids.tolist() == [0, 2, 4] and K.tolist() == [1, 0, 0, 0, 1, 1, 0, 1]
    assert E.same_bits(rows[1], (np.float32(0) + g[0]) + g[4]) and E.same_bits(rows[0], np.float32(0) + g[7])


def test_bindings_and_scratch_sizes():
    from scone_amd import _lib
    for name in ("scone_backward_plan_index", "scone_backward_default_positions", "scone_backward_wpe_scratch", "scone_backward_wpe"):
        assert name in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.scone_backward_chunk() == CHUNK
    assert _lib.backward_wpe_scratch(CHUNK, 5, 64) == 0              # one chunk per row: no partials
    assert _lib.backward_wpe_scratch(CHUNK + 1, 2, 64) == 2 * 2 * 64 * 4
    assert _lib.backward_wpe_scratch(2 * CHUNK + 5, 3, 776) == 3 * 3 * 776 * 4
    assert _lib.backward_wpe_scratch(0, 0, 64) == 0
    out = C.c_uint64(7)
    assert lib.scone_backward_wpe_scratch(-1, 2, 64, C.byref(out)) == _lib.EINVAL
    assert lib.scone_backward_wpe_scratch(1, 2, 64, None) == _lib.EINVAL
    # a null handle is refused before anything else, without a device
    assert lib.scone_backward_plan_index(None, None, 0, 4, None, None, None, None, None) == _lib.EINVAL
    assert lib.scone_backward_default_positions(None, None, 0, 1, 0, None, None) == _lib.EINVAL
    assert lib.scone_backward_wpe(None, None, 0, 0, 0, 1, None, None, None) == _lib.EINVAL
