"""CPU: the bindings of the gradient-norm entry points (include/scone_hip.h, "gradient norm, clipping and skipped steps"), and
tests/grad_norm_fixture.py checked against itself.

The GPU test compares `scone_grad_sqnorm` with the fixture bit for bit.  That proves the ORDER of the sums only if the order
shows in the fixture's result for the values used there, so this file asserts that the fixture's total of that value mix differs
from three other ways of adding the same squares: numpy's pairwise `np.sum`, a plain sequential sum, and an fp32 accumulation.
"""

import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_norm_fixture as GN  # noqa: E402

from scone_amd import _lib  # noqa: E402

NEW = ("scone_grad_sqnorm_scratch", "scone_grad_sqnorm", "scone_grad_ctl_set", "scone_opt_step_ctl", "scone_opt_step_lean_ctl")


def test_signatures_and_exports():
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.scone_abi_version() == 2
    # the _ctl steps: the plain signature with one pointer before the stream
    for plain, ctl in (("scone_opt_step", "scone_opt_step_ctl"), ("scone_opt_step_lean", "scone_opt_step_lean_ctl")):
        a, b = _lib.SIGNATURES[plain], _lib.SIGNATURES[ctl]
        assert a[0] is b[0] and b[1] == a[1][:-1] + [C.c_void_p, a[1][-1]]


def test_ctl_struct_layout():
    S = _lib.SconeGradCtl
    assert C.sizeof(S) == 24
    assert (S.sqnorm.offset, S.norm.offset, S.coef.offset, S.skip.offset, S.reserved.offset) == (0, 8, 12, 16, 20)
    assert (S.sqnorm.size, S.norm.size, S.coef.size, S.skip.size, S.reserved.size) == (8, 4, 4, 4, 4)


def test_scratch_size():
    lib = _lib.lib()
    for n, want in ((0, 0), (1, 2), (1024, 1025), (1025, 1027), (2500, 2503), (1 << 40, (1 << 40) + (1 << 30))):
        out = C.c_uint64(123)
        assert lib.scone_grad_sqnorm_scratch(n, C.byref(out)) == _lib.OK
        assert out.value == want == GN.scratch_doubles(n), n
        assert _lib.grad_sqnorm_scratch(n) == want
    assert lib.scone_grad_sqnorm_scratch(5, None) == _lib.EINVAL


def test_null_handle_is_refused_without_gpu_work():
    lib = _lib.lib()
    assert lib.scone_grad_sqnorm(None, None, 0, None, None, None) == _lib.EINVAL
    assert lib.scone_grad_ctl_set(None, None, 1, 1.0, 1.0, 0, None, None) == _lib.EINVAL
    assert lib.scone_opt_step_ctl(None, None, None, None, 0, None, None, None, None, None) == _lib.EINVAL
    assert lib.scone_opt_step_lean_ctl(None, None, None, None, 0, None, None, None, None) == _lib.EINVAL


# ------------------------------------------------------------------ the fixture against itself
def test_fixture_on_values_whose_sums_are_exact():
    # small integers: every order gives the same exact sum, so the bookkeeping (lanes, tiles, ranges) is what is checked
    rng = np.random.default_rng(1)
    for n, d in ((0, 8), (1, 8), (5, 260), (1024, 8), (1025, 12), (2500, 4)):
        g = rng.integers(-7, 8, size=(n, d)).astype(np.float32)
        total, q, p = GN.sqnorm(g)
        exact = (g.astype(np.int64) ** 2)
        assert np.array_equal(q, exact.sum(axis=1).astype(np.float64))
        assert len(p) == (n + 1023) // 1024
        assert np.array_equal(p, [exact[1024 * k:1024 * k + 1024].sum() for k in range(len(p))])
        assert total == exact.sum() and not np.signbit(total)


def test_fixture_lane_order_shows_in_a_row():
    tiny = np.float32(2.0 ** -27)                                  # tiny^2 = 2^-54, a quarter of an ulp of 1
    # elements 0 .. 3 are all lane 0, added in turn: ((1 + 2^-54) + 2^-54) + 2^-54 = 1; the three added first would give 1 + 2^-52
    g = np.zeros((1, 8), dtype=np.float32)
    g[0, :4] = (1.0, tiny, tiny, tiny)
    assert GN.row_sq(g)[0] == 1.0
    # lane 0 holds 1, lanes 1, 2, 3 hold 2^-53 each (two elements).  Stage s = 2: lane 0 = 1 + 2^-53 = 1 (a tie, to even), lane 1 =
    # 2^-53 + 2^-53; stage s = 1: 1 + 2^-52.  One at a time, in any order, all three would be lost.
    g = np.zeros((1, 16), dtype=np.float32)
    g[0, 0] = 1.0
    for lane in (1, 2, 3):
        g[0, 4 * lane:4 * lane + 2] = tiny
    assert GN.row_sq(g)[0] == 1.0 + 2.0 ** -52


def test_fixture_special_values():
    d = 8
    assert GN.sqnorm(np.full((3, d), -0.0, dtype=np.float32))[0] == 0.0 and not np.signbit(GN.sqnorm(np.full((3, d), -0.0, np.float32))[0])
    sub = np.full((2, d), 2.0 ** -149, dtype=np.float32)
    assert GN.sqnorm(sub)[0] == 16 * 2.0 ** -298 > 0
    big = np.full((2, d), 3e38, dtype=np.float32)
    assert np.isfinite(GN.sqnorm(big)[0]) and GN.sqnorm(big)[0] > 1e77
    for bad in ((np.nan,), (np.inf,), (np.inf, -np.inf)):
        g = np.ones((3, d), dtype=np.float32)
        g[1, :len(bad)] = bad
        assert not np.isfinite(GN.sqnorm(g)[0])


def test_fixture_total_differs_from_other_orders():
    g = GN.value_mix(2500, 768)                                  # the mix and the largest shape of the GPU test
    a = np.abs(g[np.isfinite(g) & (g != 0)])
    assert a.min() < 2.0 ** -126 and a.max() == np.float32(3e38) and (g < 0).any() and (g > 0).any()
    assert ((a >= 2.0 ** -70) & (a < 2.0 ** -69)).any() and ((a >= 2.0 ** 60) & (a < 2.0 ** 61)).any()
    total, q, p = GN.sqnorm(g)
    assert np.isfinite(total)
    sq = g.astype(np.float64) ** 2
    pairwise = np.sum(sq)
    sequential = np.cumsum(sq.reshape(-1))[-1]                     # np.cumsum adds one element at a time, in order
    with np.errstate(over="ignore"):
        fp32 = np.cumsum(g.reshape(-1) * g.reshape(-1), dtype=np.float32)[-1]
    assert total != pairwise and total != sequential and np.float64(fp32) != total
    assert abs(total - pairwise) <= 1e-9 * pairwise                # ... and still the same number
    # rows too: some row sum differs from numpy's sum of that row
    assert (q != sq.sum(axis=1)).any()


def test_fixture_ctl():
    c = GN.ctl([9.0, 16.0], 1.0, 2.5)
    assert c["sqnorm"] == 25.0 and c["norm"] == np.float32(5.0) and c["coef"] == np.float32(2.5 / (5.0 + 1e-6)) and c["skip"] == 0
    assert GN.ctl([25.0], 1.0, 5.0)["coef"] == np.float32(5.0 / (5.0 + 1e-6)) < 1           # equal to the norm: still clipped
    assert GN.ctl([25.0], 1.0, 6.0)["coef"] == np.float32(1.0)
    assert GN.ctl([25.0])["coef"] == np.float32(1.0)
    assert GN.ctl([25.0 * 1024 * 1024], 1.0 / 1024, 1.0)["norm"] == np.float32(5.0)
    for skip in (False, True):
        c = GN.ctl([1.0, np.nan], 1.0, 1.0, skip)
        assert np.isnan(c["sqnorm"]) and c["coef"] == np.float32(1.0) and c["skip"] == int(skip)
    assert GN.ctl([np.inf], 1.0, 1.0, True)["skip"] == 1 and GN.ctl([np.inf], 1.0, 1.0, True)["coef"] == np.float32(0.0)
    assert GN.ctl([1.0, 2.0 ** -53, 2.0 ** -53])["sqnorm"] == 1.0 and GN.ctl([2.0 ** -53, 2.0 ** -53, 1.0])["sqnorm"] == 1.0 + 2.0 ** -52
