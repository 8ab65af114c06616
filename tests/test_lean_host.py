"""CPU: the host half of the lean optimizer step (include/scone_hip.h, "lean optimizer step") and the properties of its numpy
statement, tests/lean_fixture.py.

1. `scone_lean_scalars_of` equals the fixture's scalars (double, rounded to fp32 once; no `pow` behind any: exact); what it
   refuses, without a GPU.
2. `scone_lean_rand16` equals the fixture's `rand16` on 10^4 tuples, with seeds, steps and rows at or above 2^32 and step 0.
3. Stochastic rounding is unbiased: of 65,536 values 1.0 + 0.25 ulp_bf16 the share rounded up is within 5 sigma of 0.25
   (sigma = sqrt(0.25 * 0.75 / 65536) = 0.0017).  A value bf16 holds exactly never changes; inf / NaN round as nearest does.
4. Drift: 4,096 elements at w = 1.0, 256 SGD steps of alpha * g = 2^-12 (1 / 32 of the bf16 ulp 2^-7 at 1.0, 1 / 16 of the ulp
   2^-8 just below it).  Under nearest rounding every element stays exactly 1.0.  Under stochastic rounding the mean of 1 - w
   is within 6 * 2^-11 of the true 256 * 2^-12 = 2^-4: the variance of one step is at most ulp^2 / 4 = 2^-16 / 4 = 2^-18, so
   256 independent steps give a standard deviation of at most sqrt(256 * 2^-18) = 2^-5 per element and 2^-5 / sqrt(4096) = 2^-11
   for the mean of 4,096 elements.
5. The fixture against `step_f64`: within 4 fp32 ulp of |w| + |update| (at most four roundings touch the magnitude of the
   weight or the update; the row sum's error enters through den, relatively, and is covered by the update's term).
6. The row sum's order: `row_sum_sq` equals a scalar loop that follows the contract word for word.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import lean_fixture as LF  # noqa: E402
import opt_fixture as OF  # noqa: E402

from scone_amd import _lib  # noqa: E402
from scone_amd.hip_backend import lean_rand16, lean_scalars  # noqa: E402

KINDS = ("sgd", "rowwise_adagrad")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hp", [dict(lr=3e-3, eps=1e-10, weight_decay=0.01, grad_scale=0.5), dict(lr=0.05),
                                dict(lr=1e-30, eps=1e-38, weight_decay=1e-12, grad_scale=1.0 / 3.0)])
def test_scalars_equal_the_double_definition(kind, hp):
    got, want = lean_scalars(kind, **hp), LF.scalars_f32(kind, **hp)
    assert sorted(got) == sorted(OF.NAMES)
    for name in OF.NAMES:
        assert isinstance(got[name], np.float32)
        assert got[name].view(np.uint32) == want[name].view(np.uint32), f"{name}: {got[name]!r} vs {want[name]!r}"
    assert got["alpha"] == np.float32(hp["lr"]) and all(got[k] == 0 for k in ("b1", "b2", "c1", "c2"))


def test_scalars_refusals_need_no_gpu():
    lib = _lib.lib()
    out = _lib.OptScalars()

    def call(**kw):
        hp = dict(struct_size=C.sizeof(_lib.LeanCfg), kind=_lib.LEAN_ROWWISE_ADAGRAD, rounding=_lib.ROUND_NEAREST, reserved=0,
                  lr=1e-3, eps=1e-10, weight_decay=0.0, grad_scale=1.0, seed=0, step=1)
        hp.update(kw)
        return lib.scone_lean_scalars_of(C.byref(_lib.LeanCfg(**hp)), C.byref(out))

    assert C.sizeof(_lib.LeanCfg) == 64 and _lib.LeanCfg.lr.offset == 16 and _lib.LeanCfg.seed.offset == 48
    assert call() == _lib.OK
    assert call(rounding=_lib.ROUND_STOCHASTIC, seed=2 ** 64 - 1, step=0) == _lib.OK and call(step=-7) == _lib.OK
    assert lib.scone_lean_scalars_of(None, C.byref(out)) == _lib.EINVAL
    assert lib.scone_lean_scalars_of(C.byref(_lib.LeanCfg(64, 0, 0, 0, 1e-3, 1e-10, 0.0, 1.0, 0, 1)), None) == _lib.EINVAL
    assert call(struct_size=8) == _lib.EINVAL and call(struct_size=72) == _lib.EINVAL
    assert call(kind=2) == _lib.EINVAL and call(kind=-1) == _lib.EINVAL
    assert call(rounding=2) == _lib.EINVAL and call(rounding=-1) == _lib.EINVAL
    assert call(reserved=1) == _lib.EINVAL
    for name in ("lr", "eps", "weight_decay", "grad_scale"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(**{name: bad}) == _lib.EINVAL, (name, bad)
    assert lib.scone_opt_step_lean(None, None, None, None, 0, None, None, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        lean_scalars("adam", 1e-3)
    with pytest.raises(ValueError):
        lean_scalars("sgd", float("nan"))


def test_rand16_equals_the_fixture():
    rng = np.random.default_rng(5)
    n = 10_000
    big = lambda: rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)             # noqa: E731
    seed, row = big(), big()
    step = rng.integers(-2 ** 63, 2 ** 63, size=n, dtype=np.int64)
    col = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    # small values, values at and above 2^32, step = 0, the extremes
    seed[:8] = [0, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 64 - 1, 7, 7, 7]
    step[:8] = [0, 0, 1, 2 ** 32, 2 ** 63 - 1, 0, 1, 2 ** 32 + 5]
    row[:8] = [0, 2 ** 32, 2 ** 32 - 1, 5, 2 ** 64 - 1, 0, 0, 10 ** 11]
    col[:8] = [0, 0, 1, 1023, 2 ** 32 - 1, 0, 0, 8191]
    seed[8:2000] &= np.uint64(0xFFFF)
    row[8:4000] %= np.uint64(10 ** 8)
    step[8:4000] = np.abs(step[8:4000]) % 10 ** 6
    col[8:6000] %= np.uint64(8192)
    want = LF.rand16(seed, step, row, col)
    got = np.asarray([lean_rand16(int(a), int(b), int(c), int(e)) for a, b, c, e in zip(seed, step, row, col)], dtype=np.uint32)
    assert (want < 65536).all() and np.array_equal(got, want)
    assert (row >= 2 ** 32).sum() > 1000 and (seed >= 2 ** 32).sum() > 1000 and (np.abs(step) >= 2 ** 32).sum() > 1000
    # every key matters: changing one argument alone changes the bits of most draws
    base = LF.rand16(3, 4, np.arange(4096), 9)
    for other in (LF.rand16(4, 4, np.arange(4096), 9), LF.rand16(3, 5, np.arange(4096), 9), LF.rand16(3, 4, np.arange(4096), 10),
                  LF.rand16(3, 4, np.arange(4096) + 2 ** 32, 9), LF.rand16(3 + 2 ** 32, 4, np.arange(4096), 9),
                  LF.rand16(3, 4 + 2 ** 32, np.arange(4096), 9)):
        assert (other != base).mean() > 0.99
    assert abs(base.mean() / 65536 - 0.5) < 5 * np.sqrt(1 / 12 / 4096)


def test_stochastic_rounding_is_unbiased_and_keeps_exact_values():
    n = 65536
    x = np.full((1, n), np.float32(1.0) + np.float32(0.25 * 2.0 ** -7), dtype=np.float32)
    assert x[0, 0] != 1 and BF.to_bf16_bits(x)[0, 0] == 0x3F80
    bits = LF.store_bf16(x, "stochastic", seed=11, step=3, row_ids=[123456789])
    assert set(np.unique(bits)) == {0x3F80, 0x3F81}
    up = float((bits == 0x3F81).mean())
    sigma = np.sqrt(0.25 * 0.75 / n)
    print(f"share rounded up {up:.4f} (0.25 +- {5 * sigma:.4f})")
    assert abs(up - 0.25) <= 5 * sigma
    neg = LF.store_bf16(-x, "stochastic", seed=11, step=3, row_ids=[123456789])
    assert np.array_equal(neg, bits | 0x8000), "the two signs do not round alike (away from zero, by the same bits)"
    # values bf16 holds exactly never change; inf / NaN as nearest; the largest finite value carries to infinity
    exact = BF.from_bf16_bits(np.arange(65536, dtype=np.uint16)).reshape(1, -1)
    r = np.full(exact.shape, 65535, dtype=np.uint32)
    kept = LF.round_bf16_stochastic(exact, r)
    assert BF.same_bf16_bits(kept, np.arange(65536, dtype=np.uint16).reshape(1, -1))
    assert np.array_equal(kept[~BF.is_nan_bits(kept)], np.arange(65536, dtype=np.uint16).reshape(1, -1)[~BF.is_nan_bits(kept)])
    top = np.asarray([[np.float32(3.4e38), -np.float32(3.4e38)]], dtype=np.float32)
    assert LF.round_bf16_stochastic(top, 65535).tolist() == [[0x7F80, 0xFF80]] and LF.round_bf16_stochastic(top, 0).tolist() == [[0x7F7F, 0xFF7F]]
    nan = np.asarray([[0x7F800001, 0x7FFFFFFF, 0xFF800001]], dtype=np.uint32).view(np.float32)
    assert BF.is_nan_bits(LF.round_bf16_stochastic(nan, 65535)).all(), "a NaN was carried into another class"


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_drift_of_small_steps(seed):
    n, steps = 4096, 256
    sc = LF.scalars_f32("sgd", lr=2.0 ** -12)
    g = np.ones((1, n), dtype=np.float32)
    ids = np.asarray([5], dtype=np.int64)
    near = sto = BF.to_bf16_bits(np.ones((1, n), dtype=np.float32))
    for t in range(1, steps + 1):
        near = LF.apply_bf16("sgd", sc, ids, g, near, row_begin=5, rounding="nearest")[0]
        sto = LF.apply_bf16("sgd", sc, ids, g, sto, row_begin=5, rounding="stochastic", seed=seed, step_no=t)[0]
    assert (near == 0x3F80).all(), "nearest rounding moved a weight by a step below half an ulp"
    drift = float((1.0 - BF.from_bf16_bits(sto).astype(np.float64)).mean())
    print(f"seed {seed}: mean of 1 - w = {drift:.6f} (2^-4 = {2.0 ** -4:.6f}, sd of the mean 2^-11 = {2.0 ** -11:.6f})")
    assert abs(drift - 2.0 ** -4) <= 6 * 2.0 ** -11


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [8, 264, 1032])
def test_fixture_is_close_to_float64(kind, d):
    rng = np.random.default_rng(d)
    rows = 16
    hp = dict(lr=0.05, eps=1e-10, weight_decay=0.01, grad_scale=0.5)
    sc32, sc64 = lean_scalars(kind, **hp), LF.scalars_f64(kind, **hp)
    w = rng.standard_normal((rows, d)).astype(np.float32)
    s = (rng.standard_normal(rows) ** 2).astype(np.float32)
    w64, s64 = w.astype(np.float64), s.astype(np.float64)
    for _ in range(3):
        g = rng.standard_normal((rows, d)).astype(np.float32)
        before = np.abs(w64)
        w, s = LF.step_f32(kind, sc32, g, w, s)
        new64, s64 = LF.step_f64(kind, sc64, g, w64, s64)
        update = np.abs(new64 - w64)
        w64 = new64
        err = np.abs(w.astype(np.float64) - w64)
        bound = 4 * 2.0 ** -23 * (before + update) * 3          # three steps accumulate
        assert (err <= bound).all(), f"{kind} d={d}: {float((err / bound).max()):.2f} of the bound"
        if kind == "rowwise_adagrad":
            assert np.allclose(s, s64, rtol=1e-5, atol=0) and s.dtype == np.float32


def test_row_sum_order_is_the_contract():
    rng = np.random.default_rng(2)
    for d in (8, 256, 264, 1024, 1032, 4104):
        g = rng.standard_normal((2, d)).astype(np.float32)
        got = LF.row_sum_sq(g)
        for row in range(2):
            q = [np.float32(0)] * 64
            for j in range(d):                                  # ascending j: every lane sees its elements in ascending j
                lane = (j // 4) % 64
                q[lane] = np.float32(q[lane] + np.float32(g[row, j] * g[row, j]))
            for s in (32, 16, 8, 4, 2, 1):
                q = [np.float32(q[lane] + q[lane ^ s]) for lane in range(64)]
            assert len({x.view(np.uint32) for x in q}) == 1
            assert got[row].view(np.uint32) == q[0].view(np.uint32), d
        plain = (g.astype(np.float64) ** 2).sum(axis=1)
        assert np.allclose(got, plain, rtol=1e-5)
    # the wrong machines are told apart on ordinary values
    g = rng.standard_normal((64, 768)).astype(np.float32)
    assert (LF.row_sum_sq(g, fma=True).view(np.uint32) != LF.row_sum_sq(g).view(np.uint32)).any()
    tiny = (rng.standard_normal((4, 264)) * 2.0 ** -70).astype(np.float32)       # squares are subnormal
    assert (LF.row_sum_sq(tiny) != 0).all() and (LF.row_sum_sq(tiny, ftz=True) == 0).all()
