"""CPU: the host half of the fused optimizer step (include/scone_hip.h, "optimizer step").

1. `scone_opt_scalars_of` against its definition in numpy double (tests/opt_fixture.py scalars_f64) rounded to fp32: within one
   fp32 ulp (a libm `pow` may differ from numpy's in the last place), for the three kinds, t = 1, 2, 1000, 10^6 and beta2 = 0.999
   and 0.95; what the call refuses, without a GPU.
2. The fixture (the contract in np.float32, one operation per rounding) against torch's own optimizers on CPU tensors: three
   steps over changing sets of 25 of 60 rows, d = 64, standard-normal data.  Error = the largest difference from the same
   formulas in float64.  The fixture's error must be at most max(2 x torch's own fp32 error, 2^-23 x max|w|): both sides are
   fp32 evaluations with different legal operation orders (factor 2), and the second term is one ulp at the largest weight.
   Bit equality with torch is not the contract.
3. weight_decay = 0 and grad_scale = 1 leave the bits of the plain update; other values change them.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_fixture as OF  # noqa: E402

from scone_amd import _lib  # noqa: E402
from scone_amd.hip_backend import opt_scalars  # noqa: E402

KINDS = ("sgd", "adagrad", "adam")


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0
    ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
    return abs(ia - ib)


@pytest.mark.parametrize("beta2", [0.999, 0.95])
@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
@pytest.mark.parametrize("kind", KINDS)
def test_scalars_equal_the_double_definition(kind, step, beta2):
    hp = dict(lr=3e-3, betas=(0.9, beta2), eps=1e-8, weight_decay=0.01, grad_scale=0.5, step=step)
    got = opt_scalars(kind, **hp)
    want = OF.scalars_f32(kind, **hp)
    assert sorted(got) == sorted(OF.NAMES)
    for name in OF.NAMES:
        assert isinstance(got[name], np.float32) and np.isfinite(got[name])
        assert _ulps(got[name], want[name]) <= 1, f"{name}: {got[name]!r} vs {want[name]!r}"
    for name in ("b1", "b2", "c1", "c2", "eps", "decay", "gscale"):        # no pow behind these: exact
        assert got[name] == want[name], name
    if kind != "adam":
        assert got["alpha"] == np.float32(3e-3)
    elif step == 1:
        assert got["alpha"] != np.float32(3e-3), "no bias correction at t = 1"


def test_scalars_refusals_need_no_gpu():
    lib = _lib.lib()
    out = _lib.OptScalars()

    def call(**kw):
        hp = dict(struct_size=C.sizeof(_lib.OptCfg), kind=_lib.OPT_ADAM, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, grad_scale=1.0, step=1)
        hp.update(kw)
        return lib.scone_opt_scalars_of(C.byref(_lib.OptCfg(**hp)), C.byref(out))

    assert C.sizeof(_lib.OptCfg) == 64 and C.sizeof(_lib.OptScalars) == 32
    assert call() == _lib.OK
    assert lib.scone_opt_scalars_of(None, C.byref(out)) == _lib.EINVAL
    assert lib.scone_opt_scalars_of(C.byref(_lib.OptCfg(C.sizeof(_lib.OptCfg), 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1)), None) == _lib.EINVAL
    assert call(struct_size=8) == _lib.EINVAL
    assert call(kind=3) == _lib.EINVAL and call(kind=-1) == _lib.EINVAL
    assert call(step=0) == _lib.EINVAL and call(step=-5) == _lib.EINVAL
    assert call(kind=_lib.OPT_SGD, step=0) == _lib.OK and call(kind=_lib.OPT_ADAGRAD, step=-1) == _lib.OK
    for name in ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(**{name: bad}) == _lib.EINVAL, (name, bad)
    assert lib.scone_opt_step(None, None, None, None, 0, None, None, None, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        opt_scalars("adam", 1e-3, step=0)
    with pytest.raises(ValueError):
        opt_scalars("rmsprop", 1e-3)


# ------------------------------------------------------------------ the fixture against torch on the CPU
N, D, U, STEPS = 60, 64, 25, 3
HP = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8)


def _data(seed):
    rng = np.random.default_rng(seed)
    w0 = rng.standard_normal((N, D)).astype(np.float32)
    ids = [np.sort(rng.choice(N, size=U, replace=False)).astype(np.int64) for _ in range(STEPS)]
    grads = [rng.standard_normal((U, D)).astype(np.float32) for _ in range(STEPS)]
    assert len({tuple(i) for i in ids}) == STEPS, "the id sets do not change"
    return w0, ids, grads


def _torch_run(kind, w0, ids, grads):
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    if kind == "sgd":
        opt = torch.optim.SGD([p], lr=HP["lr"])
    elif kind == "adagrad":
        opt = torch.optim.Adagrad([p], lr=HP["lr"], eps=HP["eps"])
    else:
        opt = torch.optim.SparseAdam([p], lr=HP["lr"], betas=HP["betas"], eps=HP["eps"])
    for i, g in zip(ids, grads):
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(i)[None], torch.from_numpy(g), (N, D), is_coalesced=True)
        opt.step()
    return p.detach().numpy()


def _fixture_run(kind, w0, ids, grads, f64=False, **hp_more):
    dt = np.float64 if f64 else np.float32
    w, m, v = w0.astype(dt), np.zeros((N, D), dtype=dt), np.zeros((N, D), dtype=dt)
    for t, (i, g) in enumerate(zip(ids, grads), start=1):
        hp = dict(HP, step=t, **hp_more)
        if f64:
            w, m, v, _, bad = OF.apply(kind, OF.scalars_f64(kind, **hp), i, g, w, m, v, step=OF.step_f64)
        else:
            w, m, v, _, bad = OF.apply(kind, opt_scalars(kind, **hp), i, g, w, m, v)
        assert not bad
    return w


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_is_as_close_to_float64_as_torch(kind):
    w0, ids, grads = _data(11)
    exact = _fixture_run(kind, w0, ids, grads, f64=True)
    ours = _fixture_run(kind, w0, ids, grads)
    theirs = _torch_run(kind, w0, ids, grads)
    assert ours.dtype == np.float32 and theirs.dtype == np.float32
    err_ours = float(np.abs(ours.astype(np.float64) - exact).max())
    err_torch = float(np.abs(theirs.astype(np.float64) - exact).max())
    ulp = 2.0 ** -23 * float(np.abs(exact).max())
    print(f"{kind}: fixture {err_ours:.3e}  torch {err_torch:.3e}  ulp term {ulp:.3e}")
    assert err_torch < 1e-5, "torch does not compute these formulas"
    assert err_ours <= max(2.0 * err_torch, ulp)
    touched = np.unique(np.concatenate(ids))
    rest = np.setdiff1d(np.arange(N), touched)
    assert len(rest) and np.array_equal(ours[rest].view(np.uint32), w0[rest].view(np.uint32)), "a row that was never listed changed"


@pytest.mark.parametrize("kind", KINDS)
def test_decay_and_grad_scale_are_skipped_exactly(kind):
    w0, ids, grads = _data(12)
    w0[0, :4] = [-0.0, 0.0, np.inf, -np.inf]                     # 0 * inf and -0 - (0 * -0) would show a step that is not skipped
    ids[0][0] = 0
    plain = _fixture_run(kind, w0, ids, grads)
    explicit = _fixture_run(kind, w0, ids, grads, weight_decay=0.0, grad_scale=1.0)
    assert np.array_equal(plain.view(np.uint32), explicit.view(np.uint32))
    assert np.isinf(plain[0, 2]) and np.isinf(plain[0, 3]) and not np.isnan(plain[0, :4]).any()
    decayed = _fixture_run(kind, w0, ids, grads, weight_decay=0.01)
    scaled = _fixture_run(kind, w0, ids, grads, grad_scale=0.5)
    assert (decayed.view(np.uint32) != plain.view(np.uint32)).any() and (scaled.view(np.uint32) != plain.view(np.uint32)).any()
    assert np.isnan(decayed[0, 2]), "0.0005 * inf subtracted from inf"
