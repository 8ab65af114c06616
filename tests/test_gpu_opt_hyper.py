"""The optimizer's hyper-parameters on the device (include/scone_hip.h, "optimizer hyper-parameters on the device"): the block and
its advance, the `hyper=` forms of `opt_step` / `opt_step_lean` / `grad_ctl`, and `FGramOptimizer(capturable=True)`.

Expectations.  The block: tests/opt_hyper_fixture.py, written from the header.  The steps: the contract is "the bits of
scone_opt_step_dn / scone_opt_step_lean_dn given those scalars", so the by-value call on a clone, with the same hyper-parameters
and the same t, IS the reference (its own bits are pinned by tests/test_gpu_opt_step.py and test_gpu_opt_lean.py).  Adam's step
size is computed with the header's integer power on the new road and with pow() on the old; wherever the two roads are compared
the test first asserts that the two step sizes have equal bits at the (lr, betas, t) it uses.  No tolerance anywhere: every
comparison is of bits or bytes.

Buffers are U + 64 rows with NaN rows and ids of -7 behind the count: a kernel that ignored the count, or ran although the
block said "not applied", would read them and raise SCONE_ST_BAD_ID."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_fixture as E  # noqa: E402
import opt_hyper_fixture as HF  # noqa: E402
import stream_fixture as SF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only)
import test_gpu_backward_dn as DN  # noqa: E402  (helpers only: guarded inputs, control blocks, table bytes, capture)
import test_gpu_opt_step as TO  # noqa: E402  (helpers only: small tables without an index)

pytestmark = pytest.mark.gpu

GUARD = DN.GUARD
N_OPT, U_OPT = DN.N_OPT, DN.U_OPT
HEADER = DN.HEADER


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _L():
    from scone_amd import _lib
    return _lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits32(x):
    return int(np.float32(x).view(np.uint32))


def _count(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


def _f64(x):
    return torch.tensor(x, dtype=torch.float64, device="cuda")


def _same_alpha(kind, lr, t, betas=(0.9, 0.999)):
    """The precondition of every comparison with the by-value road: the two roads' scalars have equal bits here."""
    from scone_amd.hip_backend import opt_hyper_scalars, opt_scalars
    k = kind if kind in ("sgd", "adagrad", "adam") else "sgd"
    a, b = opt_hyper_scalars(k, lr, betas=betas, step=t), opt_scalars(k, lr, betas=betas, step=t)
    assert {n: _bits32(v) for n, v in a.items()} == {n: _bits32(v) for n, v in b.items()}, f"{kind} lr {lr} t {t}: {a} != {b}"


# ------------------------------------------------------------------ 1. the block and its advance
HP1 = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=0.5)


def _fixture_block(hp, seed, step):
    return HF.init(hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], hp["grad_scale"], seed, step)


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("t0", [0, 6])
def test_advance_equals_the_fixture(t0, kind):
    t = TO._table("fp32", 8)
    hy = t.opt_hyper(**HP1, seed=(1 << 63) + 77, step=t0)
    want = _fixture_block(HP1, (1 << 63) + 77, t0)
    assert HF.same_block(hy.read(), want), f"init: {hy.read()} != {want}"
    for i in range(5):
        t.opt_hyper_advance(hy, kind)
        want = HF.advance(want, kind)
        got = hy.read()
        assert HF.same_block(got, want), f"advance {i + 1} from {t0}: {got} != {want}"
        assert got["step"] == t0 + i + 1 and got["applied"] == 1 and got["bad"] == 0
    assert int(hy.step.item()) == t0 + 5 and float(hy.lr.item()) == HP1["lr"] and int(hy.applied.item()) == 1, "the views"
    assert t.status() == 0


def test_advance_skipped_bad_and_saturated():
    t = TO._table("fp32", 8)
    hy = t.opt_hyper(**HP1, seed=5, step=2)
    t.opt_hyper_advance(hy, "adam")
    before = hy.buf.clone()
    want = hy.read()
    # a set skip flag: the 104 bytes are unchanged but for applied
    t.opt_hyper_advance(hy, "adam", ctl=DN._ctl_of(t, "skip"))
    got = hy.read()
    assert got["applied"] == 0 and got["step"] == 3
    assert HF.same_block(dict(got, applied=1), want)
    after = hy.buf.clone()
    after.view(torch.int32)[_L().SconeOptHyper.applied.offset // 4] = 1
    assert torch.equal(after.view(torch.uint8), before.view(torch.uint8)), "a skipped advance changed a byte other than applied"
    # a control block that does not skip advances
    t.opt_hyper_advance(hy, "adam", ctl=DN._ctl_of(t, "coef"))
    want = HF.advance(want, "adam")
    assert HF.same_block(hy.read(), want) and want["step"] == 4
    # a value that is not finite, written by device work of the caller's
    for field, value in (("lr", float("inf")), ("grad_scale", float("nan")), ("beta2", float("-inf"))):
        good = getattr(hy, field).clone()
        getattr(hy, field).copy_(_f64(value))
        t.opt_hyper_advance(hy, "adam")
        got = hy.read()
        assert got["bad"] == 1 and got["applied"] == 0 and got["step"] == 4, f"{field} = {value}: {got}"
        assert {k: _bits32(v) for k, v in got["sc"].items()} == {k: _bits32(v) for k, v in want["sc"].items()}, "sc changed"
        getattr(hy, field).copy_(good)
    t.opt_hyper_advance(hy, "adam")
    want = HF.advance(want, "adam")
    assert HF.same_block(hy.read(), want) and want["bad"] == 0 and want["step"] == 5, "a good advance clears bad"
    # the count saturates instead of wrapping
    hy.step.fill_(HF.INT64_MAX)
    t.opt_hyper_advance(hy, "sgd")
    got = hy.read()
    assert got["step"] == HF.INT64_MAX and got["bad"] == 1 and got["applied"] == 0
    assert t.status() == 0


def test_refusals_of_the_library():
    L = _L()
    lib = L.lib()
    t = TO._table("bf16", 72)
    hy = t.opt_hyper(lr=0.1)
    err = lambda: lib.scone_last_error(t._h).decode()  # noqa: E731

    def cfg(**change):
        c = L.OptCfg(C.sizeof(L.OptCfg), L.OPT_ADAM, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 0)
        for k, v in change.items():
            setattr(c, k, v)
        return c
    assert lib.scone_opt_hyper_init(t._h, C.byref(cfg()), 0, _ptr(hy.buf), None) == L.OK, "step = 0: no step applied yet, any kind"
    for change, word in ((dict(step=-1), ">= 0"), (dict(kind=7), "bad kind"), (dict(struct_size=4), "struct_size"),
                         (dict(lr=float("nan")), "finite"), (dict(grad_scale=float("inf")), "finite")):
        assert lib.scone_opt_hyper_init(t._h, C.byref(cfg(**change)), 0, _ptr(hy.buf), None) == L.EINVAL and word in err(), change
        assert err().startswith("scone_opt_hyper_init: ")
    assert lib.scone_opt_hyper_init(t._h, None, 0, _ptr(hy.buf), None) == L.EINVAL and "null cfg" in err()
    assert lib.scone_opt_hyper_init(t._h, C.byref(cfg()), 0, None, None) == L.EINVAL and "null d_hyper" in err()
    assert lib.scone_opt_hyper_advance(t._h, 3, _ptr(hy.buf), None, None) == L.EINVAL and "bad kind" in err()
    assert lib.scone_opt_hyper_advance(t._h, 0, None, None, None) == L.EINVAL and "null d_hyper" in err()
    ids, rows, n = DN._guarded(0, 72)
    W = torch.zeros((N_OPT, 72), device="cuda")
    S = torch.zeros(N_OPT, device="cuda")
    step = lambda **kw: lib.scone_opt_step_dh(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("h", t._h), ("kind", 0), ("ids", _ptr(ids)), ("rows", _ptr(rows)), ("n", _ptr(n)), ("cap", GUARD), ("w", _ptr(W)), ("s1", None),
        ("s2", None), ("hy", _ptr(hy.buf)), ("ctl", None), ("stream", None))])
    assert step(hy=None) == L.EINVAL and "null d_hyper" in err() and err().startswith("scone_opt_step_dh: ")
    assert step(n=None) == L.EINVAL and "null d_n" in err()
    assert step(kind=5) == L.EINVAL and "bad kind" in err()
    assert step(w=None) == L.EINVAL and "null pointer" in err()
    assert step(kind=2) == L.EINVAL and "d_state1" in err()
    assert step(kind=1) == L.EINVAL and "d_state2" in err()
    assert step(cap=0, ids=None, rows=None) == L.OK, "n_cap == 0 is a no-op"
    lean = lambda **kw: lib.scone_opt_step_lean_dh(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("h", t._h), ("kind", 0), ("rounding", 0), ("ids", _ptr(ids)), ("rows", _ptr(rows)), ("n", _ptr(n)), ("cap", GUARD), ("w", None),
        ("s", _ptr(S)), ("hy", _ptr(hy.buf)), ("ctl", None), ("stream", None))])
    assert lean(hy=None) == L.EINVAL and "null d_hyper" in err() and err().startswith("scone_opt_step_lean_dh: ")
    assert lean(n=None) == L.EINVAL and "null d_n" in err()
    assert lean(kind=2) == L.EINVAL and "bad kind" in err()
    assert lean(rounding=2) == L.EINVAL and "bad rounding" in err()
    assert lean(rounding=1, w=_ptr(W)) == L.EINVAL and "nothing to round" in err()
    assert lean(kind=1, s=None) == L.EINVAL and "d_row_state" in err()
    i8 = TO._table("int8", 80)
    assert lib.scone_opt_step_lean_dh(i8._h, 0, 0, _ptr(ids), _ptr(rows), _ptr(n), GUARD, None, None, _ptr(hy.buf), None,
                                      None) == L.EINVAL and "int8" in lib.scone_last_error(i8._h).decode()
    sq = _f64([9.0])
    ctl = DN._ctl_of(t, "coef")
    assert lib.scone_grad_ctl_set_dh(t._h, _ptr(sq), 1, None, 1.0, 0, _ptr(ctl.buf), None) == L.EINVAL and "null d_hyper" in err()
    assert lib.scone_grad_ctl_set_dh(t._h, _ptr(sq), 0, _ptr(hy.buf), 1.0, 0, _ptr(ctl.buf), None) == L.EINVAL and "n_terms" in err()
    assert lib.scone_grad_ctl_set_dh(t._h, None, 1, _ptr(hy.buf), 1.0, 0, _ptr(ctl.buf), None) == L.EINVAL
    assert lib.scone_grad_ctl_set_dh(t._h, _ptr(sq), 1, _ptr(hy.buf), 0.0, 0, _ptr(ctl.buf), None) == L.EINVAL and "max_norm" in err()
    with pytest.raises(ValueError, match="hyper="):
        t.opt_step_lean(ids, rows, kind="sgd", lr=0.1, n=n, hyper=hy)
    with pytest.raises(ValueError, match="seed"):
        t.opt_hyper(lr=0.1, seed=-1)
    torch.cuda.synchronize()
    want = t.opt_hyper(lr=0.1)
    lib.scone_opt_hyper_init(t._h, C.byref(cfg()), 0, _ptr(want.buf), None)
    assert torch.equal(hy.buf.view(torch.uint8), want.buf.view(torch.uint8)), "a refused call wrote the block"
    assert int(n.item()) == -5 and t.status() == 0 and i8.status() == 0


# ------------------------------------------------------------------ 2. the _dh steps: the by-value call on a clone
T_STEP = 3          # Adam's t of every step below: the block is initialised at T_STEP - 1 steps applied
HP2 = dict(lr=0.05, weight_decay=0.01, grad_scale=0.5)


def _bad_block(t, **hp):
    """A block whose last advance did not apply (a learning rate that is not finite): bad = 1, applied = 0."""
    hy = t.opt_hyper(step=T_STEP - 1, **hp)
    hy.lr.copy_(_f64(float("inf")))
    t.opt_hyper_advance(hy, "sgd")
    got = hy.read()
    assert got["bad"] == 1 and got["applied"] == 0 and got["step"] == T_STEP - 1
    return hy


@pytest.mark.parametrize("which", DN.CTLS)
@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("fmt,d", [("int8", 80), ("fp32", 8), ("int8", 1040)])
def test_opt_step_dh_equals_the_by_value_call(fmt, d, kind, which):
    """(("int8", 1040): a row wider than the 1024 elements a wave keeps in registers -- the kernels' second store path.)"""
    _same_alpha(kind, HP2["lr"], T_STEP)
    rng, ids_buf, rows_buf = DN._opt_inputs(d, 7 * d)
    w = rng.standard_normal((N_OPT, d)).astype(np.float32)
    m, v = (0.1 * rng.standard_normal((N_OPT, d))).astype(np.float32), (rng.standard_normal((N_OPT, d)) ** 2).astype(np.float32)
    ends = []
    for road in ("value", "dh", "dh-above-cap", "dh-not-applied"):
        t = TO._table(fmt, d)
        t.store_f32(torch.from_numpy(w))
        W, M, V = (torch.from_numpy(x).cuda() for x in (w, m, v))
        ctl = DN._ctl_of(t, which)
        if road == "value":
            t.opt_step(ids_buf[:U_OPT], rows_buf[:U_OPT], W, kind=kind, state1=M, state2=V, ctl=ctl, step=T_STEP, **HP2)
        elif road == "dh-not-applied":
            # every listed row is readable here and the count covers the guard rows: a kernel that ran would raise SCONE_ST_BAD_ID
            t.opt_step(ids_buf, rows_buf, W, kind=kind, state1=M, state2=V, ctl=None if which == "skip" else ctl,
                       n=_count(U_OPT + GUARD), hyper=_bad_block(t, **HP2))
        else:
            hy = t.opt_hyper(step=T_STEP - 1, **HP2)
            t.opt_hyper_advance(hy, kind, ctl)
            got = hy.read()
            assert got["applied"] == (which != "skip") and got["step"] == T_STEP - (which == "skip") and got["bad"] == 0
            if road == "dh":
                t.opt_step(ids_buf, rows_buf, W, kind=kind, state1=M, state2=V, ctl=ctl, n=_count(U_OPT), hyper=hy)
            else:                                                # n = min(*d_n, n_cap): a count above the capacity is the capacity
                t.opt_step(ids_buf[:U_OPT], rows_buf[:U_OPT], W, kind=kind, state1=M, state2=V, ctl=ctl, n=_count(U_OPT + 1000),
                           hyper=hy)
        assert t.status() == 0, f"{road}: a row behind the count was read, or a step that was not applied ran"
        ends.append((road, [x.cpu().numpy() for x in (W, M, V)], DN._table_bytes(t)))
    assert bool((ids_buf[U_OPT:] == -7).all()) and bool(torch.isnan(rows_buf[U_OPT:]).all()), "the guard rows stay poisoned"
    ref = ends[0]
    assert (not E.same_bits(ref[1][0], w)) == (which != "skip"), "the reference: a skipped step changes nothing, any other does"
    for road, arrays, tb in ends[1:3]:
        for name, got, want in zip(("master", "state1", "state2"), arrays, ref[1]):
            assert E.same_bits(got, want), f"{road}: {name}: {E.first_difference(got, want)}"
        assert DN._same_table(tb, ref[2]), f"{road}: the served rows or scales differ"
    road, arrays, tb = ends[3]
    start = TO._table(fmt, d)
    start.store_f32(torch.from_numpy(w))
    for name, got, want in zip(("master", "state1", "state2"), arrays, (w, m, v)):
        assert E.same_bits(got, want), f"{road}: {name} changed"
    assert DN._same_table(tb, DN._table_bytes(start)), f"{road}: the served table changed"


@pytest.mark.parametrize("which", DN.CTLS)
@pytest.mark.parametrize("kind", ["sgd", "rowwise_adagrad"])
@pytest.mark.parametrize("mode", list(DN.LEAN_MODES))
def test_opt_step_lean_dh_equals_the_by_value_call(mode, kind, which):
    fmt, with_master, rounding = DN.LEAN_MODES[mode]
    _same_alpha("sgd", HP2["lr"], T_STEP + 1)
    d = 80 if fmt == "int8" else 72
    rng, ids_buf, rows_buf = DN._opt_inputs(d, 11 * d)
    w = rng.standard_normal((N_OPT, d)).astype(np.float32)
    s = (rng.standard_normal(N_OPT) ** 2).astype(np.float32)
    seed, step = 13, T_STEP + 1
    ends = []
    for road in ("value", "dh", "dh-not-applied"):
        t = TO._table(fmt, d)
        t.store_f32(torch.from_numpy(w))
        start = DN._table_bytes(t)
        W = torch.from_numpy(w).cuda() if with_master else None
        S = torch.from_numpy(s).cuda()
        ctl = DN._ctl_of(t, which)
        if road == "value":
            t.opt_step_lean(ids_buf[:U_OPT], rows_buf[:U_OPT], kind=kind, master=W, row_state=S, ctl=ctl, rounding=rounding, seed=seed,
                            step=step, eps=1e-10, **HP2)
        elif road == "dh":
            hy = t.opt_hyper(step=step - 1, seed=seed, eps=1e-10, **HP2)
            t.opt_hyper_advance(hy, kind, ctl)
            assert hy.read()["step"] == step - (which == "skip")
            t.opt_step_lean(ids_buf, rows_buf, kind=kind, master=W, row_state=S, ctl=ctl, rounding=rounding, n=_count(U_OPT), hyper=hy)
        else:
            t.opt_step_lean(ids_buf, rows_buf, kind=kind, master=W, row_state=S, ctl=None if which == "skip" else ctl,
                            rounding=rounding, n=_count(U_OPT + GUARD), hyper=_bad_block(t, seed=seed, eps=1e-10, **HP2))
        assert t.status() == 0, f"{road}: a row behind the count was read, or a step that was not applied ran"
        ends.append(([None if W is None else W.cpu().numpy(), S.cpu().numpy()], DN._table_bytes(t), start))
    (ref, ref_tb, start), (got, got_tb, _), (idle, idle_tb, _) = ends
    assert DN._same_table(ref_tb, start) == (which == "skip"), "the reference: a skipped step changes nothing, any other does"
    if with_master:
        assert E.same_bits(got[0], ref[0]), f"master: {E.first_difference(got[0], ref[0])}"
        assert E.same_bits(idle[0], w), "not applied: master changed"
    assert E.same_bits(got[1], ref[1]), "row_state"
    assert DN._same_table(got_tb, ref_tb), "the served rows or scales differ"
    assert E.same_bits(idle[1], s) and DN._same_table(idle_tb, start), "not applied: the row state or the served table changed"
    assert bool((ids_buf[U_OPT:] == -7).all()) and bool(torch.isnan(rows_buf[U_OPT:]).all()), "the guard rows stay poisoned"


# ------------------------------------------------------------------ 3. the control block from a scale on the device
@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0 ** -16])
def test_grad_ctl_from_the_block_equals_the_by_value_call(scale):
    t = TO._table("fp32", 8)
    hy = t.opt_hyper(lr=0.1, grad_scale=scale)
    for terms, max_norm, guard in (([9.0], 1.0, False), ([9.0, 16.0e8], 3.0, True), ([0.25], None, False), ([float("inf")], 1.0, True),
                                   ([float("nan"), 1.0], 1.0, False)):
        terms = [_f64(x) for x in terms]
        want = t.grad_ctl(terms, grad_scale=scale, max_norm=max_norm, skip_nonfinite=guard)
        got = t.grad_ctl(terms, max_norm=max_norm, skip_nonfinite=guard, hyper=hy)
        assert torch.equal(got.buf.view(torch.uint8), want.buf.view(torch.uint8)), f"{terms}: {got.read()} != {want.read()}"
    assert t.status() == 0


def test_grad_ctl_with_a_scale_that_is_not_finite_declines_the_step():
    t = TO._table("fp32", 8)
    hy = t.opt_hyper(lr=0.1, grad_scale=0.5)
    for bad in (float("nan"), float("inf")):
        hy.grad_scale.copy_(_f64(bad))
        got = t.grad_ctl([_f64(9.0)], max_norm=1.0, hyper=hy).read()             # (skip_nonfinite is not even set)
        assert got["skip"] == 1 and _bits32(got["coef"]) == _bits32(1.0) and got["sqnorm"] == 9.0 and got["reserved"] == 0, got
    assert t.status() == 0


# ------------------------------------------------------------------ 4. capture and replay of the entry points
CAPTURE_DH = {"int8-master-adam": ("int8", True, "adam", "nearest"), "bf16-inplace-sgd-stochastic": ("bf16", False, "sgd", "stochastic")}
SCHEDULE = [(1e-3, 1.0), (2e-3, 0.5), (5e-4, 2.0 ** -7), (1.5e-3, 0.25)]       # (lr, grad_scale) of the steps applied, in order


@pytest.mark.parametrize("case", list(CAPTURE_DH))
def test_capture_and_replay_of_the_entry_points(case):
    """plan_dn; rows_dn; sqnorm_dn; ctl_set_dh; hyper_advance; opt_step*_dh captured once as a linear graph and replayed on other
    batches, with a new lr and a new grad_scale copied into the block between replays: table, master, m and v equal an eager
    twin stepped by the BY-VALUE road at the same t, lr and grad_scale.  One replay carries an inf gradient with skip_nonfinite:
    nothing changes, the count stays, and the next replay is the twin's next step at the un-advanced t."""
    from scone_amd.hip_backend import GradCtl
    fmt, with_master, kind, rounding = CAPTURE_DH[case]
    for i, (lr, _) in enumerate(SCHEDULE):
        _same_alpha(kind, lr, i + 1)
    w0, (cache, twin_cache) = DN._twin_tables(fmt)
    t, twin = cache.to_device(), twin_cache.to_device()
    n_rows, D = TB.N_ROWS[DN.CAP_N], DN.CAP_D
    toks, grads = DN._capture_batches()
    tok_s, g_s = torch.from_numpy(toks[0]).cuda(), grads[0].cuda()
    masters = [torch.from_numpy(w0).cuda() if with_master else None for _ in range(2)]
    ms = [torch.zeros((n_rows, D), device="cuda") if kind == "adam" else None for _ in range(2)]
    vs = [torch.zeros((n_rows, D), device="cuda") if kind == "adam" else None for _ in range(2)]
    ctx = t.backward_context(DN.CAP_B * DN.CAP_T)
    ids, rows, n = DN._guarded(n_rows, D, cap=n_rows)
    sq = torch.zeros((), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_L().grad_sqnorm_scratch(n_rows), dtype=torch.float64, device="cuda")
    ctl = GradCtl(t.device)
    seed, wd = 21, 0.01
    hy = t.opt_hyper(lr=SCHEDULE[0][0], grad_scale=SCHEDULE[0][1], weight_decay=wd, eps=1e-8 if kind == "adam" else 1e-10, seed=seed)

    def chain(warm_up):
        ctx.plan(tok_s)
        ctx.rows(g_s, "mean", out=(ids, rows, n))
        t.grad_sqnorm(rows, scratch, n=n, out=sq)
        t.grad_ctl([sq], max_norm=1.0, skip_nonfinite=True, out=ctl, hyper=hy)
        t.opt_hyper_advance(hy, kind, ctl)
        if kind == "adam":
            t.opt_step(ids, rows, masters[0], kind=kind, state1=ms[0], state2=vs[0], ctl=ctl, n=n, hyper=hy)
        else:
            t.opt_step_lean(ids, rows, kind=kind, rounding=rounding, ctl=ctl, n=n, hyper=hy)

    def eager(i, step):
        lr, gs = SCHEDULE[step - 1]
        with twin.backward_plan(torch.from_numpy(toks[i])) as plan:
            r_ids, r_rows = plan.rows(grads[i].cuda(), "mean")
            c2 = twin.grad_ctl([twin.grad_sqnorm(r_rows)[0]], grad_scale=gs, max_norm=1.0, skip_nonfinite=True)
            if kind == "adam":
                twin.opt_step(r_ids, r_rows, masters[1], kind=kind, lr=lr, step=step, state1=ms[1], state2=vs[1], weight_decay=wd,
                              grad_scale=gs, ctl=c2)
            else:
                twin.opt_step_lean(r_ids, r_rows, kind=kind, lr=lr, weight_decay=wd, grad_scale=gs, rounding=rounding, seed=seed,
                                   step=step, ctl=c2)
            return plan.n_rows, c2.read()

    def compare(tag, step, U=None, c2=None):
        torch.cuda.synchronize()
        got_h = hy.read()
        assert got_h["step"] == step and got_h["bad"] == 0, f"{tag}: the block counts {got_h['step']} applied steps, not {step}"
        if c2 is not None:
            assert int(n.item()) == U, f"{tag}: the count"
            got = ctl.read()
            assert _bits32(got["coef"]) == _bits32(c2["coef"]) and got["skip"] == 0 and got_h["applied"] == 1, f"{tag}: ctl {got} / {c2}"
        assert DN._same_table(DN._table_bytes(t), DN._table_bytes(twin)), f"{tag}: the served table differs from the eager twin's"
        for name, pair in (("master", masters), ("m", ms), ("v", vs)):
            if pair[0] is not None:
                assert E.same_bits(pair[0].cpu().numpy(), pair[1].cpu().numpy()), f"{tag}: {name}"

    def put(step):
        lr, gs = SCHEDULE[step - 1]
        hy.lr.copy_(_f64(lr))                                       # device copies: what a scheduler and a loss scaler would enqueue
        hy.grad_scale.copy_(_f64(gs))

    g = DN._capture(chain, case)
    compare("warm-up", 1, *eager(0, 1))                            # the warm-up ran once, eagerly, on batch 0: step 1
    start = DN._table_bytes(t)
    step = 1
    for i, poisoned in ((1, False), (2, True), (2, False), (3, False)):
        tok_s.copy_(torch.from_numpy(toks[i]))
        g_s.copy_(grads[i])
        if poisoned:
            g_s[:, 3] = float("inf")                                # every position: whichever rows the batch touches
            put(step + 1)
            g.replay()
            torch.cuda.synchronize()
            assert ctl.read()["skip"] == 1 and hy.read()["applied"] == 0
            compare(f"replay {i} with an inf gradient", step)       # nothing changed: still the twin, which was not stepped
            continue
        step += 1
        put(step)
        g.replay()
        compare(f"replay {i}", step, *eager(i, step))
    assert step == 4 and not DN._same_table(DN._table_bytes(t), start), "the replays left the table as it was"
    assert t.status() == 0 and twin.status() == 0
    ctx.close()


# ------------------------------------------------------------------ 5. the module layer
MODULE_CASES = {"int8-master-adam": ("int8", True, "adam", "nearest", 1e-3),
                "bf16-inplace-sgd-stochastic": ("bf16", False, "sgd", "stochastic", 0.05)}


def _modules(case, static, seed=43):
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    fmt, with_master, kind, rounding, lr = MODULE_CASES[case]
    w0, caches = DN._twin_tables(fmt, seed=seed)
    kw = dict(static_rows=TB.N_ROWS[DN.CAP_N], max_tokens=DN.CAP_B * DN.CAP_T) if static else {}
    if with_master:
        fg, fg2 = TrainableFGramTable(caches[0], torch.from_numpy(w0.copy()), **kw), TrainableFGramTable(caches[1], torch.from_numpy(w0.copy()))
    else:
        fg, fg2 = InPlaceFGramTable(caches[0], **kw), InPlaceFGramTable(caches[1])
    okw = dict(lr=lr, weight_decay=0.01, rounding=rounding, seed=9)
    return fg, fg2, FGramOptimizer(fg, kind, capturable=True, **okw), FGramOptimizer(fg2, kind, **okw), caches, okw


def _same_modules(tag, fg, fg2, opt, opt2, caches):
    torch.cuda.synchronize()
    assert DN._same_table(DN._table_bytes(caches[0].to_device()), DN._table_bytes(caches[1].to_device())), f"{tag}: the served table"
    if hasattr(fg, "weight"):
        assert E.same_bits(fg.weight.detach().cpu().numpy(), fg2.weight.detach().cpu().numpy()), f"{tag}: weight"
    for name in ("state1", "state2"):
        a, b = getattr(opt, name), getattr(opt2, name)
        assert (a is None) == (b is None), f"{tag}: {name}"
        if a is not None:
            assert E.same_bits(a.cpu().numpy(), b.cpu().numpy()), f"{tag}: {name}"


@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_capture_and_replay_of_the_module_layer(case):
    """fg(ids).sum().backward(); opt.step(max_norm=, skip_nonfinite=) with capturable=True and static_rows=, captured and replayed
    on three other batches, against the same loop run eagerly on a twin with neither (the by-value road): Adam beside a master
    and stochastic rounding in place -- the two that the default road refuses under capture.  Then a step the device skips, and
    a state_dict round trip into a fresh capturable optimizer."""
    from scone_amd import FGramOptimizer
    _, _, kind, _, lr = MODULE_CASES[case]
    for step in range(1, 7):
        _same_alpha(kind, lr if step < 5 else 2 * lr, step)
    fg, fg2, opt, opt2, caches, okw = _modules(case, static=True)
    toks, _ = DN._capture_batches()
    tok_s = torch.from_numpy(toks[0]).cuda()

    def loop(warm_up):
        fg(tok_s).sum().backward()
        opt.step(max_norm=1.0, skip_nonfinite=True)
        if warm_up:
            opt.zero_grad()

    def eager(i, o=opt2):
        fg2(torch.from_numpy(toks[i]).cuda()).sum().backward()
        o.step(max_norm=1.0, skip_nonfinite=True)
        o.zero_grad()

    g = DN._capture(loop, case)
    eager(0)
    _same_modules("warm-up", fg, fg2, opt, opt2, caches)
    for i in (1, 2, 3):
        tok_s.copy_(torch.from_numpy(toks[i]))
        g.replay()
        eager(i)
        _same_modules(f"replay {i}", fg, fg2, opt, opt2, caches)
        assert opt.last_ctl.read() == opt2.last_ctl.read() and not opt.found_nonfinite(), f"replay {i}: last_ctl"
    assert opt.t == 4 == opt2.t
    # a step the device skips does not advance t (on the default road it does, and the caller corrects it)
    before = DN._table_bytes(caches[0].to_device())
    opt.step(max_norm=1.0, extra_sqnorm=float("inf"), skip_nonfinite=True)
    assert opt.found_nonfinite() and opt.t == 4 and opt.hyper.read()["applied"] == 0
    assert DN._same_table(DN._table_bytes(caches[0].to_device()), before), "a skipped step changed the table"
    # a loss scale on the device, a learning rate assigned on the host: both are enqueued writes
    opt.lr = opt2.lr = 2 * lr
    opt.step(grad_scale=torch.tensor(0.5, dtype=torch.float64, device="cuda"), max_norm=1.0, skip_nonfinite=True)
    fg2(torch.from_numpy(toks[3]).cuda()).sum().backward()
    opt2.step(grad_scale=0.5, max_norm=1.0, skip_nonfinite=True)
    opt2.zero_grad()
    _same_modules("eager step 5", fg, fg2, opt, opt2, caches)
    assert opt.t == 5
    # state_dict round trip into a fresh capturable optimizer on the same module: the next step continues bit for bit
    sd = opt.state_dict()
    assert sd["capturable"] is True and sd["t"] == 5 and sd["lr"] == 2 * lr
    fresh = FGramOptimizer(fg, kind, capturable=True, **dict(okw, lr=123.0, seed=0))
    fresh.load_state_dict(sd)
    assert fresh.t == 5 and fresh.seed == 9 and fresh.hyper.read()["lr"] == 2 * lr
    opt.zero_grad()
    tok_s.copy_(torch.from_numpy(toks[1]))
    fg(tok_s).sum().backward()
    fresh.step(grad_scale=0.5, max_norm=1.0, skip_nonfinite=True)
    fg2(torch.from_numpy(toks[1]).cuda()).sum().backward()
    opt2.step(grad_scale=0.5, max_norm=1.0, skip_nonfinite=True)
    _same_modules("after the round trip", fg, fg2, fresh, opt2, caches)
    assert fresh.t == 6 and not fresh.rows_overflowed()
    assert caches[1].to_device().status() == 0


@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_capturable_eagerly_without_static_rows_equals_the_by_value_optimizer(case):
    """Non-static mode: the gradient is the module's, its row count goes into a device word the optimizer keeps."""
    _, _, kind, _, lr = MODULE_CASES[case]
    for step in range(1, 4):
        _same_alpha(kind, lr, step)
    fg, fg2, opt, opt2, caches, _ = _modules(case, static=False, seed=47)
    toks, _ = DN._capture_batches()
    for i, kw in enumerate((dict(), dict(grad_scale=0.25), dict(grad_scale=0.5, max_norm=1.0))):
        tok = torch.from_numpy(toks[i]).cuda()
        for m, o in ((fg, opt), (fg2, opt2)):
            m(tok).sum().backward()
            assert o.step(**kw) > 0
            o.zero_grad()
        _same_modules(f"step {i + 1}", fg, fg2, opt, opt2, caches)
    assert opt.t == 3 == opt2.t and opt.step() == 0 and opt.t == 3, "no gradient: nothing happens"
    g, marker = torch.cuda.CUDAGraph(), torch.zeros(1, device="cuda")
    fg(torch.from_numpy(toks[0]).cuda()).sum().backward()
    with torch.cuda.graph(g):
        with pytest.raises(ValueError, match="static_rows"):
            opt.step()
        marker.fill_(1.0)                                          # (a graph with nothing in it draws a warning)
    assert caches[0].to_device().status() == 0 and caches[1].to_device().status() == 0


# ------------------------------------------------------------------ 6. stream order
# The stream contract of the section: (class, the header's sentence, the test that holds the case), kept equal to the header's
# prototypes by test_every_entry_point_of_the_section_that_takes_a_stream_has_a_case.
CONTRACT_DH = {
    "scone_opt_hyper_init": (SF.A, "ONE launch of one thread stores the six doubles", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_opt_hyper_advance": (SF.A, "ONE launch of one thread, once per optimizer step", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_opt_step_dh": (SF.A, "ONE launch, no synchronisation, no allocation; n_cap == 0", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_opt_step_lean_dh": (SF.A, "ONE launch, no synchronisation, no allocation; n_cap == 0",
                               "test_chain_is_stream_ordered_without_a_sync"),
    "scone_grad_ctl_set_dh": (SF.A, "No call of this section synchronises or allocates; all are stream-ordered",
                              "test_chain_is_stream_ordered_without_a_sync"),
}


def test_every_entry_point_of_the_section_that_takes_a_stream_has_a_case():
    with open(HEADER) as f:
        text = f.read()
    section = text[text.index("/* ---- optimizer hyper-parameters on the device"):
                   text.index("/* ---- backward and optimizer step without a host synchronisation")]
    protos = re.findall(r"^(?:int|void)\s+(scone_\w+)\s*\(([^;{}]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", section, flags=re.S), flags=re.S | re.M)
    assert len(protos) == 6
    names = sorted(name for name, args in protos if re.search(r"\bstream\b", args))
    assert sorted(CONTRACT_DH) == names, (sorted(set(names) - set(CONTRACT_DH)), sorted(set(CONTRACT_DH) - set(names)))
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for name, (klass, sentence, where) in CONTRACT_DH.items():
        assert klass in (SF.A, SF.S) and callable(globals().get(where)), f"{name}: no case"
        assert sentence in flat, f"{name}: the header does not say {sentence!r}"


def test_chain_is_stream_ordered_without_a_sync():
    """scone_opt_hyper_init -> scone_grad_ctl_set_dh -> scone_opt_hyper_advance -> scone_opt_step_dh (SGD, INT8 table beside a
    master) -> scone_opt_step_lean_dh (a second table served by the same block, whose alpha = lr suits both: in place on fp32
    rows, row-wise Adagrad) as ONE chain on a side stream behind the delay kernel.  Class A throughout: the last call has returned while the delay still runs; afterwards
    block, control block, tables, master and state are those of the by-value calls on clones."""
    d, kind, t0 = 80, "sgd", 2
    hp = dict(lr=1e-3, weight_decay=0.01, grad_scale=0.5, eps=1e-8)
    _same_alpha(kind, hp["lr"], t0 + 1)
    rng, ids_buf, rows_buf = DN._opt_inputs(d, 5 * d)
    w = rng.standard_normal((N_OPT, d)).astype(np.float32)
    s = (rng.standard_normal(N_OPT) ** 2).astype(np.float32)
    ta, tb, ra, rb = (TO._table(fmt, d) for fmt in ("int8", "fp32", "int8", "fp32"))
    for x in (ta, tb, ra, rb):
        x.store_f32(torch.from_numpy(w))
    truth = rows_buf[:U_OPT].clone()
    g_in = SF.Input(truth, torch.roll(truth, 3, dims=0) * 2.0)
    term = SF.Input(_f64([9.0]), _f64([1.0e-4]))
    ids = ids_buf[:U_OPT].contiguous()
    n = _count(U_OPT)
    # the reference: the by-value road on clones
    W2, S2 = (torch.from_numpy(x).cuda() for x in (w, s))
    c2 = ra.grad_ctl([term.truth], grad_scale=hp["grad_scale"], max_norm=1.0, skip_nonfinite=True)
    assert 0 < float(c2.read()["coef"]) < 1
    ra.opt_step(ids, truth, W2, kind=kind, step=t0 + 1, ctl=c2, **hp)
    rb.opt_step_lean(ids, truth, kind="rowwise_adagrad", row_state=S2, ctl=c2, **hp)
    want_block = HF.advance(HF.init(hp["lr"], 0.9, 0.999, hp["eps"], hp["weight_decay"], hp["grad_scale"], 3, t0), kind)
    from scone_amd.hip_backend import GradCtl, OptHyper
    W, S = (torch.from_numpy(x).cuda() for x in (w, s))
    hy, ctl = OptHyper(ta.device), GradCtl(ta.device)
    state = {"table_a": SF.TableState(ta), "table_b": SF.TableState(tb), "master": SF.TensorState(W),
             "row_state": SF.TensorState(S)}

    def call():
        ta.opt_hyper(seed=3, step=t0, out=hy, **hp)
        ta.grad_ctl([term.buf], max_norm=1.0, skip_nonfinite=True, out=ctl, hyper=hy)
        ta.opt_hyper_advance(hy, kind, ctl)                        # one block serves both tables: advance once, step each
        ta.opt_step(ids, g_in.buf, W, kind=kind, ctl=ctl, n=n, hyper=hy)
        tb.opt_step_lean(ids, g_in.buf, kind="rowwise_adagrad", row_state=S, ctl=ctl, n=n, hyper=hy)
        return {}, None
    res = SF.run(call, [g_in, term], stream=SF.side_stream(ta), state=state, outputs={"hyper": hy.buf, "ctl": ctl.buf}, table=ta)
    SF.check_class(res, SF.A, "ctl_set_dh; advance; step_dh; step_lean_dh")
    got_block = _L().SconeOptHyper.from_buffer_copy(res.out["hyper"].tobytes())
    got_block = dict({k: getattr(got_block, k) for k in HF.INPUTS + ("seed", "step", "applied", "bad")},
                     sc={k: np.float32(getattr(got_block.sc, k)) for k in HF.FIELDS})
    assert HF.same_block(got_block, want_block), f"the block: {got_block} != {want_block} ({res.describe()})"
    assert res.out["ctl"].tobytes() == c2.buf.cpu().numpy().tobytes(), "the control block"
    for name, want in (("master", W2), ("row_state", S2)):
        assert E.same_bits(res.out[name], want.cpu().numpy()), f"{name}: {E.first_difference(res.out[name], want.cpu().numpy())}"
    assert not E.same_bits(res.out["master"], w) and not E.same_bits(res.out["row_state"], s), "the reference itself stepped"
    for name, ref in (("table_a", ra), ("table_b", rb)):
        want = SF.to_numpy(SF.TableState(ref).snapshot())
        assert E.same_bits(res.out[name], want), f"{name}: {E.first_difference(res.out[name], want)}"
    assert res.status == 0 and tb.status() == 0 and ra.status() == 0 and rb.status() == 0
