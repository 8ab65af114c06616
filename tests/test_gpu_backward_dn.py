"""The backward and the optimizer steps whose counts stay on the device (include/scone_hip.h, "backward and optimizer step without
a host synchronisation"): `BackwardContext`, the `n=` forms of `opt_step` / `opt_step_lean` / `grad_sqnorm`, and static mode of
the training modules.

Expectations.  Rows: tests/backward_fixture.py, through the helpers of tests/test_gpu_backward.py -- never the by-value road of
the library.  Optimizer steps and the norm: the contract is "the bits of the by-value call with n = min(*d_n, n_cap)", so the
by-value call on a clone IS the reference (its own bits are pinned by tests/test_gpu_opt_step.py, test_gpu_opt_lean.py and
test_gpu_grad_norm.py).  No tolerance anywhere: every comparison is of bits or bytes.

Buffers are U + 64 rows, pre-filled with NaN (row ids: -7); what lies behind the count must stay that.  The poison behind the
count is also what a kernel that ignored the device count would read: NaN rows and ids that raise SCONE_ST_BAD_ID."""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import opt_fixture as OF  # noqa: E402
import stream_fixture as SF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only: the batches, their id lists, gradients and expectations)
import test_gpu_opt_step as TO  # noqa: E402  (helpers only: small tables without an index)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, alphabet)

pytestmark = pytest.mark.gpu

GUARD = TB.GUARD


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


def _cur():
    return torch.cuda.current_stream().cuda_stream


def _ntok(batch, max_n):
    return len(TB._batch(batch, max_n)[0])


def _plan_dn(ctx, batch, max_n):
    tok, cu = TB._batch(batch, max_n)
    if batch in TB.RECTS:
        return ctx.plan(torch.from_numpy(tok.reshape(TB.RECTS[batch])))
    return ctx.plan(torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32)))


def _guarded(U, d, cap=None):
    cap = U + GUARD if cap is None else cap
    ids = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((cap, d), float("nan"), dtype=torch.float32, device="cuda")
    n = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    return ids, rows, n


def _rows_dn(ctx, U, g_t, reduce, d):
    """The GPU's answer out of guarded buffers: (row_ids, grad_rows) as numpy, with the count and the guard rows checked."""
    ids, rows, n = _guarded(U, d)
    got = ctx.rows(g_t.cuda(), reduce, out=(ids, rows, n))
    assert got[0] is ids and got[1] is rows and got[2] is n
    assert int(n.item()) == U, f"the count on the device is {int(n.item())}, the fixture has {U} rows"
    assert bool((ids[U:] == -7).all()) and bool(torch.isnan(rows[U:]).all()), "a guard row behind the output was written"
    return ids[:U].cpu().numpy(), rows[:U].cpu().numpy()


# ------------------------------------------------------------------ 1. rows: the cases of tests/test_gpu_backward.py
def _groups():
    """The cases of test_rows_equal_the_fixture, grouped by what one table and ONE context can serve: (max_n, mode, d).  Inside
    a group the largest batch comes first, so every smaller plan is built over the remains of a larger one."""
    groups = {}
    for p in TB._cases():
        batch, max_n, mode, reduce, dtype, d = p.values
        groups.setdefault((max_n, mode, d), []).append((batch, reduce, dtype))
    out = []
    for (max_n, mode, d), cases in sorted(groups.items()):
        cases.sort(key=lambda c: -_ntok(c[0], max_n))
        out.append(pytest.param(max_n, mode, d, tuple(cases), id=f"n{max_n}-{mode}-d{d}"))
    return out


def test_the_groups_hold_every_case_of_the_by_value_test():
    want = {p.values for p in TB._cases()}
    got = {(b, max_n, mode, r, t, d) for g in _groups() for max_n, mode, d, cases in [g.values] for b, r, t in cases}
    assert got == want and len(want) == len(TB._cases())
    for batch in ("r37", "r3", "r1", "tiny", "small"):
        for max_n in (3, 4):
            assert (batch, max_n, "cover", "mean", "fp16", 768) in want
    for d in (8, 200, 768, 4104):
        assert ("small", 4, "cover", "mean", "fp16", d) in want


@pytest.mark.parametrize("max_n,mode,d,cases", _groups())
def test_rows_equal_the_fixture(max_n, mode, d, cases):
    table = TB._table(max_n, d, mode)
    biggest = max(_ntok(b, max_n) for b, _, _ in cases)
    with table.backward_context(biggest) as ctx:
        assert ctx.nbytes > 0
        for batch, reduce, dtype in list(cases) + [cases[0]]:             # ... and the largest once more, after the smallest
            TB._assert_preconditions(batch, max_n, d)
            want = TB._want(batch, max_n, mode, reduce, d, dtype)
            off, _ = TB._lists(batch, max_n, mode)
            _plan_dn(ctx, batch, max_n)
            got = _rows_dn(ctx, len(want[0]), TB._grad(len(off) - 1, d, dtype), reduce, d)
            TB._check(got, want, f"{batch}-n{max_n}-{mode}-{reduce}-{dtype}-d{d}")
            assert ctx.counts() == (len(want[0]), int(off[-1]))
            assert table.status() == 0


def test_small_reaches_the_partials_path():
    lens = BW.row_lengths(*TB._lists("small", 4, "cover"))[1]
    assert lens.max() > TB._chunk() and (lens > TB._chunk()).sum() >= 2


# ------------------------------------------------------------------ 2. empty plans, overflow
def _table_bytes(t):
    rows, scales = t.download(t.row_begin, t.row_end - t.row_begin)
    return rows.view(np.uint8).copy(), None if scales is None else scales.view(np.uint8).copy()


def _same_table(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is b[1] or np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("case", ["0x5", "r1-longest_suffix", "r1-cover"])
def test_empty_plans(case):
    max_n, d = 3, 64
    mode = "longest_suffix" if case.endswith("longest_suffix") else "cover"
    table = TB._table(max_n, d, mode, fmt="fp32")
    w = np.random.default_rng(3).standard_normal((TB.N_ROWS[max_n], d)).astype(np.float32)
    table.store_f32(torch.from_numpy(w))
    master = torch.from_numpy(w).cuda()
    with table.backward_context(64) as ctx:
        if case == "0x5":
            ctx.plan(torch.zeros((0, 5), dtype=torch.int32))
            U, g = 0, torch.zeros((0, d), dtype=torch.float16)
            want = (np.zeros(0, dtype=np.int64), np.zeros((0, d), dtype=np.float32))
        else:
            _plan_dn(ctx, "r1", max_n)
            want = TB._want("r1", max_n, mode, "mean", d, "fp16")
            U, g = len(want[0]), TB._grad(50, d, "fp16")
            if mode == "longest_suffix":
                assert U == 0, "a sequence of one token has no f-gram of two: the plan with positions and no reference"
        got = _rows_dn(ctx, U, g, "mean", d)
        TB._check(got, want, case)
        assert ctx.counts()[0] == U
        if U == 0:                                               # steps behind an empty plan change nothing
            ids, rows, n = _guarded(0, d)
            ctx.rows(g.cuda(), "mean", out=(ids, rows, n))
            before = _table_bytes(table)
            table.opt_step(ids, rows, master, kind="sgd", lr=0.5, n=n)
            table.opt_step_lean(ids, rows, kind="sgd", lr=0.5, n=n)
            sq, _ = table.grad_sqnorm(rows, n=n)
            assert float(sq.item()) == 0.0 and not np.signbit(sq.item())
            assert E.same_bits(master.cpu().numpy(), w) and _same_table(_table_bytes(table), before)
    assert table.status() == 0


def test_overflow_writes_nothing_and_the_step_behind_it_changes_nothing():
    L = _L()
    max_n, d, batch = 3, 64, "r37"
    want = TB._want(batch, max_n, "cover", "mean", d, "fp16")
    U = len(want[0])
    table = TB._table(max_n, d, fmt="int8")
    w = np.random.default_rng(3).standard_normal((TB.N_ROWS[max_n], d)).astype(np.float32)
    table.store_f32(torch.from_numpy(w))
    master, state2 = torch.from_numpy(w).cuda(), torch.ones((TB.N_ROWS[max_n], d), device="cuda")
    before = _table_bytes(table)
    g = TB._grad(_ntok(batch, max_n), d, "fp16").cuda()
    with table.backward_context(_ntok(batch, max_n)) as ctx:
        _plan_dn(ctx, batch, max_n)
        ids, rows, n = _guarded(U, d, cap=U - 1)
        ctx.rows(g, "mean", out=(ids, rows, n))
        table.opt_step(ids, rows, master, kind="adagrad", lr=0.5, state2=state2, n=n)
        assert int(n.item()) == 0
        assert bool((ids == -7).all()) and bool(torch.isnan(rows).all()), "an overflowing call wrote into the arrays"
        assert table.status() == L.ST_ROWS_OVERFLOW and table.status() == 0, "bit 4 is raised, and cleared by the read"
        assert E.same_bits(master.cpu().numpy(), w) and bool((state2 == 1).all()) and _same_table(_table_bytes(table), before)
        ctx.rows(g, "mean", out=(ids, rows, n))
        assert table.rows_overflowed() and not table.rows_overflowed()
        # the same plan fits buffers of U rows exactly
        ids, rows, n = _guarded(U, d, cap=U)
        ctx.rows(g, "mean", out=(ids, rows, n))
        assert int(n.item()) == U
        TB._check((ids.cpu().numpy(), rows.cpu().numpy()), want, "cap == U")
    assert table.status() == 0


# ------------------------------------------------------------------ 3. optimizer steps: the by-value call on a clone
N_OPT, U_OPT = TO.N, 120
CTLS = ("plain", "coef", "skip")


def _opt_inputs(d, seed):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(N_OPT, size=U_OPT, replace=False)).astype(np.int64)
    g = rng.standard_normal((U_OPT, d)).astype(np.float32)
    ids_buf = torch.cat([torch.from_numpy(ids), torch.full((GUARD,), -7, dtype=torch.int64)]).cuda()
    rows_buf = torch.cat([torch.from_numpy(g), torch.full((GUARD, d), float("nan"))]).cuda()
    return rng, ids_buf, rows_buf


def _ctl_of(table, which):
    if which == "plain":
        return None
    if which == "coef":
        ctl = table.grad_ctl([torch.tensor(9.0, dtype=torch.float64, device="cuda")], grad_scale=0.5, max_norm=1.0)
        assert 0 < float(ctl.read()["coef"]) < 1
        return ctl
    ctl = table.grad_ctl([float("inf")], skip_nonfinite=True)
    assert ctl.read()["skip"] == 1
    return ctl


@pytest.mark.parametrize("which", CTLS)
@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("fmt,d", [("int8", 80), ("fp32", 8)])
def test_opt_step_dn_equals_the_by_value_call(fmt, d, kind, which):
    rng, ids_buf, rows_buf = _opt_inputs(d, 7 * d)
    w = rng.standard_normal((N_OPT, d)).astype(np.float32)
    m, v = (0.1 * rng.standard_normal((N_OPT, d))).astype(np.float32), (rng.standard_normal((N_OPT, d)) ** 2).astype(np.float32)
    hp = dict(kind=kind, lr=0.05, step=3, weight_decay=0.01, grad_scale=0.5)
    ends = []
    for road in ("value", "dn", "dn-above-cap"):
        t = TO._table(fmt, d)
        t.store_f32(torch.from_numpy(w))
        W, M, V = (torch.from_numpy(x).cuda() for x in (w, m, v))
        ctl = _ctl_of(t, which)
        if road == "value":
            t.opt_step(ids_buf[:U_OPT], rows_buf[:U_OPT], W, state1=M, state2=V, ctl=ctl, **hp)
        elif road == "dn":
            t.opt_step(ids_buf, rows_buf, W, state1=M, state2=V, ctl=ctl, n=torch.tensor([U_OPT], device="cuda"), **hp)
        else:                                                    # n = min(*d_n, n_cap): a count above the capacity is the capacity
            t.opt_step(ids_buf[:U_OPT], rows_buf[:U_OPT], W, state1=M, state2=V, ctl=ctl,
                       n=torch.tensor([U_OPT + 1000], device="cuda"), **hp)
        assert t.status() == 0, f"{road}: a row behind the count was read"
        ends.append((road, [x.cpu().numpy() for x in (W, M, V)], _table_bytes(t)))
    ref = ends[0]
    changed = not E.same_bits(ref[1][0], w)
    assert changed == (which != "skip"), "the reference itself: a skipped step changes nothing, any other changes the master"
    for road, arrays, tb in ends[1:]:
        for name, got, want in zip(("master", "state1", "state2"), arrays, ref[1]):
            assert E.same_bits(got, want), f"{road}: {name}: {E.first_difference(got, want)}"
        assert _same_table(tb, ref[2]), f"{road}: the served rows or scales differ"


LEAN_MODES = {"master-int8": ("int8", True, "nearest"), "inplace-bf16": ("bf16", False, "nearest"),
              "inplace-bf16-stochastic": ("bf16", False, "stochastic")}


@pytest.mark.parametrize("which", CTLS)
@pytest.mark.parametrize("kind", ["sgd", "rowwise_adagrad"])
@pytest.mark.parametrize("mode", list(LEAN_MODES))
def test_opt_step_lean_dn_equals_the_by_value_call(mode, kind, which):
    fmt, with_master, rounding = LEAN_MODES[mode]
    d = 80 if fmt == "int8" else 72
    rng, ids_buf, rows_buf = _opt_inputs(d, 11 * d)
    w = rng.standard_normal((N_OPT, d)).astype(np.float32)
    s = (rng.standard_normal(N_OPT) ** 2).astype(np.float32)
    hp = dict(kind=kind, lr=0.05, weight_decay=0.01, grad_scale=0.5, rounding=rounding, seed=13, step=4)
    ends = []
    for road in ("value", "dn"):
        t = TO._table(fmt, d)
        t.store_f32(torch.from_numpy(w))
        W = torch.from_numpy(w).cuda() if with_master else None
        S = torch.from_numpy(s).cuda()
        ctl = _ctl_of(t, which)
        if road == "value":
            t.opt_step_lean(ids_buf[:U_OPT], rows_buf[:U_OPT], master=W, row_state=S, ctl=ctl, **hp)
        else:
            t.opt_step_lean(ids_buf, rows_buf, master=W, row_state=S, ctl=ctl, n=torch.tensor([U_OPT], device="cuda"), **hp)
        assert t.status() == 0, f"{road}: a row behind the count was read"
        ends.append(([None if W is None else W.cpu().numpy(), S.cpu().numpy()], _table_bytes(t)))
    (ref, ref_tb), (got, got_tb) = ends
    if with_master:
        assert E.same_bits(got[0], ref[0]), f"master: {E.first_difference(got[0], ref[0])}"
        assert E.same_bits(ref[0], w) == (which == "skip")
    assert E.same_bits(got[1], ref[1]), "row_state"
    assert _same_table(got_tb, ref_tb), "the served rows or scales differ"


# ------------------------------------------------------------------ 4. the squared norm
@pytest.mark.parametrize("extra", [0, 2000])
@pytest.mark.parametrize("n", [0, 1, 1023, 1025])
def test_grad_sqnorm_dn_equals_the_by_value_call(n, extra):
    d = 72
    g = TB._g32(TB._grad(1025, d, "fp32"))
    t = TO._table("fp32", d)
    rows = torch.from_numpy(g[:n]).cuda()
    buf = torch.cat([rows, torch.full((extra, d), float("nan"), device="cuda")])     # a row behind the count would make it NaN
    sq_v, q_v = t.grad_sqnorm(rows)
    sq_buf = torch.full((), -1.0, dtype=torch.float64, device="cuda")
    sq_d, q_d = t.grad_sqnorm(buf, n=torch.tensor([n], device="cuda"), out=sq_buf)
    assert sq_d is sq_buf
    a, b = sq_v.cpu().numpy().view(np.int64), sq_d.cpu().numpy().view(np.int64)
    assert a == b, f"n = {n}, n_cap = {n + extra}: {sq_v.item()!r} by value, {sq_d.item()!r} with the count on the device"
    assert np.array_equal(q_v.cpu().numpy().view(np.int64), q_d[:n].cpu().numpy().view(np.int64)), "Q_r"
    if n:
        assert sq_v.item() > 0
    assert t.status() == 0


# ------------------------------------------------------------------ 5. refusals
def test_refusals_of_the_library():
    L = _L()
    lib = L.lib()
    max_n, d = 3, 64
    t, other = TB._table(max_n, d), TB._table(max_n, d)
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(TB.RECTS["r37"])).to("cuda", torch.int32)
    ctx = t.backward_context(10)
    g = torch.zeros((tok.numel(), d), dtype=torch.float16, device="cuda")
    ids, rows, n = _guarded(0, d)
    err = lambda h=t: lib.scone_last_error(h._h).decode()  # noqa: E731
    # more positions than the context holds
    assert lib.scone_backward_plan_dn(t._h, ctx._c, _ptr(tok), 9, 37, None) == L.ERANGE and "max_tokens" in err()
    with pytest.raises(IndexError):
        ctx.plan(tok)
    cu = torch.tensor([0, 333], dtype=torch.int32, device="cuda")
    assert lib.scone_backward_plan_varlen_dn(t._h, ctx._c, _ptr(tok), _ptr(cu), 1, 333, None) == L.ERANGE
    # a context of another handle, null pointers, bad enums
    assert lib.scone_backward_plan_dn(other._h, ctx._c, _ptr(tok), 1, 5, None) == L.EINVAL and "another handle" in err(other)
    assert lib.scone_backward_rows_dn(other._h, ctx._c, _ptr(g), L.DT_F16, L.REDUCE_MEAN, _ptr(ids), _ptr(rows), GUARD, _ptr(n),
                                      None) == L.EINVAL and "another handle" in err(other)
    assert lib.scone_backward_plan_dn(t._h, None, _ptr(tok), 1, 5, None) == L.EINVAL and "null ctx" in err()
    assert lib.scone_backward_plan_dn(t._h, ctx._c, None, 1, 5, None) == L.EINVAL and "null d_tok" in err()
    assert lib.scone_backward_plan_dn(t._h, ctx._c, _ptr(tok), -1, 5, None) == L.EINVAL
    assert lib.scone_backward_plan_varlen_dn(t._h, ctx._c, _ptr(tok), None, 1, 5, None) == L.EINVAL and "null pointer" in err()
    assert lib.scone_backward_plan_varlen_dn(t._h, ctx._c, _ptr(tok), _ptr(cu), -1, 5, None) == L.EINVAL
    assert lib.scone_backward_plan_dn(t._h, ctx._c, _ptr(tok), 2, 5, None) == 0
    assert lib.scone_backward_rows_dn(t._h, ctx._c, _ptr(g), L.DT_F16, L.REDUCE_MEAN, _ptr(ids), _ptr(rows), GUARD, None,
                                      None) == L.EINVAL and "null d_n_out" in err()
    assert lib.scone_backward_rows_dn(t._h, ctx._c, None, L.DT_F16, L.REDUCE_MEAN, _ptr(ids), _ptr(rows), GUARD, _ptr(n),
                                      None) == L.EINVAL and "null pointer" in err()
    assert lib.scone_backward_rows_dn(t._h, ctx._c, _ptr(g), L.DT_F16, L.REDUCE_MEAN, None, _ptr(rows), GUARD, _ptr(n),
                                      None) == L.EINVAL
    assert lib.scone_backward_rows_dn(t._h, ctx._c, _ptr(g), 7, L.REDUCE_MEAN, _ptr(ids), _ptr(rows), GUARD, _ptr(n), None) == L.EINVAL
    assert lib.scone_backward_rows_dn(t._h, ctx._c, _ptr(g), L.DT_F16, 9, _ptr(ids), _ptr(rows), GUARD, _ptr(n), None) == L.EINVAL
    torch.cuda.synchronize()
    assert int(n.item()) == -5 and bool((ids == -7).all()) and bool(torch.isnan(rows).all()), "a refused call wrote"
    # the steps and the norm: a null count
    W = torch.zeros((TB.N_ROWS[max_n], d), device="cuda")
    cfg = L.OptCfg(C.sizeof(L.OptCfg), L.OPT_SGD, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1)
    assert lib.scone_opt_step_dn(t._h, C.byref(cfg), _ptr(ids), _ptr(rows), None, GUARD, _ptr(W), None, None, None, None) == L.EINVAL
    assert "null d_n" in err()
    lean = L.LeanCfg(C.sizeof(L.LeanCfg), L.LEAN_SGD, L.ROUND_NEAREST, 0, 0.1, 1e-10, 0.0, 1.0, 0, 1)
    assert lib.scone_opt_step_lean_dn(t._h, C.byref(lean), _ptr(ids), _ptr(rows), None, GUARD, None, None, None, None) == L.EINVAL
    assert "null d_n" in err()
    sq = torch.zeros((), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(L.grad_sqnorm_scratch(GUARD), dtype=torch.float64, device="cuda")
    assert lib.scone_grad_sqnorm_dn(t._h, _ptr(rows), None, GUARD, _ptr(scratch), _ptr(sq), None) == L.EINVAL and "null d_n" in err()
    assert lib.scone_grad_sqnorm_dn(t._h, _ptr(rows), _ptr(n), GUARD, None, _ptr(sq), None) == L.EINVAL
    # creation
    out = C.c_void_p()
    assert lib.scone_backward_ctx_create(t._h, -1, C.byref(out)) == L.EINVAL and "negative max_tokens" in err()
    assert lib.scone_backward_ctx_create(t._h, 1 << 31, C.byref(out)) == L.EINVAL and "too many tokens" in err()
    assert lib.scone_backward_ctx_create(t._h, 8, None) == L.EINVAL
    with pytest.raises(ValueError, match="d % 8"):
        TB._table(max_n, 12).backward_context(8)
    ctx.close()
    ctx.close()
    assert t.status() == 0 and other.status() == 0


def test_a_plan_above_the_merge_sort_limit_is_not_captured():
    """Above 2^20 possible references the plan's sort runs kernels with a private segment; scone_backward_plan_dn refuses a
    capturing stream then (ValueError, nothing enqueued), serves the same batch eagerly, and captures a smaller batch in the
    same context."""
    max_n, d = 3, 64
    t = TB._table(max_n, d)
    ntok = (1 << 20) // 6 + 8
    assert ntok * 6 > 1 << 20
    rng = np.random.default_rng(5)
    tok = torch.from_numpy(rng.choice(WS.VOCAB + 1, size=(1, ntok), p=WS.TOKEN_P).astype(np.int32)).cuda()
    small = tok[:, :512].contiguous()
    with t.backward_plan(tok) as p_big, t.backward_plan(small) as p_small:
        want_big, want_small = (p_big.n_rows, p_big.n_refs), (p_small.n_rows, p_small.n_refs)
    assert 0 < want_small[1] < want_big[1]
    ctx = t.backward_context(ntok)
    assert ctx.plan(tok).counts() == want_big, "eagerly the large plan is served"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(ValueError, match="not captured"):
            ctx.plan(tok)
        ctx.plan(small)
    g.replay()
    assert ctx.counts() == want_small, "the refused call left something behind, or the smaller plan was not captured"
    ctx.close()
    assert t.status() == 0


def _static_modules(max_n=3, d=64):
    from scone_amd import InPlaceFGramTable, TrainableFGramTable
    w = np.random.default_rng(31).standard_normal((TB.N_ROWS[max_n], d)).astype(np.float32)
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T)).to("cuda", torch.int32)
    cap = TB.N_ROWS[max_n]
    tr = TrainableFGramTable(TB._cache("int8", d, max_n, "cover", torch.from_numpy(w)), torch.from_numpy(w.copy()), static_rows=cap,
                             max_tokens=B * T)
    ip = InPlaceFGramTable(TB._cache("bf16", d, max_n, "cover", torch.from_numpy(w)), static_rows=cap, max_tokens=B * T)
    return tr, ip, tok


def test_refusals_of_the_python_layer():
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    tr, ip, tok = _static_modules()
    with pytest.raises(ValueError, match="max_tokens"):
        TrainableFGramTable(tr.cache, tr.weight, static_rows=10)
    with pytest.raises(ValueError, match="static_rows"):
        InPlaceFGramTable(ip.cache, static_rows=0, max_tokens=10)
    with pytest.raises(ValueError, match="fused_backward"):
        FGramOptimizer(ip, "sgd", fused_backward=True)
    # accumulation: a second backward onto a gradient that is there
    for fg in (tr, ip):
        before = _table_bytes(fg.cache.to_device())
        fg(tok).sum().backward()
        assert fg.static_grad is not None and getattr(fg, "grad", None) is None
        with pytest.raises(ValueError, match="accumulation"):
            fg(tok).sum().backward()
        assert _same_table(_table_bytes(fg.cache.to_device()), before)
    # under capture: Adam and stochastic rounding
    adam = FGramOptimizer(tr, "adam", lr=0.01)
    adam.step()                                                  # eagerly it works, and the state exists
    stoch = FGramOptimizer(ip, "sgd", lr=0.01, rounding="stochastic", seed=3)
    stoch.step()
    cold = FGramOptimizer(ip, "rowwise_adagrad", lr=0.01)        # no warm-up: its state would be allocated inside the capture
    torch.cuda.synchronize()
    states = [_table_bytes(fg.cache.to_device()) for fg in (tr, ip)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(ValueError, match="Adam"):
            adam.step()
        with pytest.raises(ValueError, match="stochastic"):
            stoch.step()
        with pytest.raises(ValueError, match="warm-up"):
            cold.step()
    torch.cuda.synchronize()
    assert adam.t == 1 and stoch.t == 1 and cold.t == 0
    assert all(_same_table(_table_bytes(fg.cache.to_device()), s) for fg, s in zip((tr, ip), states)), "a refused step did device work"
    adam.zero_grad()
    assert tr.static_grad is None
    tr(tok).sum().backward()                                     # after zero_grad the next backward is a first one
    assert tr.cache.to_device().status() == 0 and ip.cache.to_device().status() == 0


# ------------------------------------------------------------------ 6. stream order
# The stream contract of this section, kept here: (class, the header's sentence, the test that holds the case).  The table of
# tests/test_gpu_stream_order.py lists the prototypes that spell their stream `scone_stream_t`; the prototypes of this section
# spell it `void *stream` (the same type), and test_every_entry_point_of_the_section_that_takes_a_stream_has_a_case keeps THIS
# table equal to them.
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scone_hip.h")
_A = "No synchronisation, no allocation"
CONTRACT_DN = {
    "scone_backward_plan_dn": (SF.A, _A + ", no free; the counts ... stay on the device", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_backward_plan_varlen_dn": (SF.A, _A + ", no free; the counts ... stay on the device", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_backward_rows_dn": (SF.A, "No synchronisation, no allocation", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_opt_step_dn": (SF.A, "ONE launch ..., no synchronisation, no allocation", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_opt_step_lean_dn": (SF.A, "ONE launch ..., no synchronisation, no allocation", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_grad_sqnorm_dn": (SF.A, "Three launches, no synchronisation, no allocation", "test_chain_is_stream_ordered_without_a_sync"),
    "scone_backward_ctx_counts": (SF.S, "the synchronising read of U and the reference count", "test_ctx_counts_synchronises_its_stream"),
}


def test_every_entry_point_of_the_section_that_takes_a_stream_has_a_case():
    import re
    with open(HEADER) as f:
        text = f.read()
    section = text[text.index("typedef struct scone_bwd_ctx scone_bwd_ctx;"):text.index("the fused lookup at CHOSEN positions only")]
    protos = re.findall(r"^(?:int|void)\s+(scone_\w+)\s*\(([^;{}]*?)\)\s*;", section, flags=re.S | re.M)
    assert len(protos) == 11
    names = sorted(name for name, args in protos if re.search(r"\bstream\b", args))
    assert sorted(CONTRACT_DN) == names, (sorted(set(names) - set(CONTRACT_DN)), sorted(set(CONTRACT_DN) - set(names)))
    for name, (klass, sentence, where) in CONTRACT_DN.items():
        assert klass in (SF.A, SF.S) and sentence and callable(globals().get(where)), f"{name}: no case"
        assert sentence.replace(" ...", "").split(";")[0].split(",")[0] in text, f"{name}: the header does not say so"


def _other_cu(rng, cu):
    """Other boundaries of the same packed stream: monotone, the same first and last entry."""
    out = cu.copy()
    for _ in range(8):
        out[1:-1] = np.sort(rng.integers(0, cu[-1] + 1, size=len(cu) - 2))
        if not np.array_equal(out, cu):
            return out
    raise AssertionError("no other boundaries found")


CHAINS = {"packed-opt_step": ("small", 4), "rect-sqnorm-opt_step_lean": ("r37", 3)}


def _chain_inputs(form):
    batch, max_n = CHAINS[form]
    d = 64
    t = TB._table(max_n, d, fmt="fp32")
    tok, cu = TB._batch(batch, max_n)
    rng = np.random.default_rng(len(tok))
    if batch in TB.RECTS:
        B, T = TB.RECTS[batch]
        x = SF.Input(tok.reshape(B, T).astype(np.int32), np.roll(tok, 5).reshape(B, T).astype(np.int32))
        inputs, plan = [x], lambda ctx: ctx.plan(x.buf)
    else:
        x, c = SF.Input(tok.astype(np.int32), np.roll(tok, 5).astype(np.int32)), SF.Input(cu.astype(np.int32), _other_cu(rng, cu).astype(np.int32))
        inputs, plan = [x, c], lambda ctx: ctx.plan(x.buf, c.buf)
    w0 = rng.standard_normal((TB.N_ROWS[max_n], d)).astype(np.float32)
    t.store_f32(torch.from_numpy(w0))
    return batch, max_n, d, t, inputs, plan, w0, rng


@pytest.mark.parametrize("form", list(CHAINS))
def test_chain_is_stream_ordered_without_a_sync(form):
    """scone_backward_plan_varlen_dn -> scone_backward_rows_dn -> scone_opt_step_dn (packed; rows of several chunks, so all three
    launches of rows_dn) and scone_backward_plan_dn -> scone_backward_rows_dn -> scone_grad_sqnorm_dn -> scone_opt_step_lean_dn
    (rectangle; in place on fp32 rows, row-wise Adagrad), each as ONE chain on a side stream behind the delay kernel.  Class A
    throughout: the last call has returned while the delay still runs; afterwards the rows are the fixture's and the weights
    the fixture's step on them."""
    import lean_fixture as LF
    from scone_amd.hip_backend import lean_scalars, opt_scalars
    batch, max_n, d, t, inputs, plan, w0, rng = _chain_inputs(form)
    n_rows = TB.N_ROWS[max_n]
    if batch == "small":
        assert BW.row_lengths(*TB._lists(batch, max_n, "cover"))[1].max() > TB._chunk()
    g = TB._grad(len(TB._batch(batch, max_n)[0]), d, "fp16")
    g_in = SF.Input(g, TB._grad(g.shape[0], d, "fp16", seed=9))
    want_ids, want_rows = TB._want(batch, max_n, "cover", "mean", d, "fp16")
    U = len(want_ids)
    ctx = t.backward_context(g.shape[0])
    ids, rows, n = _guarded(U, d)
    hp = dict(lr=0.05, weight_decay=0.01)
    state, outputs = {"table": SF.TableState(t)}, {"ids": ids, "rows": rows, "n": n}
    if form.startswith("packed"):
        master = torch.from_numpy(w0).cuda()
        state["master"] = SF.TensorState(master)
        want_w = OF.apply("sgd", opt_scalars("sgd", **hp), want_ids, want_rows, w0, None, None, 0, n_rows)[0]

        def call():
            plan(ctx)
            ctx.rows(g_in.buf, "mean", out=(ids, rows, n))
            t.opt_step(ids, rows, master, kind="sgd", n=n, **hp)
            return {}, None
    else:
        s0 = (rng.standard_normal(n_rows) ** 2).astype(np.float32)
        row_state = torch.from_numpy(s0).cuda()
        state["row_state"] = SF.TensorState(row_state)
        sq = torch.zeros((), dtype=torch.float64, device="cuda")
        scratch = torch.zeros(_L().grad_sqnorm_scratch(U + GUARD), dtype=torch.float64, device="cuda")
        outputs["sq"] = sq
        want_w, want_s, _, _ = LF.apply("rowwise_adagrad", lean_scalars("rowwise_adagrad", eps=1e-10, **hp), want_ids, want_rows, w0, s0)
        want_sq = t.grad_sqnorm(torch.from_numpy(want_rows).cuda())[0].cpu().numpy()     # the by-value call on the fixture's rows

        def call():
            plan(ctx)
            ctx.rows(g_in.buf, "mean", out=(ids, rows, n))
            t.grad_sqnorm(rows, scratch, n=n, out=sq)
            t.opt_step_lean(ids, rows, kind="rowwise_adagrad", row_state=row_state, eps=1e-10, n=n, **hp)
            return {}, None
    res = SF.run(call, inputs + [g_in], stream=SF.side_stream(t), state=state, outputs=outputs, table=t)
    SF.check_class(res, SF.A, form)
    assert res.out["n"].tolist() == [U], f"{form}: the count ({res.describe()})"
    assert np.array_equal(res.out["ids"][:U], want_ids) and (res.out["ids"][U:] == -1).all(), f"{form}: row ids"
    assert E.same_bits(res.out["rows"][:U], want_rows), f"{form}: rows: {E.first_difference(res.out['rows'][:U], want_rows)}"
    assert np.isnan(res.out["rows"][U:]).all(), f"{form}: a guard row was written"
    assert E.same_bits(res.out["table"], want_w), f"{form}: the served table: {E.first_difference(res.out['table'], want_w)}"
    if form.startswith("packed"):
        assert E.same_bits(res.out["master"], want_w), f"{form}: master"
    else:
        assert E.same_bits(res.out["row_state"], want_s), f"{form}: row state"
        assert res.out["sq"].view(np.int64) == want_sq.view(np.int64), f"{form}: the squared norm"
    assert res.status == 0
    ctx.close()


def test_ctx_counts_synchronises_its_stream():
    """scone_backward_ctx_counts (S): the counts of the plan enqueued in front of it on the same stream."""
    batch, max_n, d, t, inputs, plan, _, _ = _chain_inputs("packed-opt_step")
    off, ids_l = TB._lists(batch, max_n, "cover")
    U = len(TB._want(batch, max_n, "cover", "mean", d, "fp16")[0])
    refs = len(BW.references(off, ids_l, 0, None, TB.N_ROWS[max_n])[0])
    ctx = t.backward_context(len(off) - 1)

    def call():
        plan(ctx)
        return {}, ctx.counts()
    res = SF.run(call, inputs, stream=SF.side_stream(t), table=t)
    SF.check_class(res, SF.S, "scone_backward_ctx_counts")
    assert res.host == (U, refs), f"counts {res.host}, the fixture has {(U, refs)} ({res.describe()})"
    assert res.status == 0
    ctx.close()


# ------------------------------------------------------------------ 7. capture and replay
CAP_B, CAP_T, CAP_D, CAP_N = 8, 64, 768, 3


def _capture_batches(k=4):
    rng = np.random.default_rng(2024)
    toks = [rng.choice(WS.VOCAB + 1, size=(CAP_B, CAP_T), p=WS.TOKEN_P).astype(np.int32) for _ in range(k)]
    grads = [TB._grad(CAP_B * CAP_T, CAP_D, "fp16", seed=20 + i) for i in range(k)]
    return toks, grads


def _capture(fn, what):
    """Warm up on a side stream as torch requires, then capture fn() on one stream: a linear graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(warm_up=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            fn(warm_up=False)
    except RuntimeError as e:
        pytest.fail(f"{what}: the capture failed -- a hidden synchronisation or allocation inside the chain: {e}")
    return g


CAPTURE_CASES = {"int8-master-sgd": ("int8", True, "sgd"), "bf16-inplace-rowwise_adagrad": ("bf16", False, "rowwise_adagrad")}


def _twin_tables(fmt, seed=41):
    w0 = np.random.default_rng(seed).standard_normal((TB.N_ROWS[CAP_N], CAP_D)).astype(np.float32)
    return w0, [TB._cache(fmt, CAP_D, CAP_N, "cover", torch.from_numpy(w0)) for _ in range(2)]


@pytest.mark.parametrize("case", list(CAPTURE_CASES))
def test_capture_and_replay_of_the_entry_points(case):
    """plan_dn; rows_dn; sqnorm_dn; ctl_set; opt_step*_dn captured once and replayed on three other batches: table, master and
    state equal an eager twin stepped with the by-value road (backward_plan, rows, grad_sqnorm, grad_ctl, opt_step*_ctl)."""
    fmt, with_master, kind = CAPTURE_CASES[case]
    w0, (cache, twin_cache) = _twin_tables(fmt)
    t, twin = cache.to_device(), twin_cache.to_device()
    n_rows = TB.N_ROWS[CAP_N]
    toks, grads = _capture_batches()
    tok_s = torch.from_numpy(toks[0]).cuda()
    g_s = grads[0].cuda()
    masters = [torch.from_numpy(w0).cuda() if with_master else None for _ in range(2)]
    states = [torch.zeros(n_rows, device="cuda") if kind == "rowwise_adagrad" else None for _ in range(2)]
    ctx = t.backward_context(CAP_B * CAP_T)
    ids, rows, n = _guarded(n_rows, CAP_D, cap=n_rows)
    from scone_amd.hip_backend import GradCtl
    sq = torch.zeros((), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_L().grad_sqnorm_scratch(n_rows), dtype=torch.float64, device="cuda")
    ctl = GradCtl(t.device)
    hp = dict(lr=0.05, weight_decay=0.01)

    def step(table, i_, r_, master, state, c_, n_=None):
        if kind == "sgd":
            table.opt_step(i_, r_, master, kind="sgd", ctl=c_, n=n_, **hp)
        else:
            table.opt_step_lean(i_, r_, kind=kind, master=master, row_state=state, ctl=c_, n=n_, **hp)

    def chain(warm_up):
        ctx.plan(tok_s)
        ctx.rows(g_s, "mean", out=(ids, rows, n))
        t.grad_sqnorm(rows, scratch, n=n, out=sq)
        t.grad_ctl([sq], max_norm=1.0, skip_nonfinite=True, out=ctl)
        step(t, ids, rows, masters[0], states[0], ctl, n)

    def eager(i):
        with twin.backward_plan(torch.from_numpy(toks[i])) as plan:
            r_ids, r_rows = plan.rows(grads[i].cuda(), "mean")
            c2 = twin.grad_ctl([twin.grad_sqnorm(r_rows)[0]], max_norm=1.0, skip_nonfinite=True)
            step(twin, r_ids, r_rows, masters[1], states[1], c2)
            return plan.n_rows, c2.read()

    def compare(tag, U, c2):
        torch.cuda.synchronize()
        assert int(n.item()) == U, f"{tag}: the count"
        got = ctl.read()
        assert got["coef"].view(np.uint32) == c2["coef"].view(np.uint32) and 0 < float(got["coef"]) < 1 and got["skip"] == 0, f"{tag}: ctl"
        assert np.float64(got["sqnorm"]).view(np.int64) == np.float64(c2["sqnorm"]).view(np.int64), f"{tag}: the squared norm"
        assert _same_table(_table_bytes(t), _table_bytes(twin)), f"{tag}: the served table differs from the eager twin's"
        if with_master:
            assert E.same_bits(masters[0].cpu().numpy(), masters[1].cpu().numpy()), f"{tag}: master"
        if states[0] is not None:
            assert E.same_bits(states[0].cpu().numpy(), states[1].cpu().numpy()), f"{tag}: row state"

    g = _capture(chain, case)
    compare("warm-up", *eager(0))                                  # the warm-up ran once, eagerly, on batch 0
    start = _table_bytes(t)
    for i in (1, 2, 3):
        tok_s.copy_(torch.from_numpy(toks[i]))
        g_s.copy_(grads[i])
        g.replay()
        compare(f"replay {i}", *eager(i))
    assert not _same_table(_table_bytes(t), start), "three replays left the table as it was"
    assert t.status() == 0 and twin.status() == 0
    ctx.close()


@pytest.mark.parametrize("case", list(CAPTURE_CASES))
def test_capture_and_replay_of_the_module_layer(case):
    """fg(ids).sum().backward(); opt.step(max_norm=) captured with static_rows=, replayed on three other batches, against the
    same loop run eagerly on a twin built without static_rows= (the by-value road)."""
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    fmt, with_master, kind = CAPTURE_CASES[case]
    w0, caches = _twin_tables(fmt, seed=43)
    n_rows = TB.N_ROWS[CAP_N]
    toks, _ = _capture_batches()
    kw = dict(static_rows=n_rows, max_tokens=CAP_B * CAP_T)
    if with_master:
        fg = TrainableFGramTable(caches[0], torch.from_numpy(w0.copy()), **kw)
        fg2 = TrainableFGramTable(caches[1], torch.from_numpy(w0.copy()))
    else:
        fg, fg2 = InPlaceFGramTable(caches[0], **kw), InPlaceFGramTable(caches[1])
    opt, opt2 = (FGramOptimizer(m, kind, lr=0.05, weight_decay=0.01) for m in (fg, fg2))
    tok_s = torch.from_numpy(toks[0]).cuda()

    def loop(warm_up):
        fg(tok_s).sum().backward()
        opt.step(max_norm=1.0)
        if warm_up:
            opt.zero_grad()

    def eager(i):
        fg2(torch.from_numpy(toks[i]).cuda()).sum().backward()
        rows = opt2.step(max_norm=1.0)
        opt2.zero_grad()
        return rows

    def compare(tag, U):
        torch.cuda.synchronize()
        assert int(fg.static_grad[2].item()) == U, f"{tag}: the count"
        assert opt.last_ctl.read() == opt2.last_ctl.read() and not opt.found_nonfinite(), f"{tag}: last_ctl"
        assert _same_table(_table_bytes(caches[0].to_device()), _table_bytes(caches[1].to_device())), f"{tag}: the served table"
        if with_master:
            assert E.same_bits(fg.weight.detach().cpu().numpy(), fg2.weight.detach().cpu().numpy()), f"{tag}: weight"
        if opt.state2 is not None:
            assert E.same_bits(opt.state2.cpu().numpy(), opt2.state2.cpu().numpy()), f"{tag}: state"

    g = _capture(loop, case)
    assert fg.static_grad is not None
    compare("warm-up", eager(0))
    for i in (1, 2, 3):
        tok_s.copy_(torch.from_numpy(toks[i]))
        g.replay()
        compare(f"replay {i}", eager(i))
    assert not opt.rows_overflowed()
    assert caches[1].to_device().status() == 0
