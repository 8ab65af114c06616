"""`scone_grad_sqnorm`, `scone_grad_ctl_set`, `scone_opt_step_ctl` and `scone_opt_step_lean_ctl` (include/scone_hip.h, "gradient
norm, clipping and skipped steps") against tests/grad_norm_fixture.py and against the plain optimizer steps.

The contract fixes the order of every sum and every rounding, so nothing here has a tolerance: the total, every row sum Q_r and
every tile sum P_k equal the fixture's float64 bits; the five fields of the control block equal the fixture's; a `_ctl` step
leaves the bytes the plain step leaves when given the product `fp32(grad_scale) * coef` as its `grad_scale`.
tests/test_grad_norm_host.py shows that the fixture's total of the value mix used here depends on the order of the sums.

Shapes.  d = 8: two of 64 lanes hold elements; d = 260: 65 pieces, lane 0 holds two; d = 768: three passes; d = 1280: a row wider
than one block of 1024 elements.  n = 0, 1, 5; 1024 and 1025: one tile, and a second tile of one row; 2500: three tiles, the last
partial, and more rows than one workgroup's waves.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import grad_norm_fixture as GN  # noqa: E402
import test_gpu_opt_step as TO  # noqa: E402  (helpers only: tables, guarded arrays, id sets)

pytestmark = pytest.mark.gpu

N = TO.N
SENTINEL = -123.25
WIDTHS = [("bf16", 8), ("fp32", 260), ("int8", 768), ("fp16", 1280)]
COUNTS = (0, 1, 5, 1024, 1025, 2500)
SEED = 0x1234_5678_9ABC_DEF1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


_expected = {}


def _expect(n, d):
    """The value mix of (n, d) and the fixture's result for it: computed once, shared, never changed."""
    if (n, d) not in _expected:
        g = GN.value_mix(n, d)
        g.setflags(write=False)
        _expected[n, d] = (g,) + GN.sqnorm(g)
    return _expected[n, d]


def _same64(a, b):
    return np.array_equal(GN.bits64(a), GN.bits64(b))


def _run(table, g):
    """One call with a scratch of its own, four doubles longer than needed: (sq, Q, P) on the host; the tail must stay as it was."""
    n = g.shape[0]
    need = GN.scratch_doubles(n)
    scratch = torch.full((need + 4,), SENTINEL, dtype=torch.float64, device="cuda")
    sq, row_sq = table.grad_sqnorm(torch.from_numpy(g.copy()).cuda(), scratch=scratch)
    assert sq.dtype == torch.float64 and sq.dim() == 0 and sq.is_cuda
    assert row_sq.dtype == torch.float64 and tuple(row_sq.shape) == (n,) and (n == 0 or row_sq.data_ptr() == scratch.data_ptr())
    host = scratch.cpu().numpy()
    assert (host[need:] == SENTINEL).all(), "the call wrote past its scratch"
    return np.float64(sq.item()), host[:n], host[n:need]


# ------------------------------------------------------------------ 1. the order of the sums
@pytest.mark.parametrize("fmt,d", WIDTHS, ids=[f"{f}-d{d}" for f, d in WIDTHS])
def test_sums_equal_the_fixture_bit_for_bit(fmt, d):
    table = TO._table(fmt, d)
    for n in COUNTS:
        g, want_sq, want_q, want_p = _expect(n, d)
        sq, q, p = _run(table, g)
        assert len(p) == (n + 1023) // 1024
        assert _same64(q, want_q), f"n={n}: row {int(np.argmax(GN.bits64(q) != GN.bits64(want_q)))} differs"
        assert _same64(p, want_p), f"n={n}: tile sums {p} != {want_p}"
        assert _same64(sq, want_sq), f"n={n}: total {sq!r} != {want_sq!r}"
        assert n == 0 or (np.isfinite(sq) and sq > 1e76), "the mix holds 3e38"
        # the default scratch gives the same
        sq2, q2 = table.grad_sqnorm(torch.from_numpy(g.copy()).cuda())
        assert _same64(sq2.item(), want_sq) and _same64(q2.cpu().numpy(), want_q)
    assert table.status() == 0


def test_grid_cap_does_not_change_a_bit(monkeypatch):
    n, d = 2500, 768
    g, want_sq, want_q, want_p = _expect(n, d)
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "1")              # read at create: four waves walk the 2500 rows
    table = TO._table("int8", d)
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    sq, q, p = _run(table, g)
    assert _same64(q, want_q) and _same64(p, want_p) and _same64(sq, want_sq)


def test_special_values():
    d = 768
    table = TO._table("int8", d)
    rng = np.random.default_rng(2)

    def total(g):
        sq, q, p = _run(table, g)
        want = GN.sqnorm(g)
        if np.isfinite(want[0]):
            assert _same64(sq, want[0]) and _same64(q, want[1]) and _same64(p, want[2])
        return sq

    big = np.full((5, d), 3e38, dtype=np.float32)
    assert np.isfinite(total(big)) and total(big) > 1e77, "the square of 3e38 overflows fp32, not double"
    sub = (rng.integers(1, 1 << 23, size=(5, d)) * 2.0 ** -149).astype(np.float32)
    assert 0 < total(sub) < 1e-70, "subnormal elements count"
    one = np.zeros((1030, d), dtype=np.float32)
    one[1029, d - 1] = np.float32(2.0 ** -149)                   # the smallest subnormal, last element of the last tile
    assert total(one) == 2.0 ** -298
    ordinary = rng.standard_normal((1030, d)).astype(np.float32)
    for bad in ((np.nan,), (np.inf,), (np.inf, -np.inf)):
        g = ordinary.copy()
        g[1027, 5:5 + len(bad)] = bad
        sq, q, p = _run(table, g)
        assert not np.isfinite(sq), bad
        assert np.isfinite(q[:1027]).all() and not np.isfinite(q[1027]) and np.isfinite(p[0]) and not np.isfinite(p[1])
    assert np.isfinite(total(ordinary))
    zero = total(np.full((5, d), -0.0, dtype=np.float32))
    assert zero == 0.0 and not np.signbit(zero), "all -0.0 gives +0.0"
    empty = total(np.zeros((0, d), dtype=np.float32))
    assert empty == 0.0 and not np.signbit(empty)


# ------------------------------------------------------------------ 2. the control block
def _same_ctl(got, want):
    for name in ("sqnorm", "norm", "coef"):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype, name
        assert (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes(), f"{name}: {got[name]!r} != {want[name]!r}"
    assert got["skip"] == want["skip"] and got["reserved"] == want["reserved"] == 0, (got, want)


CTL_CASES = {
    "below": ([7.3], 1.0, 1.0, False),
    "equal": ([7.3], 1.0, float(np.sqrt(np.float64(7.3))), False),          # c = n / (n + 1e-6) < 1: still clipped
    "above": ([7.3], 1.0, 10.0, False),
    "no-clipping": ([7.3], 1.0, None, False),
    "infinite-max": ([7.3], 1.0, float("inf"), True),
    "loss-scale": ([7.3 * 1024 * 1024], 1.0 / 1024, 1.0, False),
    "negative-scale": ([7.3], -0.5, 1.0, False),
    "nan-term": ([1.0, float("nan")], 1.0, 1.0, False),
    "nan-term-skip": ([1.0, float("nan")], 1.0, 1.0, True),
    "inf-term-skip": ([float("inf"), 1.0], 1.0, 1.0, True),
    "inf-term": ([float("inf"), 1.0], 1.0, None, False),
    "finite-skip": ([7.3, 2.0], 1.0, 1.0, True),
    "zero": ([0.0], 1.0, 1.0, True),
    "order-a": ([1.0, 2.0 ** -53, 2.0 ** -53], 1.0, 0.5, False),            # 1
    "order-b": ([2.0 ** -53, 2.0 ** -53, 1.0], 1.0, 0.5, False),            # 1 + 2^-52
    "tiny-coef": ([1e300], 1.0, 1e-200, False),                             # (float)c is 0
}


@pytest.mark.parametrize("case", sorted(CTL_CASES))
def test_ctl_equals_the_fixture(case):
    terms, gs, max_norm, skip = CTL_CASES[case]
    table = TO._table("int8", 16)
    want = GN.ctl(terms, gs, np.inf if max_norm is None else max_norm, skip)
    as_floats = table.grad_ctl(terms, grad_scale=gs, max_norm=max_norm, skip_nonfinite=skip)
    as_tensors = table.grad_ctl([torch.tensor(x, dtype=torch.float64, device="cuda") for x in terms], grad_scale=gs,
                                max_norm=max_norm, skip_nonfinite=skip)
    as_vector = table.grad_ctl(torch.tensor(terms, dtype=torch.float64), grad_scale=gs, max_norm=max_norm, skip_nonfinite=skip)
    for ctl in (as_floats, as_tensors, as_vector):
        got = ctl.read()
        _same_ctl(got, want)
        # the views: 0-dim, on the device, the block's own bytes
        assert ctl.coef.dim() == 0 and ctl.coef.is_cuda and ctl.coef.dtype == torch.float32
        assert ctl.skip.dim() == 0 and ctl.skip.is_cuda
        assert np.float32(ctl.coef.item()).tobytes() == got["coef"].tobytes() and int(ctl.skip.item()) == got["skip"]
        assert ctl.coef.data_ptr() == ctl.buf.data_ptr() + 12 and ctl.skip.data_ptr() == ctl.buf.data_ptr() + 16
    assert CTL_CASES["order-a"][0] != CTL_CASES["order-b"][0]
    if case == "order-b":
        assert want["sqnorm"] == 1.0 + 2.0 ** -52 and GN.ctl(CTL_CASES["order-a"][0])["sqnorm"] == 1.0


def test_ctl_from_the_table_norm_and_a_dense_term():
    d = 768
    table = TO._table("int8", d)
    g, want_sq, _, _ = _expect(5, d)
    sq, _ = table.grad_sqnorm(torch.from_numpy(g.copy()).cuda())
    dense = torch.tensor(3.0e75, dtype=torch.float64, device="cuda")
    ctl = table.grad_ctl([sq, dense], grad_scale=2.0 ** -100, max_norm=1.0, skip_nonfinite=True)
    _same_ctl(ctl.read(), GN.ctl([want_sq, 3.0e75], 2.0 ** -100, 1.0, True))
    assert 0 < ctl.read()["coef"] < 1 and ctl.read()["skip"] == 0


# ------------------------------------------------------------------ 3. the _ctl steps against the plain steps
def _norm_of(table, g, gs):
    sq, _ = table.grad_sqnorm(torch.from_numpy(g).cuda())
    return float(np.sqrt(np.float64(sq.item())) * abs(gs)), sq


CLIPS = {"clipped": (0.37, 1.0), "not-clipped": (1e6, 1.0), "clipped-and-scaled": (0.37, 0.5), "scaled-only": (1e6, 0.5)}
FULL = [("sgd", "int8", 80), ("adagrad", "bf16", 264), ("adam", "int4", 128)]


def _check_coef(ctl, clip):
    coef = ctl.read()["coef"]
    assert (coef < 1 and 0.36 < coef < 0.38) if clip < 1 else coef.tobytes() == np.float32(1.0).tobytes()
    return coef


@pytest.mark.parametrize("case", sorted(CLIPS))
@pytest.mark.parametrize("kind,fmt,d", FULL, ids=[k for k, _, _ in FULL])
def test_opt_step_ctl_equals_the_plain_step(kind, fmt, d, case):
    clip, gs = CLIPS[case]
    rng, a, b, host, _ = TO._start(fmt, d, 11)
    dev_a, dev_b = ([TO._Guarded(x) for x in host] for _ in range(2))
    uses_m, uses_v = kind == "adam", kind != "sgd"
    for t, ids in enumerate(TO._id_sets(rng, 0, N), start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        norm, sq = _norm_of(a, g, gs)
        ctl = a.grad_ctl([sq], grad_scale=gs, max_norm=clip * norm)
        coef = _check_coef(ctl, clip)
        hp = dict(TO.HP, weight_decay=0.01, step=t)
        for table, dev, kw in ((a, dev_a, dict(grad_scale=gs, ctl=ctl)),
                               (b, dev_b, dict(grad_scale=float(np.float32(gs) * np.float32(coef))))):
            table.opt_step(torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), dev[0].view, kind=kind,
                           state1=dev[1].view if uses_m else None, state2=dev[2].view if uses_v else None, **hp, **kw)
        got_a, got_b = ([x.read() for x in dev] for dev in (dev_a, dev_b))
        for name, x, y in zip(("master", "state1", "state2"), got_a, got_b):
            assert TO._same_bytes(x, y), f"t={t}: {name} differs from the plain step's"
        assert not TO._same_bytes(got_a[0], host[0]), "the step changed nothing"
        ta, tb = a.download(0, N), b.download(0, N)
        assert TO._same_bytes(ta[0], tb[0]) and TO._same_bytes(ta[1], tb[1]), f"t={t}: the served table differs"
        assert a.status() == 0 and b.status() == 0
        host = got_a


LEAN = [("sgd", "master", "mxfp4", 128), ("rowwise_adagrad", "master", "int8", 1040), ("sgd", "f32", "fp32", 260),
        ("rowwise_adagrad", "f32", "fp32", 8), ("sgd", "bf16", "bf16", 264), ("rowwise_adagrad", "bf16", "bf16", 1280),
        ("sgd", "bf16s", "bf16", 8), ("rowwise_adagrad", "bf16s", "bf16", 264)]


def _lean_pair(mode, fmt, d, seed):
    """Two handles holding the same table, each with its own guarded master (master mode) and row state."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((N, d)).astype(np.float32)
    if fmt == "bf16":
        w = BF.stored(w)
    s = (rng.standard_normal(N) ** 2).astype(np.float32)
    sides = []
    for _ in range(2):
        t = TO._table(fmt, d)
        t.store_f32(torch.from_numpy(w))
        sides.append((t, TO._Guarded(w) if mode == "master" else None, TO._Guarded(s[:, None])))
    return rng, w, s, sides


def _lean_call(side, mode, kind, ids, g, t, **kw):
    table, dev_w, dev_s = side
    table.opt_step_lean(torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), kind=kind, lr=0.05, eps=1e-10, weight_decay=0.01,
                        master=dev_w.view if mode == "master" else None,
                        row_state=dev_s.view.reshape(-1) if kind == "rowwise_adagrad" else None,
                        rounding="stochastic" if mode == "bf16s" else "nearest", seed=SEED, step=t, **kw)


def _lean_bytes(side):
    table, dev_w, dev_s = side
    rows, scales = table.download(0, N)
    return [rows, scales, None if dev_w is None else dev_w.read(), dev_s.read()]


@pytest.mark.parametrize("case", sorted(CLIPS))
@pytest.mark.parametrize("kind,mode,fmt,d", LEAN, ids=[f"{k}-{m}" for k, m, _, _ in LEAN])
def test_opt_step_lean_ctl_equals_the_plain_step(kind, mode, fmt, d, case):
    clip, gs = CLIPS[case]
    rng, w, s, (a, b) = _lean_pair(mode, fmt, d, 13)
    start = _lean_bytes(a)
    for t, ids in enumerate(TO._id_sets(rng, 0, N), start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        norm, sq = _norm_of(a[0], g, gs)
        ctl = a[0].grad_ctl([sq], grad_scale=gs, max_norm=clip * norm)
        coef = _check_coef(ctl, clip)
        _lean_call(a, mode, kind, ids, g, t, grad_scale=gs, ctl=ctl)
        _lean_call(b, mode, kind, ids, g, t, grad_scale=float(np.float32(gs) * np.float32(coef)))
        got_a, got_b = _lean_bytes(a), _lean_bytes(b)
        for name, x, y in zip(("table rows", "scales", "master", "row state"), got_a, got_b):
            assert TO._same_bytes(x, y), f"t={t}: {name} differ from the plain step's"
        assert not TO._same_bytes(got_a[0], start[0]), "the step changed nothing"
        assert a[0].status() == 0 and b[0].status() == 0


def _skip_ctl(table, g):
    sq, _ = table.grad_sqnorm(torch.from_numpy(g).cuda())
    ctl = table.grad_ctl([sq], max_norm=1.0, skip_nonfinite=True)
    got = ctl.read()
    assert got["skip"] == 1 and np.isnan(got["sqnorm"])
    return ctl


def _poisoned(rng, d):
    """Ids with one outside the table and one out of order, and a gradient with a NaN: a skipped step looks at neither."""
    ids = np.asarray([0, 5, 4, 17, N - 1, N + 3], dtype=np.int64)
    g = rng.standard_normal((len(ids), d)).astype(np.float32)
    g[3, d // 2] = np.nan
    return ids, g


@pytest.mark.parametrize("kind,fmt,d", FULL, ids=[k for k, _, _ in FULL])
def test_a_skipped_opt_step_changes_nothing(kind, fmt, d):
    from scone_amd import _lib
    rng, a, b, host, dev = TO._start(fmt, d, 17)
    ids, g = _poisoned(rng, d)
    before = a.download(0, N)
    ctl = _skip_ctl(a, g)
    args = (torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), dev[0].view)
    kw = dict(TO.HP, kind=kind, state1=dev[1].view if kind == "adam" else None, state2=dev[2].view if kind != "sgd" else None,
              weight_decay=0.01, step=1)
    a.opt_step(*args, ctl=ctl, **kw)
    for name, x, y in zip(("master", "state1", "state2"), [x.read() for x in dev], host):        # read() checks the guard rows
        assert TO._same_bytes(x, y), f"{name} changed"
    after = a.download(0, N)
    assert TO._same_bytes(after[0], before[0]) and TO._same_bytes(after[1], before[1]), "the served table changed"
    assert a.status() == 0, "a skipped step raised a status bit"
    # the same call without the block does write NaN and does report the ids: the skip is what kept them out
    a.opt_step(*args, **kw)
    assert a.status() == _lib.ST_BAD_ID and np.isnan(dev[0].read()).any()


@pytest.mark.parametrize("kind,mode,fmt,d", LEAN[1::2], ids=[f"{k}-{m}" for k, m, _, _ in LEAN[1::2]])
def test_a_skipped_lean_step_changes_nothing(kind, mode, fmt, d):
    from scone_amd import _lib
    rng, w, s, (a, _) = _lean_pair(mode, fmt, d, 19)
    ids, g = _poisoned(rng, d)
    before = _lean_bytes(a)
    ctl = _skip_ctl(a[0], g)
    _lean_call(a, mode, kind, ids, g, 1, ctl=ctl)
    for name, x, y in zip(("table rows", "scales", "master", "row state"), _lean_bytes(a), before):
        assert TO._same_bytes(x, y), f"{name} changed"
    assert a[0].status() == 0, "a skipped step raised a status bit"
    _lean_call(a, mode, kind, ids, g, 1)
    assert a[0].status() == _lib.ST_BAD_ID and not TO._same_bytes(_lean_bytes(a)[0], before[0])


# ------------------------------------------------------------------ 4. refusals
def test_refusals():
    from scone_amd import _lib
    from scone_amd.hip_backend import SconeTable
    lib = _lib.lib()
    d = 16
    t = TO._table("bf16", d)
    P = lambda x: x.data_ptr()                                   # noqa: E731
    w, s = torch.zeros((N, d), device="cuda"), torch.zeros(N, device="cuda")
    ids, g = torch.arange(4, device="cuda"), torch.ones((4, d), device="cuda")
    terms = torch.ones(65, dtype=torch.float64, device="cuda")
    block = torch.zeros(3, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(8, dtype=torch.float64, device="cuda")
    out = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda")
    stored = t.download(0, N)[0].copy()

    def refused(rc, *words):
        msg = lib.scone_last_error(t._h)
        return rc == _lib.EINVAL and all(x in msg for x in words)

    ocfg = _lib.OptCfg(C.sizeof(_lib.OptCfg), _lib.OPT_SGD, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1)
    lcfg = _lib.LeanCfg(C.sizeof(_lib.LeanCfg), _lib.LEAN_SGD, 0, 0, 0.1, 1e-10, 0.0, 1.0, 0, 1)
    assert refused(lib.scone_opt_step_ctl(t._h, ocfg, P(ids), P(g), 4, P(w), None, None, None, None), b"scone_opt_step_ctl: ", b"null d_ctl")
    assert refused(lib.scone_opt_step_lean_ctl(t._h, lcfg, P(ids), P(g), 4, P(w), None, None, None), b"scone_opt_step_lean_ctl: ", b"null d_ctl")
    assert refused(lib.scone_opt_step_lean_ctl(t._h, lcfg, P(ids), P(g), 4, None, None, None, None), b"scone_opt_step_lean_ctl: ", b"null d_ctl")
    assert refused(lib.scone_opt_step_ctl(t._h, ocfg, None, P(g), 4, P(w), None, None, P(block), None), b"scone_opt_step_ctl: ", b"null pointer")
    assert refused(lib.scone_opt_step_ctl(t._h, None, P(ids), P(g), 4, P(w), None, None, P(block), None), b"scone_opt_step_ctl: ", b"null cfg")
    for n_terms in (0, 65, -1):
        assert refused(lib.scone_grad_ctl_set(t._h, P(terms), n_terms, 1.0, 1.0, 0, P(block), None), b"scone_grad_ctl_set: ", b"n_terms")
    for max_norm in (0.0, -1.0, float("nan")):
        assert refused(lib.scone_grad_ctl_set(t._h, P(terms), 1, 1.0, max_norm, 0, P(block), None), b"scone_grad_ctl_set: ", b"max_norm")
    for gs in (float("inf"), float("nan")):
        assert refused(lib.scone_grad_ctl_set(t._h, P(terms), 1, gs, 1.0, 0, P(block), None), b"scone_grad_ctl_set: ", b"grad_scale")
    assert refused(lib.scone_grad_ctl_set(t._h, None, 1, 1.0, 1.0, 0, P(block), None), b"scone_grad_ctl_set: ", b"null")
    assert refused(lib.scone_grad_ctl_set(t._h, P(terms), 1, 1.0, 1.0, 0, None, None), b"scone_grad_ctl_set: ", b"null")
    assert refused(lib.scone_grad_sqnorm(t._h, None, 4, P(scratch), P(out), None), b"scone_grad_sqnorm: ", b"null")
    assert refused(lib.scone_grad_sqnorm(t._h, P(g), 4, None, P(out), None), b"scone_grad_sqnorm: ", b"null")
    assert refused(lib.scone_grad_sqnorm(t._h, P(g), 4, P(scratch), None, None), b"scone_grad_sqnorm: ", b"d_sq_out")
    index_only = SconeTable(3, N)                                  # dim == 0
    rc = lib.scone_grad_sqnorm(index_only._h, P(g), 4, P(scratch), P(out), None)
    assert rc == _lib.EINVAL and b"scone_grad_sqnorm: " in lib.scone_last_error(index_only._h) and b"dim == 0" in lib.scone_last_error(index_only._h)
    # the Python layer
    with pytest.raises(ValueError, match="max_norm"):
        t.grad_ctl([1.0], max_norm=0.0)
    with pytest.raises(ValueError, match="n_terms"):
        t.grad_ctl([])
    with pytest.raises(ValueError, match="grad_rows"):
        t.grad_sqnorm(torch.ones((4, d + 4), device="cuda"))
    with pytest.raises(ValueError, match="scratch"):
        t.grad_sqnorm(g, scratch=torch.zeros(2, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert bool((w == 0).all()) and bool((s == 0).all()) and bool((block == 0).all()) and bool((scratch == 0).all()), "a refused call wrote"
    assert float(out.item()) == SENTINEL and t.status() == 0 and np.array_equal(t.download(0, N)[0], stored), "a refused call wrote"
    # n == 0 with a block: a no-op; n == 0 of the norm: +0.0 with no other pointer
    assert lib.scone_opt_step_ctl(t._h, ocfg, None, None, 0, None, None, None, P(block), None) == _lib.OK
    assert lib.scone_grad_sqnorm(t._h, None, 0, None, P(out), None) == _lib.OK
    assert float(out.item()) == 0.0
