"""The lean optimizer step (`scone_opt_step_lean`, `SconeTable.opt_step_lean`, `InPlaceFGramTable`, `FGramOptimizer`'s lean
kinds) against its numpy statement, tests/lean_fixture.py.

The contract (include/scone_hip.h, "lean optimizer step") fixes every rounding, the order of the row sum and the random bits,
so there is no tolerance: every comparison is bit for bit (`edge_fixture.same_bits`; NaN payloads are not compared) and over
WHOLE arrays -- the table's download, the master, the row state -- so a row that is not listed is covered by the same
comparison.  Device arrays sit between guard rows of NaN that must come back untouched (test_gpu_opt_step's `_Guarded`), the
scalars are read from `scone_lean_scalars_of`, and `table.status()` is checked after every step.

A `_Run` holds one table in one of four modes and its host twin: "master" (fp32 master + a served table of any format; the
table must equal a second handle's after `store_f32` of the new master rows), "f32" (in place on an fp32 table), "bf16" and
"bf16s" (in place on a bf16 table, rounded to nearest / stochastically).  Set-up as in test_gpu_opt_step: N = 300 rows, three
steps over overlapping id sets that hold rows 0 and N - 1.

Widths: d = 8 (two pieces, 62 idle lanes in the butterfly), 256 (one piece per lane), 264 (ragged), 768, 1024 (exactly one
block), 1032 (the first row that walks g twice), 4104 (more than four blocks).
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import bf16_fixture as BF  # noqa: E402
import edge_fixture as E  # noqa: E402
import lean_fixture as LF  # noqa: E402
import opt_fixture as OF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only: the WS batches, their id lists)
import test_gpu_opt_step as TO  # noqa: E402  (helpers only: tables, guarded arrays, id sets, FORMAT_CASES)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, bit views)

pytestmark = pytest.mark.gpu

N = TO.N
HP = dict(lr=0.05, eps=1e-10)
KINDS = ("sgd", "rowwise_adagrad")
WIDTHS = (8, 256, 264, 768, 1024, 1032, 4104)
MODES = ("master", "f32", "bf16", "bf16s")
SEED = 0x1234_5678_9ABC_DEF1           # above 2^32: the high half of the seed is used


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _scalars(kind, wd=0.0, gs=1.0, **hp):
    from scone_amd.hip_backend import lean_scalars
    return lean_scalars(kind, **dict(HP, weight_decay=wd, grad_scale=gs, **hp))


class _Run:
    """One table, its device arrays and their host twins; `step` makes one call and checks everything."""

    def __init__(self, mode, d, kind, fmt=None, n=N, own=None, table_kw=None, seed=0, w=None, s=None):
        self.mode, self.d, self.kind, self.n = mode, d, kind, n
        self.lo, self.hi = own if own else (0, n)
        self.fmt = fmt or {"master": "int8", "f32": "fp32"}.get(mode, "bf16")
        self.rng = rng = np.random.default_rng(1000 * d + seed)
        rows = self.hi - self.lo
        w = rng.standard_normal((rows, d)).astype(np.float32) if w is None else w
        if mode in ("bf16", "bf16s"):
            w = BF.stored(w)                                   # what the table holds, exactly
        self.w = w                                             # master / the fp32 table / the bf16 table widened
        self.s = (rng.standard_normal(rows) ** 2).astype(np.float32) if s is None else s
        self.a = TO._table(self.fmt, d, n, own, **(table_kw or {}))
        self.a.store_f32(torch.from_numpy(w), row0=self.lo)
        self.b = None
        if mode == "master":
            self.b = TO._table(self.fmt, d, n, own, **(table_kw or {}))
            self.b.store_f32(torch.from_numpy(w), row0=self.lo)
            self.dev_w = TO._Guarded(w)
        self.dev_s = TO._Guarded(self.s[:, None])
        self.t = 0

    @property
    def rounding(self):
        return "stochastic" if self.mode == "bf16s" else "nearest"

    def table_bits(self):
        raw = self.a.download(self.lo, self.hi - self.lo)[0]
        return raw.view(np.float32) if self.mode == "f32" else BF.rows_as_bits(raw)

    def expect(self, ids, g, sc, t):
        state = self.s if self.kind == "rowwise_adagrad" else None
        if self.mode in ("bf16", "bf16s"):
            bits, s, applied, bad, _ = LF.apply_bf16(self.kind, sc, ids, g, BF.to_bf16_bits(self.w), state, self.lo, self.hi,
                                                     rounding=self.rounding, seed=SEED, step_no=t)
            return BF.from_bf16_bits(bits), s, applied, bad
        return LF.apply(self.kind, sc, ids, g, self.w, state, self.lo, self.hi)

    def call(self, ids, g, t, wd=0.0, gs=1.0):
        rowwise = self.kind == "rowwise_adagrad"
        self.a.opt_step_lean(torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), kind=self.kind,
                             master=self.dev_w.view if self.mode == "master" else None,
                             row_state=self.dev_s.view.reshape(-1) if rowwise else None, weight_decay=wd, grad_scale=gs,
                             rounding=self.rounding, seed=SEED, step=t, **HP)

    def step(self, ids, g, wd=0.0, gs=1.0, tag=""):
        from scone_amd import _lib
        self.t += 1
        tag = f"{tag or self.mode}-{self.fmt}-d{self.d}-{self.kind}-wd{wd}-gs{gs}-t{self.t}"
        sc = _scalars(self.kind, wd, gs)
        want_w, want_s, applied, bad = self.expect(ids, g, sc, self.t)
        before = self.a.download(self.lo, self.hi - self.lo)
        self.call(ids, g, self.t, wd, gs)
        assert self.a.status() == (_lib.ST_BAD_ID if bad else 0), f"{tag}: status"
        got_s = self.dev_s.read()[:, 0]
        keep_s = want_s if self.kind == "rowwise_adagrad" else self.s
        assert E.same_bits(got_s, keep_s), f"{tag}: row state: {E.first_difference(got_s[:, None], keep_s[:, None])}"
        rest = np.setdiff1d(np.arange(self.lo, self.hi), applied) - self.lo
        after = self.a.download(self.lo, self.hi - self.lo)
        assert np.array_equal(after[0][rest], before[0][rest]), f"{tag}: a table row that is not listed changed"
        if self.mode == "master":
            got_w = self.dev_w.read()
            assert E.same_bits(got_w, want_w), f"{tag}: master: {E.first_difference(got_w, want_w)}"
            assert np.array_equal(got_w[rest].view(np.uint32), self.w[rest].view(np.uint32)), f"{tag}: an unlisted master row changed"
            if len(applied):                                   # the GPU's own w': equal NaN payloads too
                self.b.store_f32(torch.from_numpy(np.ascontiguousarray(got_w[applied - self.lo])), ids=torch.from_numpy(applied))
            ref = self.b.download(self.lo, self.hi - self.lo)
            assert TO._same_bytes(after[0], ref[0]) and TO._same_bytes(after[1], ref[1]), f"{tag}: the served table differs from store_f32's"
            assert before[1] is None or np.array_equal(after[1][rest].view(np.uint8), before[1][rest].view(np.uint8)), f"{tag}: scales"
            assert self.b.status() == 0
        else:
            got = self.table_bits()
            want = want_w if self.mode == "f32" else BF.to_bf16_bits(want_w)
            assert E.same_bits(got, want), f"{tag}: table: {E.first_difference(got, want)}"
        self.w, self.s = want_w, keep_s
        return applied

    def three_steps(self, wd=0.0, gs=1.0, id_sets=None, tag=""):
        for ids in id_sets or TO._id_sets(self.rng, self.lo, self.hi):
            g = self.rng.standard_normal((len(ids), self.d)).astype(np.float32)
            self.step(ids, g, wd, gs, tag)
        return self


# ------------------------------------------------------------------ 1. widths, in every mode
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", WIDTHS)
def test_widths(d, mode):
    fmt = "bf16" if mode == "master" else None                # a format every width here fits (d % 8 == 0)
    _Run(mode, d, "rowwise_adagrad", fmt=fmt).three_steps(0.01, 1.0)


# ------------------------------------------------------------------ 2. master mode: every format
@pytest.mark.parametrize("fmt,d", TO.FORMAT_CASES, ids=[f"{f}-d{d}" for f, d in TO.FORMAT_CASES])
def test_master_mode_formats(fmt, d):
    _Run("master", d, "rowwise_adagrad", fmt=fmt).three_steps(0.01, 0.5)


@pytest.mark.parametrize("fmt,d", [("fp32", 4), ("fp16", 8), ("int8", 80), ("int8", 1040), ("bf16", 264), ("int4", 128), ("mxfp4", 128)])
def test_master_sgd_equals_opt_step(fmt, d):
    lean = _Run("master", d, "sgd", fmt=fmt, seed=3)
    rng = np.random.default_rng(d)
    other = TO._table(fmt, d)
    other.store_f32(torch.from_numpy(lean.w))
    master = TO._Guarded(lean.w)
    for t, ids in enumerate(TO._id_sets(rng, 0, N), start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        lean.step(ids, g, 0.01, 0.5)
        other.opt_step(torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), master.view, kind="sgd", lr=HP["lr"],
                       weight_decay=0.01, grad_scale=0.5, step=t)
        assert np.array_equal(master.read().view(np.uint32), lean.dev_w.read().view(np.uint32)), "master differs from scone_opt_step's"
        x, y = other.download(0, N), lean.a.download(0, N)
        assert TO._same_bytes(x[0], y[0]) and TO._same_bytes(x[1], y[1]), "table differs from scone_opt_step's"


# ------------------------------------------------------------------ 3. in place: kinds, decay, gradient scale
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16s"])
def test_in_place_kinds_decay_and_grad_scale(mode, kind, wd, gs):
    _Run(mode, 264, kind, seed=7).three_steps(wd, gs)


@pytest.mark.parametrize("kind", KINDS)
def test_in_place_fp32_equals_master_mode_on_an_fp32_table(kind):
    d = 264
    a, b = _Run("f32", d, kind, seed=9), _Run("master", d, kind, fmt="fp32", seed=9)
    assert np.array_equal(a.w, b.w)
    a.three_steps(0.01, 0.5)
    b.three_steps(0.01, 0.5)                                  # the same generator state: the same ids and gradients
    x, y = a.a.download(0, N)[0], b.a.download(0, N)[0]
    assert np.array_equal(x, y) and np.array_equal(a.dev_s.read().view(np.uint32), b.dev_s.read().view(np.uint32))
    assert np.array_equal(x.view(np.float32).view(np.uint32), b.dev_w.read().view(np.uint32))


# ------------------------------------------------------------------ 4. U, and a grid of one workgroup
def test_row_counts():
    run = _Run("bf16s", 264, "rowwise_adagrad", seed=5)
    sets = [np.zeros(0, dtype=np.int64), np.asarray([N - 1], dtype=np.int64), np.asarray([0, 150, N - 1], dtype=np.int64),
            np.asarray([0, 1, 150, N - 1], dtype=np.int64), np.asarray([0, 7, 8, 150, N - 1], dtype=np.int64)]
    assert [len(s) for s in sets] == [0, 1, 3, 4, 5]
    for ids in sets:
        run.step(ids, run.rng.standard_normal((len(ids), 264)).astype(np.float32), 0.01, 1.0, tag=f"U{len(ids)}")


@pytest.mark.parametrize("mode", ["master", "bf16s"])
def test_one_workgroup_takes_257_rows(monkeypatch, mode):
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "1")             # read at create: 4 waves walk the 257 rows
    run = _Run(mode, 1040 if mode == "master" else 1032, "rowwise_adagrad", seed=6)
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    for _ in (1, 2):
        ids = np.sort(run.rng.choice(N, size=257, replace=False)).astype(np.int64)
        run.step(ids, run.rng.standard_normal((257, run.d)).astype(np.float32), 0.01, 1.0, tag="capped")


# ------------------------------------------------------------------ 5. stochastic rounding, without the fixture's rand16
def _bf16_table(w, n=None, own=None, **kw):
    t = TO._table("bf16", w.shape[1], n or w.shape[0], own, **kw)
    t.store_f32(torch.from_numpy(w), row0=own[0] if own else 0)
    return t


def _bits_of(t, lo=0, n=None):
    return BF.rows_as_bits(t.download(lo, n if n is not None else t.row_end - t.row_begin)[0])


def _lean(t, ids, g, **kw):
    t.opt_step_lean(torch.from_numpy(np.asarray(ids, dtype=np.int64)).cuda(), torch.from_numpy(g).cuda(),
                    **dict(dict(kind="sgd", rounding="stochastic", seed=SEED, step=1, **HP), **kw))
    assert t.status() == 0


def test_stochastic_zero_gradient_and_neighbours():
    rows, d = 40, 1032
    rng = np.random.default_rng(12)
    w = BF.stored(rng.standard_normal((rows, d)).astype(np.float32))
    t = _bf16_table(w)
    ids = np.arange(0, rows, 2, dtype=np.int64)
    before = _bits_of(t)
    for kind in KINDS:                                          # a listed row with a zero gradient and no decay keeps every bit
        state = torch.ones(rows, device="cuda")
        _lean(t, ids, np.zeros((len(ids), d), dtype=np.float32), kind=kind, row_state=state if kind != "sgd" else None)
        assert np.array_equal(_bits_of(t), before), f"{kind}: a zero gradient changed a row"
    g = rng.standard_normal((len(ids), d)).astype(np.float32)
    sc = _scalars("sgd", 0.01, 0.5)
    want = OF.step_f32(OF.SGD, sc, g, w[ids])[0]                # opt_fixture's arithmetic on the widened row
    _lean(t, ids, g, weight_decay=0.01, grad_scale=0.5)
    got = _bits_of(t)
    u = want.view(np.uint32)
    down, frac = (u >> 16).astype(np.uint16), u & 0xFFFF
    up = np.where(frac != 0, down + 1, down).astype(np.uint16)
    assert ((got[ids] == down) | (got[ids] == up)).all(), "a stored value is not a bf16 neighbour of w'"
    share = float((got[ids] == up)[frac != 0].mean())
    assert 0.4 < share < 0.6, f"{share:.3f} of the inexact values were rounded away from zero"
    assert np.array_equal(got[1::2], before[1::2]), "an unlisted row changed"


def test_stochastic_drift_on_the_device():
    """4 rows x d = 1024 at w = 1.0, 256 launches of alpha * g = 2^-12: see tests/test_lean_host.py test_drift_of_small_steps
    for the bound (4,096 elements: the standard deviation of the mean is about 2^-11)."""
    rows, d, steps = 4, 1024, 256
    ones = np.ones((rows, d), dtype=np.float32)
    near, sto = _bf16_table(ones), _bf16_table(ones)
    ids, g = torch.arange(rows, device="cuda"), torch.ones((rows, d), device="cuda")
    for t in range(1, steps + 1):
        near.opt_step_lean(ids, g, kind="sgd", lr=2.0 ** -12, rounding="nearest")
        sto.opt_step_lean(ids, g, kind="sgd", lr=2.0 ** -12, rounding="stochastic", seed=SEED, step=t)
    assert (_bits_of(near) == 0x3F80).all(), "nearest rounding moved a weight by a step below half an ulp"
    drift = float((1.0 - BF.from_bf16_bits(_bits_of(sto)).astype(np.float64)).mean())
    print(f"mean of 1 - w = {drift:.6f} (2^-4 = {2.0 ** -4:.6f}, sd of the mean 2^-11 = {2.0 ** -11:.6f})")
    assert abs(drift - 2.0 ** -4) <= 6 * 2.0 ** -11
    assert near.status() == 0 and sto.status() == 0


def test_stochastic_bits_depend_on_seed_step_row_and_column_only(monkeypatch):
    n, d, row = 300, 1032, 157
    rng = np.random.default_rng(13)
    w = BF.stored(rng.standard_normal((n, d)).astype(np.float32))
    g_row = rng.standard_normal((1, d)).astype(np.float32)

    def alone(**kw):
        t = _bf16_table(w)
        _lean(t, [row], g_row, **kw)
        return _bits_of(t)[row]

    base = alone()
    assert np.array_equal(alone(), base), "two runs with the same (seed, step) differ"
    assert not np.array_equal(alone(seed=SEED + 1), base) and not np.array_equal(alone(step=2), base)
    assert not np.array_equal(alone(seed=SEED ^ (1 << 40)), base), "the high half of the seed is not used"
    # inside a 100-row list
    ids = np.unique(np.concatenate([rng.choice(n, size=99, replace=False), [row]])).astype(np.int64)
    g = rng.standard_normal((len(ids), d)).astype(np.float32)
    g[np.searchsorted(ids, row)] = g_row[0]
    t = _bf16_table(w)
    _lean(t, ids, g)
    assert np.array_equal(_bits_of(t)[row], base), "the bits of a row depend on the list it is in"
    # the same list on a handle whose grid is one workgroup
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "1")
    t = _bf16_table(w)
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    _lean(t, ids, g)
    assert np.array_equal(_bits_of(t)[row], base), "the bits of a row depend on the grid"
    # a handle that owns the row as a shard with row_begin > 0
    own = (100, 200)
    t = _bf16_table(w[own[0]:own[1]], n=n, own=own)
    _lean(t, [row], g_row)
    assert np.array_equal(_bits_of(t, own[0])[row - own[0]], base), "the bits of a row depend on the shard (local row ids were hashed)"


# ------------------------------------------------------------------ 6. edge values
EDGE_D = 272                                                     # 68 pieces: lanes 0 .. 3 hold eight elements, d % 16 == 0 for INT8


def _edge_inputs(kind, seed=3):
    """g, w [40, 272], s [40].  By row: 0-7 ordinary values (their sum of squares shows a fused multiply-add); 8-15 gradients of
    about 2^-70 with s = 0 (every square is subnormal: flush-to-zero leaves q = 0); 16-19 a gradient with +-inf (q = inf: the
    step is x / inf = 0, and inf / inf = NaN); 20-23 -0.0 in g and in w; 24-27 bf16-subnormal weights and gradients whose update
    is an fp32 subnormal; 28-31 weights at the largest finite bf16 pushed outwards by 3/4 of a bf16 ulp (SGD: the carry gives
    infinity); 32-35 weights holding +-inf and NaN; 36-39 gradients holding NaN."""
    rng = np.random.default_rng(seed)
    f = np.float32
    rows, d = 40, EDGE_D
    g = rng.standard_normal((rows, d)).astype(f)
    w = rng.standard_normal((rows, d)).astype(f)
    s = (rng.standard_normal(rows) ** 2).astype(f)
    sign = rng.choice(np.asarray([-1.0, 1.0], dtype=f), size=(rows, d))
    k = rng.integers(1, 9, size=(rows, d)).astype(f)
    g[8:16] = (g[8:16] * f(2.0 ** -70)).astype(f)
    s[8:16] = 0
    for r in range(16, 20):
        g[r, rng.choice(d, size=2, replace=False)] = [np.inf, -np.inf][:2] if r % 2 else [np.inf, np.inf]
    g[20:24, ::3], w[20:24, 1::3] = f(-0.0), f(-0.0)
    g[20:24, 5::7] = f(0.0)
    g[20:24, 4::21] = f(-0.0)                                   # with w = -0.0: -0.0 - (-0.0) = +0.0
    w[24:28] = sign[24:28] * k[24:28] * f(2.0 ** -133)
    g[24:28] = sign[24:28] * k[24:28] * f(2.0 ** -128)
    big = f(np.uint32(0x7F7F0000).view(f))
    w[28:32] = sign[28:32] * big
    if kind == "sgd":
        g[28:32] = -sign[28:32] * f(0.75 * 2.0 ** 120 / HP["lr"])
    w[32:36, ::5], w[32:36, 1::5], w[32:36, 2::5] = f(np.inf), f(-np.inf), f(np.nan)
    g[36:40, ::9] = f(np.nan)
    return g, w, s


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_edge_values(kind, mode):
    g, w, s = _edge_inputs(kind)
    rows = g.shape[0]
    ids = np.arange(rows, dtype=np.int64)
    run = _Run(mode, EDGE_D, kind, n=rows, w=w, s=s)
    for wd, gs in ((0.0, 1.0), (0.01, 0.5)):
        sc = _scalars(kind, wd, gs)
        args = (kind, sc, g, run.w, run.s if kind != "sgd" else None)
        outs = LF.step_f32(*args)
        fused, flushed = LF.step_f32(*args, fma=True), LF.step_f32(*args, ftz=True)

        def differs(other, rows_=slice(None)):
            return any(x is not None and not E.same_bits(x[rows_], y[rows_]) for x, y in zip(other, outs))

        if wd == 0.0:                                           # (the second round starts from what the first one left: not asserted)
            assert differs(fused), "a fused multiply-add would pass"
            assert differs(flushed), "flush-to-zero would pass"
        if kind == "rowwise_adagrad" and wd == 0.0:
            q, qf, qz = LF.row_sum_sq(g), LF.row_sum_sq(g, fma=True), LF.row_sum_sq(g, ftz=True)
            assert (q[:8].view(np.uint32) != qf[:8].view(np.uint32)).any(), "the row sum does not show an FMA"
            assert (q[8:16] != 0).all() and (qz[8:16] == 0).all(), "the row sum does not show flushed squares"
            assert differs(fused, slice(0, 8)) and differs(flushed, slice(8, 16))
            assert np.isinf(q[16:20]).all() and np.isnan(q[36:40]).all()
        want = outs[0]
        assert np.isnan(want).any() and (want == 0).any() and (wd != 0.0 or np.isinf(want).any())    # inf - decay * inf = NaN
        assert ((np.abs(want) < np.float32(2.0 ** -126)) & (want != 0)).any(), "no subnormal result"
        if kind == "sgd" and wd == 0.0:
            assert np.isfinite(run.w[28:32]).all() and np.isinf(BF.stored(want[28:32])).all(), "no carry out of the largest bf16"
            assert (BF.to_bf16_bits(want[20:24]) == 0x8000).any(), "no -0.0 result"
        run.step(ids, g, wd, gs, tag="edge")
    if mode == "bf16s" and kind == "sgd":                       # the carry is a matter of the random bits: both outcomes occur
        t = _bf16_table(BF.stored(w))
        _lean(t, ids, g)
        got = _bits_of(t)[28:32] & 0x7FFF
        assert set(np.unique(got)) == {0x7F7F, 0x7F80}, "3/4 of a bf16 ulp beyond the largest finite value: both neighbours occur"
        assert 0.6 < float((got == 0x7F80).mean()) < 0.9


# ------------------------------------------------------------------ 7. bad ids, a row-sharded handle, placements
@pytest.mark.parametrize("mode", ["master", "bf16s"])
def test_bad_ids_are_skipped_and_reported(mode):
    run = _Run(mode, 272, "rowwise_adagrad", seed=8)
    lists = [np.asarray([-1, 2, 5, 5, 9, 7, 20, 31, N], dtype=np.int64),
             np.asarray([0, 3, 3, 299, 298, N + 5, -(2 ** 40), 2 ** 40], dtype=np.int64),
             np.asarray([0, 5, 9, N - 1], dtype=np.int64)]
    want_applied = [[2, 5, 9, 20, 31], [0, 3, 299], [0, 5, 9, N - 1]]
    for ids, wa in zip(lists, want_applied):
        applied = run.step(ids, run.rng.standard_normal((len(ids), 272)).astype(np.float32), 0.01, 1.0, tag="bad-ids")
        assert applied.tolist() == wa                           # (the row state of every skipped row is in the whole-array comparison)


@pytest.mark.parametrize("mode", ["master", "f32", "bf16s"])
def test_row_sharded_handle(mode):
    own = (100, 200)
    run = _Run(mode, 256, "rowwise_adagrad", fmt="int4" if mode == "master" else None, own=own, seed=9)
    assert run.w.shape == (100, 256) and run.s.shape == (100,)
    lists = [np.asarray([-3, 50, 99, 100, 120, 120, 150, 140, 199, 200, 250], dtype=np.int64)] + TO._id_sets(run.rng, *own, count=40)[:2]
    for i, ids in enumerate(lists):
        applied = run.step(ids, run.rng.standard_normal((len(ids), 256)).astype(np.float32), 0.01, 1.0, tag="shard")
        if i == 0:
            assert applied.tolist() == [100, 120, 150, 199]


@pytest.mark.parametrize("mode", ["master", "f32", "bf16s"])
def test_pinned_host_table_with_a_hot_head(mode):
    sets = [np.asarray([0, 10, 15, 16, 17, 40, N - 1], dtype=np.int64), np.asarray([0, 15, 16, 100, N - 1], dtype=np.int64),
            np.asarray([0, 14, 15, 16, 17, 18, 200, N - 1], dtype=np.int64)]
    run = _Run(mode, 1040, "rowwise_adagrad", table_kw=dict(placement="pinned_host", hot_rows=16, stage_tokens=0))
    run.three_steps(0.01, 1.0, id_sets=sets, tag="pinned")


def test_staged_prefetch_table():
    """stage_tokens > 0: the staged cache of cold rows is dropped by the step, so the next lookup reads the updated rows."""
    from scone_amd.hip_backend import SconeTable
    max_n, d = 3, 768
    n = WS.N_ROWS[max_n]
    rng = np.random.default_rng(17)
    w = BF.stored(rng.standard_normal((n, d)).astype(np.float32))
    tables = [SconeTable(max_n, n, dim=d, table_format="bf16", **kw)
              for kw in (dict(placement="pinned_host", hot_rows=16, stage_tokens=128), dict())]
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    ids = np.arange(n, dtype=np.int64)                          # every row: both sides of the hot head
    g = rng.standard_normal((len(ids), d)).astype(np.float32)
    state = [torch.zeros(n, device="cuda") for _ in tables]
    outs = []
    for t, s in zip(tables, state):
        t.index_build(*WS._vocabulary(max_n))
        t.store_f32(torch.from_numpy(w))
        first = t.embed(tok).cpu()
        _lean(t, ids, g, kind="rowwise_adagrad", row_state=s, weight_decay=0.01)
        outs.append((first, t.embed(tok).cpu(), _bits_of(t), s.cpu().numpy()))
    assert tables[0].stage_counters()["chunks"] > 0, "the staged pipeline did not run"
    (f0, a0, b0, s0), (f1, a1, b1, s1) = outs
    assert torch.equal(f0, f1) and not torch.equal(f0, a0), "the lookup does not see the step"
    assert torch.equal(a0, a1), "the staged table serves rows from before the step"
    want, want_s, _, _, _ = LF.apply_bf16("rowwise_adagrad", _scalars("rowwise_adagrad", 0.01), ids, g, BF.to_bf16_bits(w),
                                          np.zeros(n, dtype=np.float32), rounding="stochastic", seed=SEED, step_no=1)
    assert np.array_equal(b0, want) and np.array_equal(b1, want) and E.same_bits(s0, want_s) and E.same_bits(s1, want_s)


# ------------------------------------------------------------------ 8. refusals
def test_refusals():
    from scone_amd import _lib
    from scone_amd.hip_backend import SconeTable
    d = 16
    w = torch.zeros((N, d), device="cuda")
    s = torch.zeros(N, device="cuda")
    ids = torch.arange(4, device="cuda")
    g = torch.ones((4, d), device="cuda")
    i8, f32, b16 = TO._table("int8", d), TO._table("fp32", d), TO._table("bf16", d)
    stored = [t.download(0, N)[0].copy() for t in (i8, f32, b16)]
    with pytest.raises(ValueError, match="needs row_state"):
        b16.opt_step_lean(ids, g, kind="rowwise_adagrad", lr=0.1)
    with pytest.raises(ValueError, match="row_state"):
        b16.opt_step_lean(ids, g, kind="rowwise_adagrad", lr=0.1, row_state=s[:10])
    with pytest.raises(ValueError, match="master"):
        i8.opt_step_lean(ids, g, kind="sgd", lr=0.1, master=w[:10])
    with pytest.raises(ValueError, match="master"):
        i8.opt_step_lean(ids, g, kind="sgd", lr=0.1, master=w.cpu())
    with pytest.raises(ValueError, match="in place"):
        i8.opt_step_lean(ids, g, kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="stochastic"):
        i8.opt_step_lean(ids, g, kind="sgd", lr=0.1, master=w, rounding="stochastic")
    with pytest.raises(ValueError, match="stochastic"):
        f32.opt_step_lean(ids, g, kind="sgd", lr=0.1, rounding="stochastic")
    with pytest.raises(ValueError, match="kind"):
        b16.opt_step_lean(ids, g, kind="adam", lr=0.1)
    with pytest.raises(ValueError, match="rounding"):
        b16.opt_step_lean(ids, g, kind="sgd", lr=0.1, rounding="up")
    with pytest.raises(ValueError, match="grad_rows"):
        b16.opt_step_lean(ids, g[:3], kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="int64"):
        b16.opt_step_lean(ids.int(), g, kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="finite"):
        b16.opt_step_lean(ids, g, kind="sgd", lr=float("nan"))
    # the library's own refusals, past the Python checks
    lib = _lib.lib()
    P = lambda t: t.data_ptr()                                   # noqa: E731

    def cfg(**kw):
        hp = dict(struct_size=64, kind=_lib.LEAN_ROWWISE_ADAGRAD, rounding=0, reserved=0, lr=0.1, eps=1e-10, weight_decay=0.0,
                  grad_scale=1.0, seed=0, step=1)
        hp.update(kw)
        return _lib.LeanCfg(**hp)

    def refused(t, c, ids_=P(ids), g_=P(g), master=None, state=P(s), word=b""):
        rc = lib.scone_opt_step_lean(t._h, c, ids_, g_, 4, master, state, None)
        return rc == _lib.EINVAL and word in lib.scone_last_error(t._h)

    assert refused(b16, None, word=b"null cfg")
    assert refused(b16, cfg(), ids_=None, word=b"null") and refused(b16, cfg(), g_=None, word=b"null")
    assert refused(b16, cfg(), state=None, word=b"d_row_state")
    assert refused(b16, cfg(kind=2), word=b"kind") and refused(b16, cfg(rounding=2), word=b"rounding")
    assert refused(b16, cfg(struct_size=60), word=b"struct_size") and refused(b16, cfg(reserved=1), word=b"reserved")
    for name in ("lr", "eps", "weight_decay", "grad_scale"):
        assert refused(b16, cfg(**{name: float("inf")}), word=b"finite")
    for fmt, name in (("int8", b"int8"), ("fp16", b"fp16"), ("int4", b"int4"), ("mxfp4", b"mxfp4")):
        t = TO._table(fmt, 128)
        g128 = torch.ones((4, 128), device="cuda")
        assert refused(t, cfg(), g_=P(g128), word=name), fmt
    assert refused(f32, cfg(rounding=1), word=b"fp32") and refused(b16, cfg(rounding=1), master=P(w), word=b"master")
    index_only = SconeTable(3, N)                                  # dim == 0
    assert refused(index_only, cfg(), word=b"dim == 0")
    assert lib.scone_opt_step_lean(b16._h, cfg(), None, None, 0, None, None, None) == _lib.OK, "n == 0 is a no-op"
    torch.cuda.synchronize()
    assert bool((w == 0).all()) and bool((s == 0).all()), "a refused call wrote"
    for t, rows in zip((i8, f32, b16), stored):
        assert t.status() == 0 and np.array_equal(t.download(0, N)[0], rows), "a refused call wrote"


# ------------------------------------------------------------------ 9. the modules and FGramOptimizer
def _cache(fmt, d, max_n, rows):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = WS._vocabulary(max_n)
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt)
    cache.cache_embeddings(list(range(rows.shape[0])), rows, verbose=False)
    return cache


def _in_place_loop(iters=3, resume_at=None):
    """`iters` iterations of forward / backward / step / zero_grad on the WS vocabulary (max_n = 3), the 9 x 37 batch, a bf16 cache
    at d = 64, row-wise Adagrad with stochastic rounding.  Returns the table's bits after every iteration and the bits of the last
    forward.  resume_at = k: after iteration k the optimizer is rebuilt from state_dict()."""
    from scone_amd import FGramOptimizer, InPlaceFGramTable
    from scone_amd.hip_backend import backward_chunk
    max_n, d = 3, 64
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    off, ids = TB._lists("r37", max_n, "cover")
    n_rows = WS.N_ROWS[max_n]
    w0 = BF.stored(np.random.default_rng(31).standard_normal((n_rows, d)).astype(np.float32))
    base = TB._grad(B * T, d, "fp16", seed=5).reshape(B, T, d).cuda().requires_grad_(True)
    rid, grows = BW.backward_rows(off, ids, np.ones((B * T, d), dtype=np.float32), "mean", backward_chunk(), 0, None, n_rows)
    assert 0 < len(rid) < n_rows
    cache = _cache("bf16", d, max_n, torch.from_numpy(w0))
    fg = InPlaceFGramTable(cache)
    assert sum(p.numel() for p in fg.parameters()) == 0 and not hasattr(fg, "weight")
    hp = dict(lr=0.05, eps=1e-10, weight_decay=0.01)
    opt = FGramOptimizer(fg, "rowwise_adagrad", rounding="stochastic", seed=SEED, **hp)
    bits, s = BF.to_bf16_bits(w0), np.zeros(n_rows, dtype=np.float32)
    sc = _scalars("rowwise_adagrad", 0.01, lr=0.05, eps=1e-10)
    table = cache.to_device()
    history, last = [], None
    for it in range(1, iters + 1):
        out = fg(tok, base=base)
        fresh = _cache("bf16", d, max_n, torch.from_numpy(BF.from_bf16_bits(bits)))
        assert E.same_bits(WS._bits(out), WS._bits(fresh.embed_tokens(tok, base=base.detach()))), f"iteration {it}: the forward does not read the updated rows"
        last = WS._bits(out)
        out.sum().backward()
        assert np.array_equal(base.grad.cpu().numpy(), np.ones((B, T, d), dtype=np.float16)), "grad_base"
        base.grad = None
        got_ids, got_rows = fg.grad
        assert np.array_equal(got_ids.cpu().numpy(), rid) and E.same_bits(got_rows.cpu().numpy(), grows)
        assert opt.step() == len(rid) and opt.t == it
        opt.zero_grad()
        assert fg.grad is None and opt.step() == 0 and opt.t == it
        bits, s, _, bad, _ = LF.apply_bf16("rowwise_adagrad", sc, rid, grows, bits, s, rounding="stochastic", seed=SEED, step_no=it)
        assert not bad and table.status() == 0
        got = _bits_of(table)
        assert np.array_equal(got, bits), f"iteration {it}: table: {E.first_difference(got, bits)}"
        assert E.same_bits(opt.state2.cpu().numpy(), s) and opt.state1 is None and tuple(opt.state2.shape) == (n_rows,)
        history.append(got.copy())
        if resume_at == it:
            state = opt.state_dict()
            opt = FGramOptimizer(fg, "rowwise_adagrad", lr=123.0)      # everything comes back from the state
            opt.load_state_dict(state)
            assert opt.t == it and opt.lr == 0.05 and opt.seed == SEED and opt.rounding == "stochastic"
    return history, last


def test_in_place_module_loop_state_dict_and_determinism():
    first, out1 = _in_place_loop()
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])
    second, out2 = _in_place_loop()
    assert all(np.array_equal(x, y) for x, y in zip(first, second)), "two runs differ"
    assert np.array_equal(out1, out2)
    resumed, out3 = _in_place_loop(resume_at=2)
    assert np.array_equal(resumed[2], first[2]), "a state_dict round trip changes step 3"
    assert np.array_equal(out3, out1)


def test_in_place_module_accumulates_two_backwards():
    from scone_amd import FGramOptimizer, InPlaceFGramTable
    max_n, d = 3, 64
    n_rows = WS.N_ROWS[max_n]
    w0 = np.random.default_rng(33).standard_normal((n_rows, d)).astype(np.float32)
    fg = InPlaceFGramTable(_cache("fp32", d, max_n, torch.from_numpy(w0)))
    rng = np.random.default_rng(34)
    a_ids, b_ids = np.asarray([3, 7, 59], dtype=np.int64), np.asarray([0, 7, 20], dtype=np.int64)
    a, b = (rng.standard_normal((3, d)).astype(np.float32) for _ in range(2))
    fg._accumulate(torch.from_numpy(a_ids).cuda(), torch.from_numpy(a).cuda())
    fg._accumulate(torch.from_numpy(b_ids).cuda(), torch.from_numpy(b).cuda())
    ids, rows = fg.grad
    assert ids.cpu().tolist() == [0, 3, 7, 20, 59]
    want = np.stack([b[0], a[0], a[1] + b[1], b[2], a[2]])
    assert E.same_bits(rows.cpu().numpy(), want)
    opt = FGramOptimizer(fg, "sgd", lr=0.05)
    assert opt.step(grad_scale=0.5) == 5 and opt.state2 is None
    neww = LF.apply("sgd", _scalars("sgd", gs=0.5), ids.cpu().numpy(), want, w0)[0]
    got = fg.cache.to_device().download(0, n_rows)[0].view(np.float32)
    assert E.same_bits(got, neww)
    opt.zero_grad(set_to_none=False)
    assert fg.grad is not None and fg.grad[0].numel() == 0 and opt.step() == 0


def test_optimizer_refusals():
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    max_n, d = 3, 128
    n_rows = WS.N_ROWS[max_n]
    w0 = torch.zeros((n_rows, d))
    for fmt in ("fp16", "int8", "int4", "mxfp4"):
        with pytest.raises(ValueError, match="fp32 or bf16"):
            FGramOptimizer(InPlaceFGramTable(_cache(fmt, d, max_n, w0)), "sgd")
    fg = InPlaceFGramTable(_cache("bf16", d, max_n, w0))
    for kind in ("adam", "adagrad", "rmsprop"):
        with pytest.raises(ValueError, match="kind"):
            FGramOptimizer(fg, kind)
    with pytest.raises(ValueError, match="rounding"):
        FGramOptimizer(fg, "sgd", rounding="up")
    with pytest.raises(ValueError, match="stochastic"):
        FGramOptimizer(InPlaceFGramTable(_cache("fp32", d, max_n, w0)), "sgd", rounding="stochastic")
    with pytest.raises(ValueError, match="stochastic"):
        FGramOptimizer(TrainableFGramTable(_cache("int8", d, max_n, w0), w0.clone()), "rowwise_adagrad", rounding="stochastic")


def test_rowwise_adagrad_on_a_trainable_table_leaves_nothing_to_commit():
    from scone_amd import FGramOptimizer, TrainableFGramTable
    max_n, d = 3, 64
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    n_rows = WS.N_ROWS[max_n]
    w0 = np.random.default_rng(35).standard_normal((n_rows, d)).astype(np.float32)
    cache = _cache("int8", d, max_n, torch.from_numpy(w0))
    fg = TrainableFGramTable(cache, torch.from_numpy(w0.copy()))
    opt = FGramOptimizer(fg, "rowwise_adagrad", lr=0.05, eps=1e-10, weight_decay=0.01)
    w, s = w0, np.zeros(n_rows, dtype=np.float32)
    for it in (1, 2):
        fg(tok).sum().backward()
        rid, grows = fg.weight.grad._indices()[0].cpu().numpy(), fg.weight.grad._values().cpu().numpy()
        assert opt.step() == len(rid) and fg.commit() == 0, "the optimizer left rows for commit()"
        opt.zero_grad()
        w, s, _, bad = LF.apply("rowwise_adagrad", _scalars("rowwise_adagrad", 0.01, lr=0.05, eps=1e-10), rid, grows, w, s)
        assert not bad and E.same_bits(fg.weight.detach().cpu().numpy(), w)
        assert tuple(opt.state2.shape) == (n_rows,) and E.same_bits(opt.state2.cpu().numpy(), s) and opt.state1 is None
        fresh = _cache("int8", d, max_n, fg.weight.detach().cpu())
        assert E.same_bits(WS._bits(fg(tok)), WS._bits(fresh.embed_tokens(tok))), "the served table is not current"
    state = opt.state_dict()
    again = FGramOptimizer(fg, "rowwise_adagrad")
    again.load_state_dict(state)
    assert again.t == 2 and torch.equal(again.state2, opt.state2)


def test_in_place_training_keeps_no_table_sized_tensor():
    """N = 65,536 rows, d = 64: what the in-place module, its optimizer and the first step keep allocated on the device is below
    N * d * 4 / 4 bytes -- a master copy alone would be N * d * 4."""
    from scone_amd import EmbeddingCache, FGramOptimizer, InPlaceFGramTable, NGramExtractor
    n, d = 65536, 64
    keys = np.stack([np.arange(n) % 256, np.arange(n) // 256], axis=1).astype(np.uint32)      # n distinct 2-grams
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, np.full(n, 2, dtype=np.uint8), max_n=2), d, table_format="bf16",
                           keep_host_copy=False)
    rows = torch.from_numpy(np.random.default_rng(36).standard_normal((n, d)).astype(np.float32))
    cache.cache_embeddings(list(range(n)), rows, verbose=False)
    table = cache.to_device()
    tok = torch.from_numpy(np.random.default_rng(37).integers(0, 256, size=(4, 64))).cuda()
    before_rows = _bits_of(table)
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    fg = InPlaceFGramTable(cache)
    opt = FGramOptimizer(fg, "rowwise_adagrad", lr=0.05, rounding="stochastic", seed=1)
    fg(tok).sum().backward()
    touched = opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - start
    print(f"kept {kept} bytes for {touched} touched rows; a master copy would be {n * d * 4}")
    assert 0 < touched <= 4 * 63 and kept < n * d * 4 // 4
    assert opt.state2.numel() == n and table.status() == 0
    assert int((_bits_of(table) != before_rows).any(axis=1).sum()) == touched
