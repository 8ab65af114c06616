"""The fused sparse optimizer step (`scone_opt_step`, `SconeTable.opt_step`, `FGramOptimizer`) against its numpy statement.

The contract (include/scone_hip.h, "optimizer step") fixes every rounding, so there is no tolerance: master and state equal
tests/opt_fixture.py's bits (`edge_fixture.same_bits`; NaN payloads are not compared), with the scalars read from
`scone_opt_scalars_of`.  Every array handed to the call sits between two runs of 64 guard rows filled with NaN that must come
back untouched, and `table.status()` is checked after every step.

Set-up of every case: N = 300 rows, random master and state, the table first stored from the master, three consecutive steps
(t = 1, 2, 3) over overlapping id sets that each hold rows 0 and N - 1.  After every step:
  1. master and state equal the fixture's bits (on the listed rows, and)
  2. every row that is not listed keeps its bits: master, state (the whole arrays are compared) and the table's download;
  3. the handle's `download()` equals, byte for byte, that of a second handle given `store_f32(w'[ids], ids=ids)`;
  4. `gather_rows(ids)` agrees between the two handles.

Shapes: the smallest at which the kernel's structure changes -- one active lane (fp32, d = 4), 20 of 64 lanes and a row maximum
over idle lanes (INT8, d = 80), one full pass of 64 lanes plus a partial one (bf16, d = 264), one and three INT4 groups and the
d = 1024 scale-slot orders, rows wider than one block of 1024 elements.  INT8 keeps a row of up to 1024 elements in registers
and reads wider rows back from the master: d = 1024 and d = 1040 sit on either side of that switch, d = 4112 far above it.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import opt_fixture as OF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only: the WS batches, their id lists, the cache builder)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, bit views)

pytestmark = pytest.mark.gpu

N, GUARD = 300, 64
HP = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8)
KINDS = ("sgd", "adagrad", "adam")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _table(fmt, d, n=N, own=None, **kw):
    from scone_amd.hip_backend import SconeTable
    lo, hi = own if own else (0, n)
    return SconeTable(3, n, dim=d, table_format=fmt, row_begin=lo, row_end=hi, **kw)


class _Guarded:
    """A device array [rows, d] between two runs of GUARD rows of NaN."""

    def __init__(self, x):
        self.rows = x.shape[0]
        self.buf = torch.full((self.rows + 2 * GUARD, x.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.rows]
        self.view.copy_(torch.from_numpy(x))
        assert self.view.is_contiguous()

    def read(self):
        host = self.buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + self.rows:]).all(), "a guard row was written"
        return host[GUARD:GUARD + self.rows]


def _id_sets(rng, lo, hi, count=100):
    """Three overlapping ascending id sets inside [lo, hi), each with the first and the last owned row."""
    pool = np.arange(lo, hi)
    common = rng.choice(pool, size=min(count // 3, len(pool)), replace=False)
    sets = []
    for _ in range(3):
        own = rng.choice(pool, size=min(count, len(pool)), replace=False)
        sets.append(np.unique(np.concatenate([own, common, [lo, hi - 1]])).astype(np.int64))
    assert len(set(map(tuple, sets))) == 3 and len(np.intersect1d(sets[0], sets[1])) > 2
    assert all(len(s) < hi - lo for s in sets), "every row is listed: nothing shows an unlisted row"
    return sets


def _same_bytes(a, b):
    return a is b or (a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape
                      and np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def _start(fmt, d, seed, n=N, own=None, table_kw=None, state=None):
    """Two handles holding the same table (stored from the master), the guarded device arrays and their host twins."""
    lo, hi = own if own else (0, n)
    rng = np.random.default_rng(seed)
    if state is None:
        w = rng.standard_normal((hi - lo, d)).astype(np.float32)
        m = (0.1 * rng.standard_normal((hi - lo, d))).astype(np.float32)
        v = (rng.standard_normal((hi - lo, d)) ** 2).astype(np.float32)
    else:
        w, m, v = state
    a, b = (_table(fmt, d, n, own, **(table_kw or {})) for _ in range(2))
    for t in (a, b):
        t.store_f32(torch.from_numpy(w), row0=lo)
    return rng, a, b, [w, m, v], [_Guarded(w), _Guarded(m), _Guarded(v)]


def _one_step(kind, a, b, host, dev, ids, g, t, wd=0.0, gs=1.0, own=None, n=N, tag=""):
    """One call on handle `a`, checked as the module docstring says; `host` is advanced to the fixture's result."""
    from scone_amd import _lib
    from scone_amd.hip_backend import opt_scalars
    lo, hi = own if own else (0, n)
    hp = dict(HP, weight_decay=wd, grad_scale=gs, step=t)
    sc = opt_scalars(kind, **hp)
    uses_m, uses_v = kind == "adam", kind != "sgd"
    want_w, want_m, want_v, applied, bad = OF.apply(kind, sc, ids, g, host[0], host[1] if uses_m else None,
                                                    host[2] if uses_v else None, lo, hi)
    before = a.download(lo, hi - lo)
    a.opt_step(torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), dev[0].view, kind=kind, state1=dev[1].view if uses_m else None,
               state2=dev[2].view if uses_v else None, **hp)
    got = [x.read() for x in dev]
    assert a.status() == (_lib.ST_BAD_ID if bad else 0), f"{tag}: status"
    # 1 + 2: the whole arrays -- the listed rows are the fixture's, every other row is the one before
    assert E.same_bits(got[0], want_w), f"{tag}: master: {E.first_difference(got[0], want_w)}"
    assert E.same_bits(got[1], want_m if uses_m else host[1]), f"{tag}: state1: {E.first_difference(got[1], want_m if uses_m else host[1])}"
    assert E.same_bits(got[2], want_v if uses_v else host[2]), f"{tag}: state2: {E.first_difference(got[2], want_v if uses_v else host[2])}"
    rest = np.setdiff1d(np.arange(lo, hi), applied) - lo
    for x, y in zip(got, host):
        assert np.array_equal(x[rest].view(np.uint32), y[rest].view(np.uint32)), f"{tag}: a row that is not listed changed"
    # 3: the served table equals a table given store_f32 of the updated rows (the GPU's own w': equal NaN payloads too)
    if len(applied):
        b.store_f32(torch.from_numpy(np.ascontiguousarray(got[0][applied - lo])), ids=torch.from_numpy(applied))
    after, ref = a.download(lo, hi - lo), b.download(lo, hi - lo)
    assert _same_bytes(after[0], ref[0]) and _same_bytes(after[1], ref[1]), f"{tag}: the served table differs from store_f32's"
    assert np.array_equal(after[0][rest], before[0][rest]), f"{tag}: a table row that is not listed changed"
    assert before[1] is None or np.array_equal(after[1][rest].view(np.uint8), before[1][rest].view(np.uint8)), f"{tag}: scales"
    # 4: the dequantised rows
    if len(applied):
        ga, gb = (t_.gather_rows(torch.from_numpy(applied)).cpu().numpy() for t_ in (a, b))
        assert E.same_bits(ga, gb), f"{tag}: gather_rows"
    assert a.status() == 0 and b.status() == 0
    host[0] = want_w
    if uses_m:
        host[1] = want_m
    if uses_v:
        host[2] = want_v
    return applied


def _three_steps(fmt, d, kind, wd, gs, seed=0, **kw):
    rng, a, b, host, dev = _start(fmt, d, 1000 * d + seed, **{k: v for k, v in kw.items() if k in ("n", "own", "table_kw")})
    own, n = kw.get("own"), kw.get("n", N)
    lo, hi = own if own else (0, n)
    sets = kw.get("id_sets") or _id_sets(rng, lo, hi)
    for t, ids in enumerate(sets, start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        _one_step(kind, a, b, host, dev, ids, g, t, wd, gs, own, n, tag=f"{fmt}-d{d}-{kind}-wd{wd}-gs{gs}-t{t}")
    return host


# ------------------------------------------------------------------ 1. formats and widths
FORMAT_CASES = [("fp32", 4), ("fp16", 8), ("int8", 16), ("int8", 80), ("bf16", 264), ("int4", 128), ("int4", 384), ("int4", 1024),
                ("mxfp4", 128), ("mxfp4", 1024), ("int8", 1024), ("int8", 1040), ("int8", 4112), ("int4", 8192)]


@pytest.mark.parametrize("fmt,d", FORMAT_CASES, ids=[f"{f}-d{d}" for f, d in FORMAT_CASES])
def test_formats_and_widths(fmt, d):
    _three_steps(fmt, d, "adam", 0.01, 1.0)


# ------------------------------------------------------------------ 2. kinds, decay, gradient scale
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt,d", [("int8", 80), ("fp32", 4)])
def test_kinds_decay_and_grad_scale(fmt, d, kind, wd, gs):
    _three_steps(fmt, d, kind, wd, gs, seed=7)


# ------------------------------------------------------------------ 3. U, and a grid of two workgroups
def test_row_counts():
    fmt, d, kind = "int8", 80, "adam"
    rng, a, b, host, dev = _start(fmt, d, 5)
    sets = [np.zeros(0, dtype=np.int64), np.asarray([N - 1], dtype=np.int64), np.asarray([0, 150, N - 1], dtype=np.int64),
            np.sort(rng.choice(N, size=257, replace=False)).astype(np.int64)]
    assert [len(s) for s in sets] == [0, 1, 3, 257]
    for t, ids in enumerate(sets, start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        _one_step(kind, a, b, host, dev, ids, g, t, 0.01, 1.0, tag=f"U{len(ids)}")


def test_every_wave_takes_many_rows(monkeypatch):
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "2")             # read at create: 8 waves walk the 257 rows
    fmt, d, kind = "int8", 80, "adam"
    rng, a, b, host, dev = _start(fmt, d, 6)
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    for t in (1, 2):
        ids = np.sort(rng.choice(N, size=257, replace=False)).astype(np.int64)
        g = rng.standard_normal((257, d)).astype(np.float32)
        _one_step(kind, a, b, host, dev, ids, g, t, 0.01, 1.0, tag=f"capped-t{t}")


# ------------------------------------------------------------------ 4. edge values
def _edge_inputs(rows, d=64, seed=3):
    """g, w, m, v [rows, 64]; the class of a column is j % 16 (see the comments): +-0, the smallest subnormal, 2^-126, 1e38 (g * g
    overflows: the step is x / inf = 0), +-inf and NaN in g and in w, v = 0 with g = 0 (sqrt(0) + eps), products that are
    subnormal, and ordinary values whose square roots and quotients are not representable."""
    rng = np.random.default_rng(seed)
    f = np.float32
    g = rng.standard_normal((rows, d)).astype(f)
    w = rng.standard_normal((rows, d)).astype(f)
    m = (0.1 * rng.standard_normal((rows, d))).astype(f)
    v = (rng.standard_normal((rows, d)) ** 2).astype(f)
    sign = rng.choice(np.asarray([-1.0, 1.0], dtype=f), size=(rows, d))
    k = rng.integers(1, 9, size=(rows, d)).astype(f)
    tiny, fmin = f(2.0 ** -149), f(2.0 ** -126)
    for j in range(d):
        c = j % 16
        col = slice(j, j + 1)
        s, kk = sign[:, col], k[:, col]
        if c == 0:
            g[:, col], m[:, col], v[:, col] = f(0.0), f(0.0), f(0.0)
        elif c == 1:
            g[:, col], m[:, col], v[:, col] = f(-0.0), f(-0.0), f(0.0)
            w[::2, col] = f(-0.0)
        elif c == 2:
            g[:, col], w[:, col], m[:, col], v[:, col] = s * tiny, s * kk * tiny, s * tiny, tiny
        elif c == 3:
            g[:, col], w[:, col], m[:, col], v[:, col] = s * fmin, s * kk * fmin, s * fmin, fmin
        elif c == 4:
            g[:, col] = s * f(1e38)
        elif c == 5:
            g[:, col] = s * f(np.inf)
        elif c == 6:
            g[::2, col] = f(np.nan)
        elif c == 7:
            w[:, col] = s * f(np.inf)
        elif c == 8:
            w[::3, col] = f(np.nan)
            v[1::3, col] = f(np.inf)
        elif c == 9:
            g[:, col], w[:, col] = s * kk * f(2.0 ** -125), s * kk * f(2.0 ** -120)      # alpha * g and decay * w are subnormal
        elif c == 10:
            v[:, col], m[:, col] = f(3.0), f(1.0) / f(3.0)
        elif c == 11:
            w[:, col] = s * f(3e38)                                                     # w - step stays finite or not, by one rounding
    return g, w, m, v


@pytest.mark.parametrize("fmt", ["fp32", "int8"])
@pytest.mark.parametrize("kind", KINDS)
def test_edge_values(fmt, kind):
    from scone_amd.hip_backend import opt_scalars
    rows, d = 48, 64
    g, w, m, v = _edge_inputs(rows)
    ids = np.arange(rows, dtype=np.int64)
    rng, a, b, host, dev = _start(fmt, d, 0, n=rows, state=(w, m, v))
    # the plain update first (an infinite weight stays infinite), then decay and a gradient scale from the state that step left
    for t, wd, gs in ((1, 0.0, 1.0), (2, 0.01, 0.5)):
        sc = opt_scalars(kind, **dict(HP, weight_decay=wd, grad_scale=gs, step=t))
        args = (kind, sc, g, host[0], host[1] if kind == "adam" else None, host[2] if kind != "sgd" else None)
        outs = OF.step_f32(*args)
        want = outs[0]
        # on the CPU: these inputs tell a fused multiply-add and flushed subnormals from the contract (in the master or, where
        # the weight's own rounding hides it, in the state the test compares too)
        fused, flushed = OF.step_f32(*args, fma=True), OF.step_f32(*args, ftz=True)

        def differs(other, cols=slice(None)):
            return any(x is not None and not E.same_bits(x[:, cols], y[:, cols]) for x, y in zip(other, outs))

        assert differs(fused), "a fused multiply-add would pass"
        assert differs(flushed), "flush-to-zero would pass"
        assert differs(fused, slice(12, 16)), "ordinary values do not show an FMA"
        assert np.isnan(want).any() and (want == 0).any() and (t > 1 or np.isinf(want).any())
        assert ((np.abs(want) < np.float32(2.0 ** -126)) & (want != 0)).any(), "no subnormal result"
        _one_step(kind, a, b, host, dev, ids, g, t, wd, gs, n=rows, tag=f"edge-{fmt}-{kind}-t{t}")
        assert E.same_bits(host[0], want)


# ------------------------------------------------------------------ 5. bad ids, a row-sharded handle
def test_bad_ids_are_skipped_and_reported():
    fmt, d, kind = "int8", 80, "adam"
    rng, a, b, host, dev = _start(fmt, d, 8)
    lists = [np.asarray([-1, 2, 5, 5, 9, 7, 20, 31, N], dtype=np.int64),
             np.asarray([0, 3, 3, 299, 298, N + 5, -(2 ** 40), 2 ** 40], dtype=np.int64),
             np.asarray([0, 5, 9, N - 1], dtype=np.int64)]
    want_applied = [[2, 5, 9, 20, 31], [0, 3, 299], [0, 5, 9, N - 1]]
    for t, (ids, wa) in enumerate(zip(lists, want_applied), start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        applied = _one_step(kind, a, b, host, dev, ids, g, t, 0.01, 1.0, tag=f"bad-ids-t{t}")
        assert applied.tolist() == wa


def test_row_sharded_handle():
    fmt, d, kind, own = "int4", 128, "adam", (100, 200)
    rng, a, b, host, dev = _start(fmt, d, 9, own=own)
    assert host[0].shape == (100, d)
    lists = [np.asarray([-3, 50, 99, 100, 120, 120, 150, 140, 199, 200, 250], dtype=np.int64)] + _id_sets(rng, *own, count=40)[:2]
    want_first = [100, 120, 150, 199]
    for t, ids in enumerate(lists, start=1):
        g = rng.standard_normal((len(ids), d)).astype(np.float32)
        applied = _one_step(kind, a, b, host, dev, ids, g, t, 0.01, 1.0, own=own, tag=f"shard-t{t}")
        if t == 1:
            assert applied.tolist() == want_first


# ------------------------------------------------------------------ 6. a pinned-host table with a hot head
def test_pinned_host_table():
    sets = [np.asarray([0, 10, 15, 16, 17, 40, N - 1], dtype=np.int64), np.asarray([0, 15, 16, 100, N - 1], dtype=np.int64),
            np.asarray([0, 14, 15, 16, 17, 18, 200, N - 1], dtype=np.int64)]
    _three_steps("int4", 128, "adam", 0.01, 1.0, table_kw=dict(placement="pinned_host", hot_rows=16, stage_tokens=0), id_sets=sets)


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    from scone_amd import _lib
    d = 16
    a = _table("int8", d)
    w = torch.zeros((N, d), device="cuda")
    ids = torch.arange(4, device="cuda")
    g = torch.zeros((4, d), device="cuda")
    with pytest.raises(ValueError, match="needs state1"):
        a.opt_step(ids, g, w, kind="adam", lr=0.1, state2=w.clone())
    with pytest.raises(ValueError, match="needs state2"):
        a.opt_step(ids, g, w, kind="adagrad", lr=0.1)
    with pytest.raises(ValueError, match="master"):
        a.opt_step(ids, g, w[:10], kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="master"):
        a.opt_step(ids, g, w.cpu(), kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="grad_rows"):
        a.opt_step(ids, g[:3], w, kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="int64"):
        a.opt_step(ids.int(), g, w, kind="sgd", lr=0.1)
    with pytest.raises(ValueError, match="finite"):
        a.opt_step(ids, g, w, kind="sgd", lr=float("nan"))
    with pytest.raises(ValueError, match="step >= 1"):
        a.opt_step(ids, g, w, kind="adam", lr=0.1, step=0, state1=w.clone(), state2=w.clone())
    lib = _lib.lib()
    cfg = _lib.OptCfg(64, _lib.OPT_ADAM, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1)
    rc = lib.scone_opt_step(a._h, cfg, ids.data_ptr(), g.data_ptr(), 4, w.data_ptr(), None, w.data_ptr(), None)
    assert rc == _lib.EINVAL and b"d_state1" in lib.scone_last_error(a._h)
    rc = lib.scone_opt_step(a._h, cfg, None, g.data_ptr(), 4, w.data_ptr(), w.data_ptr(), w.data_ptr(), None)
    assert rc == _lib.EINVAL and b"null" in lib.scone_last_error(a._h)
    cfg.kind = 7
    assert lib.scone_opt_step(a._h, cfg, ids.data_ptr(), g.data_ptr(), 4, w.data_ptr(), None, None, None) == _lib.EINVAL
    assert b"kind" in lib.scone_last_error(a._h)
    from scone_amd.hip_backend import SconeTable
    index_only = SconeTable(3, N)                                  # dim == 0
    cfg.kind = _lib.OPT_SGD
    assert lib.scone_opt_step(index_only._h, cfg, ids.data_ptr(), g.data_ptr(), 4, w.data_ptr(), None, None, None) == _lib.EINVAL
    assert b"dim == 0" in lib.scone_last_error(index_only._h)
    torch.cuda.synchronize()
    assert bool((w == 0).all()) and a.status() == 0, "a refused call wrote"


# ------------------------------------------------------------------ 8. the module and FGramOptimizer
def _loop(iters=3, resume_at=None):
    """`iters` iterations of forward / backward / step / zero_grad on the WS vocabulary (max_n = 3), the 9 x 37 batch, an INT8 cache
    at d = 64, Adam.  Returns the weight bits after every iteration and the bits of the last forward.  resume_at = k: after
    iteration k the optimizer and the module are rebuilt from state_dict() and the weights."""
    from scone_amd import FGramOptimizer, TrainableFGramTable
    from scone_amd.hip_backend import backward_chunk, opt_scalars
    max_n, d = 3, 64
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    off, ids = TB._lists("r37", max_n, "cover")
    n_rows = WS.N_ROWS[max_n]
    w0 = np.random.default_rng(31).standard_normal((n_rows, d)).astype(np.float32)
    base = TB._grad(B * T, d, "fp16", seed=5).reshape(B, T, d).cuda()
    rid, grows = BW.backward_rows(off, ids, np.ones((B * T, d), dtype=np.float32), "mean", backward_chunk(), 0, None, n_rows)
    assert 0 < len(rid) < n_rows

    def build(weights):
        cache = TB._cache("int8", d, max_n, "cover", torch.from_numpy(weights))
        return cache, TrainableFGramTable(cache, torch.from_numpy(weights.copy()))

    cache, fg = build(w0)
    opt = FGramOptimizer(fg, "adam", **HP)
    w, m, v = w0, np.zeros_like(w0), np.zeros_like(w0)
    bits, last = [], None
    for it in range(1, iters + 1):
        fg(tok, base=base).sum().backward()
        assert fg.weight.grad.is_sparse and fg.weight.grad.is_coalesced()
        assert opt.step() == len(rid) and opt.t == it
        opt.zero_grad()
        assert fg.weight.grad is None
        w, m, v, _, bad = OF.apply("adam", opt_scalars("adam", step=it, **HP), rid, grows, w, m, v)
        assert not bad
        got = fg.weight.detach().cpu().numpy()
        assert E.same_bits(got, w), f"iteration {it}: weight: {E.first_difference(got, w)}"
        assert E.same_bits(opt.state1.cpu().numpy(), m) and E.same_bits(opt.state2.cpu().numpy(), v)
        assert fg.commit() == 0, "the optimizer left rows for commit()"
        fresh = TB._cache("int8", d, max_n, "cover", fg.weight.detach().cpu())
        last = WS._bits(fg(tok, base=base))
        assert E.same_bits(last, WS._bits(fresh.embed_tokens(tok, base=base))), f"iteration {it}: the served table is not current"
        assert cache.table.status() == 0
        bits.append(got.copy())
        if resume_at == it:
            state = opt.state_dict()
            cache, fg = build(got)
            opt = FGramOptimizer(fg, "adam", lr=123.0)           # every hyper-parameter comes back from the state
            opt.load_state_dict(state)
            assert opt.t == it and opt.lr == HP["lr"]
    return bits, last


def test_module_loop_state_dict_and_determinism():
    first, out1 = _loop()
    assert not E.same_bits(first[0], first[1]) and not E.same_bits(first[1], first[2])
    second, out2 = _loop()
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(first, second)), "two runs differ"
    assert np.array_equal(out1.view(np.uint16), out2.view(np.uint16))
    resumed, out3 = _loop(resume_at=2)
    assert np.array_equal(resumed[2].view(np.uint32), first[2].view(np.uint32)), "a state_dict round trip changes step 3"
    assert np.array_equal(out3.view(np.uint16), out1.view(np.uint16))


def test_optimizer_takes_a_gradient_that_is_not_coalesced_and_other_kinds():
    """A caller's own sparse gradient with a repeated row is combined without coalesce(); sgd and adagrad through the class."""
    from scone_amd import FGramOptimizer, TrainableFGramTable
    from scone_amd.hip_backend import opt_scalars
    max_n, d = 3, 64
    n_rows = WS.N_ROWS[max_n]
    rng = np.random.default_rng(41)
    w0 = rng.standard_normal((n_rows, d)).astype(np.float32)
    for kind in ("sgd", "adagrad"):
        cache = TB._cache("fp16", d, max_n, "cover", torch.from_numpy(w0))
        fg = TrainableFGramTable(cache, torch.from_numpy(w0.copy()))
        opt = FGramOptimizer(fg, kind, lr=0.05, weight_decay=0.01)
        idx = np.asarray([7, 3, 7, 59], dtype=np.int64)
        vals = rng.standard_normal((4, d)).astype(np.float32)
        fg.weight.grad = torch.sparse_coo_tensor(torch.from_numpy(idx)[None], torch.from_numpy(vals), (n_rows, d)).cuda()
        assert not fg.weight.grad.is_coalesced()
        fg._touched.append(torch.from_numpy(idx).cuda())
        assert opt.step(grad_scale=0.5) == 3 and fg.commit() == 0
        rows = np.stack([vals[1], vals[0] + vals[2], vals[3]])
        sc = opt_scalars(kind, lr=0.05, weight_decay=0.01, grad_scale=0.5, step=1)
        w, _, s, _, _ = OF.apply(kind, sc, np.asarray([3, 7, 59]), rows, w0, None, np.zeros_like(w0) if kind == "adagrad" else None)
        assert E.same_bits(fg.weight.detach().cpu().numpy(), w)
        if kind == "adagrad":
            assert E.same_bits(opt.state2.cpu().numpy(), s) and opt.state1 is None
        fresh = TB._cache("fp16", d, max_n, "cover", fg.weight.detach().cpu())
        ids = torch.arange(n_rows)
        assert E.same_bits(cache.table.gather_rows(ids).cpu().numpy(), fresh.table.gather_rows(ids).cpu().numpy())
        opt.zero_grad(set_to_none=False)
        assert fg.weight.grad is not None and fg.weight.grad._nnz() == 0 and opt.step() == 0
