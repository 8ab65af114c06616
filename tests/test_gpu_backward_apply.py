"""The backward applied in place (`scone_backward_apply_lean`, `BackwardPlan.apply_lean`, `FGramOptimizer(fused_backward=True)`)
against the two calls it fuses.

The contract (include/scone_hip.h, "backward applied in place") is bit equality with `scone_backward_rows` followed by the in-place
`scone_opt_step_lean`, so there is no tolerance.  A `_Pair` holds two identically filled handles: `a` takes the fused call, `b`
the two calls with the same arguments.  Compared, bit for bit (`edge_fixture.same_bits`: NaN payloads are not compared) and over
WHOLE arrays, so that a row the plan does not list is covered by the same comparison: the downloaded table of the owned range and
the row state, which sits between guard rows of NaN that must come back untouched (test_gpu_opt_step's `_Guarded`).  A row that is
not listed must also equal what it held before, and `table.status()` must be 0 on both handles.

At d = 72 and d = 1032 the device bits are also held to the numpy statements, tests/backward_fixture.py fed into
tests/lean_fixture.py: a bug the two device roads shared would pass the pair.

Batches.  Most cases plan the caller's lists (no index needed) over `test_gpu_backward_edges._matrix_lists`: 2 C + 3 positions,
rows of 1, 3, 4, 7, .. C - 1, C, C + 1, 2 C and 2 C + 1 references (C = `scone_backward_chunk()`), so rows that take the partial
pass, with a ragged last chunk, stand next to rows that are one chunk, and one list holds an id three times.
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
import test_gpu_backward as TB  # noqa: E402  (helpers only: batches, their id lists, plans)
import test_gpu_backward_edges as GE  # noqa: E402  (helpers only: the matrix lists, the edge batch, spread gradients)
import test_gpu_opt_lean as LT  # noqa: E402  (helpers only: scalars, the module's cache)
import test_gpu_opt_step as TO  # noqa: E402  (helpers only: guarded arrays)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, bit views)

pytestmark = pytest.mark.gpu

HP = LT.HP
SEED = LT.SEED
TABLES = {"f32": ("fp32", "nearest"), "bf16": ("bf16", "nearest"), "bf16s": ("bf16", "stochastic")}
WIDTHS = (8, 72, 264, 768, 1024, 1032, 4096)
KINDS = ("sgd", "rowwise_adagrad")
GRAD_DTYPES = ("fp32", "fp16", "bf16")
REDUCES = ("mean", "sum")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _new_table(fmt, d, n, own=None, max_n=3, mode="cover", index=False, **kw):
    from scone_amd.hip_backend import SconeTable
    lo, hi = own if own else (0, n)
    t = SconeTable(max_n, n, dim=d, table_format=fmt, lookup_mode=mode, row_begin=lo, row_end=hi, **kw)
    if index:
        t.index_build(*WS._vocabulary(max_n))
    return t


def _raw(x):
    """Bits of a table download: fp32 rows as uint32, bf16 rows are uint16 already."""
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _csr_plan(off, ids):
    return lambda t: t.backward_plan_csr(torch.from_numpy(np.asarray(off)), torch.from_numpy(np.asarray(ids)))


class _Pair:
    """Two identically filled handles and their guarded row states: `a` takes the fused call, `b` the two calls."""

    def __init__(self, tab, d, n, own=None, seed=0, w=None, s=None, **table_kw):
        self.tab, self.d, self.n = tab, d, n
        self.fmt, self.rounding = TABLES[tab]
        self.lo, self.hi = own if own else (0, n)
        rows = self.hi - self.lo
        rng = np.random.default_rng(1000 * d + seed)
        w = rng.standard_normal((rows, d)).astype(np.float32) if w is None else w
        self.w = BF.stored(w) if self.fmt == "bf16" else w             # what the table holds, exactly
        self.s = (rng.standard_normal(rows) ** 2).astype(np.float32) if s is None else s
        self.a, self.b = (_new_table(self.fmt, d, n, own, **table_kw) for _ in range(2))
        for t in (self.a, self.b):
            t.store_f32(torch.from_numpy(self.w), row0=self.lo)
        self.sa, self.sb = TO._Guarded(self.s[:, None]), TO._Guarded(self.s[:, None])
        self.t = 0

    def bits(self, t):
        raw = t.download(self.lo, self.hi - self.lo)[0]
        return raw.view(np.float32) if self.fmt == "fp32" else BF.rows_as_bits(raw)

    def hp(self, kind, wd, gs, step):
        return dict(kind=kind, weight_decay=wd, grad_scale=gs, rounding=self.rounding, seed=SEED, step=step, **HP)

    def run(self, plan_of, g_t, reduce, kind, wd=0.0, gs=1.0, tag="", changes=True):
        """One fused call on `a`, the two calls on `b`, everything compared.  Returns (row ids, table bits, row state)."""
        self.t += 1
        tag = f"{tag}-{self.tab}-d{self.d}-{kind}-{reduce}-{g_t.dtype}-wd{wd}-gs{gs}-t{self.t}"
        rowwise = kind == "rowwise_adagrad"
        before, s_before = self.bits(self.b), self.sb.read()[:, 0].copy()
        assert E.same_bits(self.bits(self.a), before), f"{tag}: the two handles do not start equal"
        g = g_t.cuda()
        kw = self.hp(kind, wd, gs, self.t)
        with plan_of(self.a) as plan:
            U = plan.apply_lean(g, reduce, row_state=self.sa.view.reshape(-1) if rowwise else None, **kw)
        with plan_of(self.b) as plan:
            ids, rows = plan.rows(g, reduce)
            self.b.opt_step_lean(ids, rows, row_state=self.sb.view.reshape(-1) if rowwise else None, **kw)
        ids = ids.cpu().numpy()
        assert U == len(ids), f"{tag}: apply_lean returned {U} rows, the plan lists {len(ids)}"
        got, want = self.bits(self.a), self.bits(self.b)
        assert E.same_bits(got, want), f"{tag}: table: {E.first_difference(got, want)}"
        got_s, want_s = self.sa.read()[:, 0], self.sb.read()[:, 0]
        assert E.same_bits(got_s, want_s), f"{tag}: row state: {E.first_difference(got_s[:, None], want_s[:, None])}"
        rest = np.setdiff1d(np.arange(self.lo, self.hi), ids) - self.lo
        assert np.array_equal(_raw(got[rest]), _raw(before[rest])), f"{tag}: a table row that is not listed changed"
        assert np.array_equal(got_s[rest].view(np.uint32), s_before[rest].view(np.uint32)), f"{tag}: the state of an unlisted row changed"
        if not rowwise:
            assert np.array_equal(got_s.view(np.uint32), s_before.view(np.uint32)), f"{tag}: SGD wrote the row state"
        if changes and len(ids):
            assert not E.same_bits(got[ids - self.lo], before[ids - self.lo]), f"{tag}: no listed row changed"
        assert self.a.status() == 0 and self.b.status() == 0, f"{tag}: status"
        return ids, got, got_s


def _matrix(dtype, d):
    C = TB._chunk()
    off, ids = GE._matrix_lists(C)
    return off, ids, GE._spread_grad(len(off) - 1, d, dtype)


# ------------------------------------------------------------------ 1. widths and tiles, crossed pairwise
def _width_cases():
    """21 cases: every pair of values of any two of (d, table, kind, grad dtype, reduce) occurs (checked below)."""
    import itertools
    cases = []
    for di, d in enumerate(WIDTHS):
        for ti, tab in enumerate(TABLES):
            s = di + ti
            cases.append((d, tab, KINDS[s % 2], GRAD_DTYPES[s % 3], REDUCES[(s // 2 + ti) % 2]))
    factors = (WIDTHS, tuple(TABLES), KINDS, GRAD_DTYPES, REDUCES)
    for x, y in itertools.combinations(range(5), 2):
        assert {(c[x], c[y]) for c in cases} == set(itertools.product(factors[x], factors[y])), "not pairwise"
    return cases


@pytest.mark.parametrize("d,tab,kind,dtype,reduce", _width_cases(), ids=lambda v: str(v))
def test_widths_tables_kinds_dtypes_and_reduces(d, tab, kind, dtype, reduce):
    """d = 8: one fp16 piece, lane 0 only; 72: 9 fp16 pieces, a ragged tile; 264: 33; 768; 1024 / 1032: either side of the lean
    step's one-block boundary; 4096: the LDS ceiling.  Two calls per case: the second has weight decay and a gradient scale."""
    off, ids, g = _matrix(dtype, d)
    lens = BW.row_lengths(off, ids)[1]
    C = TB._chunk()
    assert (lens > C).sum() >= 3 and (lens <= C).sum() >= 10 and ((lens > C) & (lens % C != 0)).any()
    pair = _Pair(tab, d, GE.MATRIX_ROWS)
    pair.run(_csr_plan(off, ids), g, reduce, kind, tag="widths")
    pair.run(_csr_plan(off, ids), g, reduce, kind, wd=0.01, gs=0.5, tag="widths")


# ------------------------------------------------------------------ 2. chunk edges
@pytest.mark.parametrize("tab,kind,dtype,reduce", [("f32", "rowwise_adagrad", "fp16", "mean"), ("bf16", "sgd", "fp32", "sum"),
                                                   ("bf16s", "rowwise_adagrad", "bf16", "mean")])
def test_chunk_edges(tab, kind, dtype, reduce):
    """3 C + 7 positions; rows 1, 3, 5, 7, 9 of 12 have exactly 1, C - 1, C, C + 1 and 3 C + 5 references -- one id repeated over
    consecutive positions each -- so rows of one chunk (the last one full) stand next to rows that take the partial pass, with
    last chunks of 1 and 5 references."""
    C, d, n = TB._chunk(), 264, 12
    lens = {1: 1, 3: C - 1, 5: C, 7: C + 1, 9: 3 * C + 5}
    ntok = 3 * C + 7
    off, ids = GE._csr([[r for r, k in lens.items() if 1 <= p <= k] for p in range(ntok)])
    rid, got_lens = BW.row_lengths(off, ids)
    assert dict(zip(rid.tolist(), got_lens.tolist())) == lens and 300 < ntok < 1000
    g = TB._grad(ntok, d, dtype, seed=2)
    pair = _Pair(tab, d, n, seed=2)
    with _csr_plan(off, ids)(pair.a) as plan:
        assert plan.n_rows == 5 and plan.n_refs == sum(lens.values())
    listed, _, _ = pair.run(_csr_plan(off, ids), g, reduce, kind, wd=0.01, tag="chunk-edges")
    assert listed.tolist() == sorted(lens)


# ------------------------------------------------------------------ 3. against the numpy statements
@pytest.mark.parametrize("d,tab,kind,dtype,reduce", [(72, "f32", "rowwise_adagrad", "fp16", "mean"), (72, "bf16s", "sgd", "bf16", "sum"),
                                                     (1032, "bf16s", "rowwise_adagrad", "fp16", "mean"), (1032, "f32", "sgd", "fp32", "sum"),
                                                     (1032, "bf16", "rowwise_adagrad", "bf16", "sum")])
def test_device_bits_equal_the_fixtures(d, tab, kind, dtype, reduce):
    """`backward_fixture.backward_rows` fed into `lean_fixture.apply` / `apply_bf16`: neither passes through HIP code."""
    off, ids, g = _matrix(dtype, d)
    wd, gs = 0.01, 0.5
    pair = _Pair(tab, d, GE.MATRIX_ROWS, seed=3)
    rid, grows = BW.backward_rows(off, ids, TB._g32(g), reduce, TB._chunk(), 0, None, GE.MATRIX_ROWS)
    sc = LT._scalars(kind, wd, gs)
    state = pair.s if kind == "rowwise_adagrad" else None
    if pair.fmt == "bf16":
        want, want_s, applied, bad, _ = LF.apply_bf16(kind, sc, rid, grows, BF.to_bf16_bits(pair.w), state, rounding=pair.rounding,
                                                      seed=SEED, step_no=1)
    else:
        want, want_s, applied, bad = LF.apply(kind, sc, rid, grows, pair.w, state)
    assert not bad and np.array_equal(applied, rid)
    listed, got, got_s = pair.run(_csr_plan(off, ids), g, reduce, kind, wd=wd, gs=gs, tag="fixture")
    assert np.array_equal(listed, rid)
    assert E.same_bits(got, want), f"table differs from the fixtures: {E.first_difference(got, want)}"
    if kind == "rowwise_adagrad":
        assert E.same_bits(got_s, want_s), "row state differs from the fixtures"


# ------------------------------------------------------------------ 4. a grid of one workgroup
def test_one_workgroup_takes_291_rows(monkeypatch):
    """SCONE_OPT_MAX_BLOCKS=1: four waves walk 291 touched rows (one of them through the partial pass), each wave reusing its
    LDS region row after row.  Only `a` is capped: the yardstick runs on the default grid."""
    C, d, n = TB._chunk(), 264, 300
    lists = [[p] if p < 290 else [] for p in range(2 * C + 40)]
    for p in range(3, 2 * C + 6):
        lists[p].append(299)
    lists[7] += [7, 7]
    off, ids = GE._csr(lists)
    assert len(BW.row_lengths(off, ids)[0]) == 291
    pair = _Pair("bf16s", d, n, seed=4)
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "1")             # read at create
    pair.a = _new_table("bf16", d, n)
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    pair.a.store_f32(torch.from_numpy(pair.w))
    for seed in (1, 2):
        listed, _, _ = pair.run(_csr_plan(off, ids), TB._grad(len(off) - 1, d, "fp16", seed=seed), "mean", "rowwise_adagrad",
                                wd=0.01, tag="one-workgroup")
        assert len(listed) == 291


# ------------------------------------------------------------------ 5. plans and lookup modes
@pytest.mark.parametrize("batch,max_n,mode", [("tiny", 3, "cover"), ("small", 4, "longest_suffix"), ("small", 4, "cover"),
                                              ("r37", 3, "cover")])
def test_token_plans(batch, max_n, mode):
    """A packed plan whose cu_seqlens hold empty sequences ("tiny": at the front, inside and at the end), a longest_suffix handle,
    a packed and a rectangular plan in cover mode."""
    d, n = 200, WS.N_ROWS[max_n]
    tok, cu = TB._batch(batch, max_n)
    if batch == "tiny":
        assert (np.diff(cu) == 0).sum() >= 3 and np.diff(cu)[0] == 0 and np.diff(cu)[-1] == 0
    off, ids = TB._lists(batch, max_n, mode)
    pair = _Pair("bf16s", d, n, seed=5, max_n=max_n, mode=mode, index=True)
    listed, _, _ = pair.run(lambda t: TB._plan(t, batch, max_n), TB._grad(len(tok), d, "fp16", seed=1), "mean", "rowwise_adagrad",
                            wd=0.01, tag=f"{batch}-{mode}")
    assert np.array_equal(listed, BW.row_lengths(off, ids)[0]), "the plan lists other rows than the oracle's lists"


def test_csr_plan_with_a_repeated_id_on_a_middle_third():
    """test_gpu_backward's lists: one list holds an id three times, ids of other shards everywhere, row_begin = 30."""
    C, n, d, own = TB._chunk(), 90, 200, (30, 60)
    off, ids, names = TB._csr_lists(C, n, own, np.random.default_rng(3))
    assert (ids[off[7]:off[8]] == names["triple"]).sum() == 3
    pair = _Pair("bf16s", d, n, own=own, seed=6)
    listed, _, _ = pair.run(_csr_plan(off, ids), TB._grad(len(off) - 1, d, "fp16"), "mean", "rowwise_adagrad", tag="csr-third")
    assert listed.min() >= own[0] and listed.max() < own[1] and names["triple"] in listed


# ------------------------------------------------------------------ 6. placements
def test_row_sharded_handle_has_the_unsharded_tables_bits():
    """A handle that owns rows [100, 200) of 300: its rows, stochastic bits included, are the unsharded table's for the same
    global rows (the random bits are keyed by the global row id), and equal the two calls' on a shard."""
    C, d, n, own = TB._chunk(), 264, 300, (100, 200)
    rng = np.random.default_rng(7)
    lists = [rng.choice(n, size=int(rng.integers(0, 5)), replace=False).tolist() for _ in range(2 * C + 20)]
    for p in range(1, 2 * C + 4):
        lists[p].append(150)                                    # a row of the shard that takes the partial pass
    off, ids = GE._csr(lists)
    w = rng.standard_normal((n, d)).astype(np.float32)
    s = (rng.standard_normal(n) ** 2).astype(np.float32)
    g = TB._grad(len(off) - 1, d, "fp16", seed=3)
    whole = _Pair("bf16s", d, n, w=w, s=s)
    shard = _Pair("bf16s", d, n, own=own, w=w[own[0]:own[1]], s=s[own[0]:own[1]])
    _, all_bits, all_s = whole.run(_csr_plan(off, ids), g, "mean", "rowwise_adagrad", wd=0.01, tag="whole")
    listed, bits, state = shard.run(_csr_plan(off, ids), g, "mean", "rowwise_adagrad", wd=0.01, tag="shard")
    assert len(listed) > 50 and listed.min() >= own[0] and listed.max() < own[1]
    assert np.array_equal(bits, all_bits[own[0]:own[1]]), "the shard's rows differ from the unsharded table's (local row ids were hashed?)"
    assert E.same_bits(state, all_s[own[0]:own[1]])


@pytest.mark.parametrize("tab", ["f32", "bf16s"])
def test_pinned_host_table_with_a_hot_head(tab):
    """16 hot rows in HBM, the rest in pinned host memory: touched rows on both sides of the boundary (14 .. 18), the rows at the
    boundary through the partial pass."""
    C, d, n = TB._chunk(), 264, 300
    lists = [[r for r in (0, 10, 14, 15, 16, 17, 18, 40, n - 1) if (p + r) % 3] for p in range(C + 30)]
    for p in range(C + 5):
        lists[p] += [15, 16][:1 + p % 2]
    off, ids = GE._csr(lists)
    lens = dict(zip(*[x.tolist() for x in BW.row_lengths(off, ids)]))
    assert lens[15] > C and lens[16] > C // 2 and lens[14] <= C
    pair = _Pair(tab, d, n, seed=8, placement="pinned_host", hot_rows=16, stage_tokens=0)
    for seed in (1, 2):
        pair.run(_csr_plan(off, ids), TB._grad(len(off) - 1, d, "fp16", seed=seed), "mean", "rowwise_adagrad", wd=0.01, tag="pinned")


def test_staged_prefetch_table():
    """stage_tokens > 0: the staged cache of cold rows is dropped by the call, so the next lookup reads the updated rows."""
    max_n, d = 3, 768
    n = WS.N_ROWS[max_n]
    rng = np.random.default_rng(17)
    w = BF.stored(rng.standard_normal((n, d)).astype(np.float32))
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    g = TB._grad(B * T, d, "fp16", seed=9).cuda()
    kw = dict(kind="rowwise_adagrad", weight_decay=0.01, rounding="stochastic", seed=SEED, step=1, **HP)
    outs = []
    for name, table_kw in (("staged", dict(placement="pinned_host", hot_rows=16, stage_tokens=128)), ("hbm", {}), ("two calls", {})):
        t = _new_table("bf16", d, n, max_n=max_n, index=True, **table_kw)
        t.store_f32(torch.from_numpy(w))
        state = torch.zeros(n, device="cuda")
        first = t.embed(tok).cpu()
        with t.backward_plan(tok) as plan:
            if name == "two calls":
                ids, rows = plan.rows(g, "mean")
                t.opt_step_lean(ids, rows, row_state=state, **kw)
            else:
                assert plan.apply_lean(g, "mean", row_state=state, **kw) == plan.n_rows > 16
        outs.append((first, t.embed(tok).cpu(), LT._bits_of(t), state.cpu().numpy()))
        if name == "staged":
            assert t.stage_counters()["chunks"] > 0, "the staged pipeline did not run"
        assert t.status() == 0
    (f0, a0, b0, s0), (f1, a1, b1, s1), (f2, a2, b2, s2) = outs
    assert torch.equal(f0, f1) and not torch.equal(f0, a0), "the lookup does not see the update"
    assert torch.equal(a0, a1) and torch.equal(a0, a2), "the staged table serves rows from before the update"
    assert np.array_equal(b0, b2) and np.array_equal(b1, b2) and E.same_bits(s0, s2) and E.same_bits(s1, s2)
    assert not np.array_equal(b2, BF.to_bf16_bits(w))


# ------------------------------------------------------------------ 7. edges
def test_empty_plan_is_a_no_op():
    from scone_amd import _lib
    d, n = 64, WS.N_ROWS[3]
    pair = _Pair("bf16s", d, n, seed=10, index=True)
    before = pair.bits(pair.a)
    with pair.a.backward_plan(torch.zeros((0, 5), dtype=torch.int32)) as plan:
        assert plan.n_rows == 0
        assert plan.apply_lean(torch.zeros((0, d)), "mean", row_state=pair.sa.view.reshape(-1), **pair.hp("rowwise_adagrad", 0.01, 1.0, 1)) == 0
        cfg = _lib.LeanCfg(struct_size=64, kind=_lib.LEAN_ROWWISE_ADAGRAD, rounding=1, reserved=0, lr=0.1, eps=1e-10, weight_decay=0.0,
                           grad_scale=1.0, seed=0, step=1)
        rc = _lib.lib().scone_backward_apply_lean(pair.a._h, plan._p, None, _lib.DT_F16, _lib.REDUCE_MEAN, cfg, None, None)
        assert rc == _lib.OK, "U == 0 is a no-op whatever the other pointers hold"
    all_empty = GE._csr([[] for _ in range(9)])
    with _csr_plan(*all_empty)(pair.a) as plan:
        assert plan.n_rows == 0 and plan.apply_lean(torch.zeros((9, d)), "sum", kind="sgd", lr=0.1) == 0
    assert np.array_equal(pair.bits(pair.a), before) and E.same_bits(pair.sa.read()[:, 0], pair.s) and pair.a.status() == 0


@pytest.mark.parametrize("tab,kind,reduce", [("f32", "rowwise_adagrad", "mean"), ("bf16s", "sgd", "sum"), ("bf16", "rowwise_adagrad", "sum")])
@pytest.mark.parametrize("dtype", GRAD_DTYPES)
def test_edge_values_in_grad_out_and_in_the_table(dtype, tab, kind, reduce):
    """test_gpu_backward_edges' batch: gradients of +-0, subnormals, +-inf (and inf - inf inside a chunk and across chunks), NaN
    and sums that overflow, next to ordinary columns.  The table holds `edge_fixture.table`'s values (subnormals, 3e38, +-inf,
    NaN, the fp16 / bf16 ties) in its even rows and ordinary values in its odd rows."""
    off, ids, g_t, names, _ = GE._edge_batch(dtype, TB._chunk())
    n, d = GE.EDGE_ROWS, 64
    g32 = TB._g32(g_t)
    assert np.isnan(g32).any() and np.isinf(g32).any() and (g32 == 0).any() and np.signbit(g32[g32 == 0]).any()
    assert ((g32 != 0) & (np.abs(g32) < np.float32(2.0 ** -126))).any() == (dtype != "fp16")
    w = np.random.default_rng(11).standard_normal((n, d)).astype(np.float32)
    w[::2] = E.table(n, d)[::2]
    pair = _Pair(tab, d, n, w=w)
    for wd, gs in ((0.0, 1.0), (0.01, 0.5)):
        _, got, _ = pair.run(_csr_plan(off, ids), g_t, reduce, kind, wd=wd, gs=gs, tag="edge", changes=False)
    as_f32 = got if tab == "f32" else BF.from_bf16_bits(got)
    odd = as_f32[1::2]                                              # ordinary weights: what is not finite there came from grad_out
    assert np.isnan(odd).any() and np.isfinite(odd).any() and names["nan_one_column"] % 2 == 1


def test_two_runs_from_identical_tables_give_identical_bits():
    off, ids, g = _matrix("fp16", 768)
    runs = []
    for _ in (1, 2):
        pair = _Pair("bf16s", 768, GE.MATRIX_ROWS, seed=12)
        out = [pair.run(_csr_plan(off, ids), g, "mean", "rowwise_adagrad", wd=0.01, tag="twice") for _ in (1, 2)]
        runs.append(out[-1])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32))


# ------------------------------------------------------------------ 8. refusals
def test_refusals():
    from scone_amd import _lib
    from scone_amd.hip_backend import SconeTable
    lib = _lib.lib()
    d, n = 16, 40
    off, ids = GE._csr([[1, 2], [2, 5], [7]])
    g = torch.ones((3, d), dtype=torch.float16, device="cuda")
    s = torch.zeros(n, device="cuda")
    f32, b16, other = _new_table("fp32", d, n), _new_table("bf16", d, n), _new_table("bf16", d, n)
    stored = [t.download(0, n)[0].copy() for t in (f32, b16)]
    plans = {t: _csr_plan(off, ids)(t) for t in (f32, b16, other)}

    def cfg(**kw):
        hp = dict(struct_size=64, kind=_lib.LEAN_ROWWISE_ADAGRAD, rounding=0, reserved=0, lr=0.1, eps=1e-10, weight_decay=0.0,
                  grad_scale=1.0, seed=0, step=1)
        hp.update(kw)
        return _lib.LeanCfg(**hp)

    def refused(t, c, text, plan="own", g_=g.data_ptr(), dt=_lib.DT_F16, reduce=_lib.REDUCE_MEAN, state=s.data_ptr()):
        p = plans[t]._p if plan == "own" else plan
        rc = lib.scone_backward_apply_lean(t._h, p, g_, dt, reduce, c, state, None)
        got = lib.scone_last_error(t._h)
        assert rc == _lib.EINVAL and got == b"scone_backward_apply_lean: " + text, (rc, got)

    refused(b16, None, b"null cfg")
    refused(b16, cfg(struct_size=60), b"cfg.struct_size does not match this library")
    refused(b16, cfg(kind=2), b"bad kind")
    refused(b16, cfg(rounding=2), b"bad rounding")
    refused(b16, cfg(reserved=1), b"cfg.reserved must be 0")
    for name in ("lr", "eps", "weight_decay", "grad_scale"):
        refused(b16, cfg(**{name: float("inf")}), b"lr, eps, weight_decay and grad_scale must be finite")
    index_only = SconeTable(3, n)                                  # dim == 0
    refused(index_only, cfg(), b"handle has no table (dim == 0)", plan=plans[b16]._p)
    refused(b16, cfg(), b"null plan", plan=None)
    refused(b16, cfg(), b"null pointer", g_=None)
    refused(b16, cfg(), b"the plan belongs to another handle", plan=plans[other]._p)
    refused(b16, cfg(), b"bad grad_dtype", dt=7)
    refused(b16, cfg(), b"bad reduce", reduce=7)
    for fmt in ("int8", "fp16", "int4", "mxfp4"):
        t = _new_table(fmt, 128, n)
        with _csr_plan(off, ids)(t) as plan:
            refused(t, cfg(), b"in place needs an fp32 or bf16 table, this one is " + fmt.encode(), plan=plan._p)
    refused(f32, cfg(rounding=1), b"stochastic rounding on an fp32 table: there is nothing to round")
    refused(b16, cfg(), b"row-wise Adagrad needs d_row_state (one fp32 per owned row)", state=None)
    wide = _new_table("bf16", 4104, n)
    with _csr_plan(off, ids)(wide) as plan:
        rc = lib.scone_backward_apply_lean(wide._h, plan._p, g.data_ptr(), _lib.DT_F16, _lib.REDUCE_MEAN, cfg(kind=_lib.LEAN_SGD), None, None)
        text = lib.scone_last_error(wide._h)
        assert rc == _lib.EINVAL and text.startswith(b"scone_backward_apply_lean: d > 4096") and b"scone_backward_rows" in text \
            and b"scone_opt_step_lean" in text
    # the Python layer's own
    with plans[b16] as plan:
        with pytest.raises(ValueError, match="needs row_state"):
            plan.apply_lean(g, "mean", kind="rowwise_adagrad", lr=0.1)
        with pytest.raises(ValueError, match="row_state"):
            plan.apply_lean(g, "mean", kind="rowwise_adagrad", lr=0.1, row_state=s[:10])
        with pytest.raises(ValueError, match="kind"):
            plan.apply_lean(g, "mean", kind="adam", lr=0.1)
        with pytest.raises(ValueError, match="rounding"):
            plan.apply_lean(g, "mean", kind="sgd", lr=0.1, rounding="up")
        with pytest.raises(ValueError, match="grad_out"):
            plan.apply_lean(g[:2], "mean", kind="sgd", lr=0.1)
        with pytest.raises(ValueError, match="finite"):
            plan.apply_lean(g, "mean", kind="sgd", lr=float("nan"))
    with plans[f32] as plan:
        with pytest.raises(ValueError, match="stochastic"):
            plan.apply_lean(g.float(), "mean", kind="sgd", lr=0.1, rounding="stochastic")
    i8 = _new_table("int8", d, n)
    with _csr_plan(off, ids)(i8) as plan:
        with pytest.raises(ValueError, match="fp32 or bf16"):
            plan.apply_lean(g, "mean", kind="sgd", lr=0.1)
    plans[other].close()
    torch.cuda.synchronize()
    assert bool((s == 0).all()), "a refused call wrote the row state"
    for t, rows in zip((f32, b16), stored):
        assert t.status() == 0 and np.array_equal(t.download(0, n)[0], rows), "a refused call wrote"


def test_a_wider_row_takes_the_two_calls_in_python():
    """d = 4104: the library refuses, `BackwardPlan.apply_lean` runs `rows` + `opt_step_lean` and leaves their bits."""
    off, ids, g = _matrix("fp16", 4104)
    pair = _Pair("bf16s", 4104, GE.MATRIX_ROWS, seed=13)
    pair.run(_csr_plan(off, ids), g, "mean", "rowwise_adagrad", wd=0.01, tag="wide")


# ------------------------------------------------------------------ 9. the module and FGramOptimizer
def _loop(fused, iters=3, resume_at=2):
    """`iters` iterations of forward / backward / step on the WS vocabulary (max_n = 3), the 9 x 37 batch, a bf16 cache at d = 64,
    row-wise Adagrad with stochastic rounding, weight decay and a gradient scale of 0.5.  After iteration `resume_at` the
    optimizer is rebuilt from state_dict().  Returns per iteration (table bits, state2, t, rows updated)."""
    from scone_amd import FGramOptimizer, InPlaceFGramTable
    max_n, d = 3, 64
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    n_rows = WS.N_ROWS[max_n]
    w0 = BF.stored(np.random.default_rng(31).standard_normal((n_rows, d)).astype(np.float32))
    base = TB._grad(B * T, d, "fp16", seed=5).reshape(B, T, d).cuda().requires_grad_(True)
    cache = LT._cache("bf16", d, max_n, torch.from_numpy(w0))
    fg = InPlaceFGramTable(cache)
    opt = FGramOptimizer(fg, "rowwise_adagrad", rounding="stochastic", seed=SEED, lr=0.05, eps=1e-10, weight_decay=0.01,
                         fused_backward=fused)
    assert opt.fused_backward is fused and (fg._fused_opt is opt) == fused
    table = cache.to_device()
    history = []
    for it in range(1, iters + 1):
        out = fg(tok, base=base)
        g = TB._grad(B * T, d, "fp16", seed=40 + it).reshape(B, T, d).cuda()
        if fused:
            opt.grad_scale = 0.5                                   # read at backward time
            out.backward(g)
            assert fg.grad is None, "the fused road left a gradient on the module"
            assert opt.t == it, "t advances once per backward"
            rows = opt.step()
            assert opt.t == it and opt.step() == 0, "step() only reports"
        else:
            out.backward(g)
            assert fg.grad is not None
            rows = opt.step(grad_scale=0.5)
        assert E.same_bits(WS._bits(base.grad), WS._bits(g)), "grad_base"
        base.grad = None
        opt.zero_grad()
        assert fg.grad is None and table.status() == 0
        history.append((LT._bits_of(table), opt.state2.cpu().numpy(), opt.t, rows))
        if resume_at == it:
            state = opt.state_dict()
            assert state["fused_backward"] is fused
            opt = FGramOptimizer(fg, "rowwise_adagrad", lr=123.0)      # everything comes back from the state
            opt.load_state_dict(state)
            assert opt.fused_backward is fused and (fg._fused_opt is opt) == fused and opt.t == it and opt.lr == 0.05
    return history


def test_module_loop_equals_the_unfused_loop():
    fused, plain = _loop(True), _loop(False)
    assert not np.array_equal(plain[0][0], plain[1][0]) and not np.array_equal(plain[1][0], plain[2][0])
    for it, ((fb, fs, ft, fr), (pb, ps, pt, pr)) in enumerate(zip(fused, plain), start=1):
        assert np.array_equal(fb, pb), f"iteration {it}: table: {E.first_difference(fb, pb)}"
        assert E.same_bits(fs, ps), f"iteration {it}: state2"
        assert ft == pt == it and fr == pr > 0


def test_two_backwards_are_two_updates():
    from scone_amd import FGramOptimizer, InPlaceFGramTable
    max_n, d = 3, 64
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    w0 = np.random.default_rng(33).standard_normal((WS.N_ROWS[max_n], d)).astype(np.float32)
    tables = []
    for fused in (True, False):
        fg = InPlaceFGramTable(LT._cache("fp32", d, max_n, torch.from_numpy(w0)))
        opt = FGramOptimizer(fg, "rowwise_adagrad", lr=0.05, eps=1e-10, fused_backward=fused)
        counts = []
        for seed in (1, 2):
            fg(tok).backward(TB._grad(B * T, d, "fp32", seed=seed).reshape(B, T, d).cuda())
            if not fused:
                counts.append(opt.step())
                opt.zero_grad()
        if fused:
            assert opt.t == 2 and fg.grad is None
            counts = [opt.step()]
        assert opt.t == 2
        tables.append((fg.cache.to_device().download(0, w0.shape[0])[0].view(np.float32), opt.state2.cpu().numpy(), sum(counts)))
    assert E.same_bits(tables[0][0], tables[1][0]) and E.same_bits(tables[0][1], tables[1][1]) and tables[0][2] == tables[1][2] > 0


def test_optimizer_refusals():
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    max_n = 3
    n_rows = WS.N_ROWS[max_n]
    with pytest.raises(ValueError, match="InPlaceFGramTable"):
        FGramOptimizer(TrainableFGramTable(LT._cache("int8", 64, max_n, torch.zeros((n_rows, 64))), torch.zeros((n_rows, 64))),
                       "rowwise_adagrad", fused_backward=True)
    wide = InPlaceFGramTable(LT._cache("bf16", 4104, max_n, torch.zeros((n_rows, 4104))))
    with pytest.raises(ValueError, match="4096"):
        FGramOptimizer(wide, "sgd", fused_backward=True)
    assert FGramOptimizer(wide, "sgd").fused_backward is False and wide._fused_opt is None
    state = FGramOptimizer(InPlaceFGramTable(LT._cache("bf16", 64, max_n, torch.zeros((n_rows, 64)))), "sgd", fused_backward=True).state_dict()
    with pytest.raises(ValueError, match="4096"):
        FGramOptimizer(wide, "sgd").load_state_dict(state)


def test_the_fused_road_never_allocates_the_table_gradient():
    """4,096 bigrams at d = 2048, 8 x 1024 tokens: U * d * 4 is at least 16 MB, and the peak of backward + step is lower on the
    fused road by at least that much -- the fp32 [U, d] gradient that no longer exists."""
    from scone_amd import EmbeddingCache, FGramOptimizer, InPlaceFGramTable, NGramExtractor
    n, d, side = 4096, 2048, 64
    keys = np.stack([np.arange(n) % side, np.arange(n) // side], axis=1).astype(np.uint32)      # n distinct 2-grams
    rows = torch.from_numpy(np.random.default_rng(36).standard_normal((n, d)).astype(np.float32))
    # int32 on the device, what the library reads: the plan then makes no converted copy of the tokens (a 4 * ntok byte transient
    # that is live before the gradient rows are, so it would count in the fused arm's peak only)
    tok = torch.from_numpy(np.random.default_rng(37).integers(0, side, size=(8, 1024)).astype(np.int32)).cuda()
    peaks, touched, tables = {}, {}, {}
    for fused in (True, False):
        cache = EmbeddingCache(NGramExtractor.from_arrays(keys, np.full(n, 2, dtype=np.uint8), max_n=2), d, table_format="bf16",
                               keep_host_copy=False)
        cache.cache_embeddings(list(range(n)), rows, verbose=False)
        fg = InPlaceFGramTable(cache)
        opt = FGramOptimizer(fg, "rowwise_adagrad", lr=0.05, rounding="stochastic", seed=1, fused_backward=fused)
        opt._ensure_state()                                        # [N] fp32: allocated before the measurement on both roads
        loss = fg(tok, out_dtype=torch.float16).float().sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        loss.backward()
        touched[fused] = opt.step()
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - start
        tables[fused] = LT._bits_of(cache.to_device())
        assert fg.grad is None if fused else fg.grad is not None
        del loss, fg, opt, cache
    U = touched[True]
    print(f"U = {U}, U * d * 4 = {U * d * 4}; peak of backward + step: fused {peaks[True]}, two calls {peaks[False]}")
    assert U == touched[False] and U * d * 4 >= 16 * 2 ** 20
    assert np.array_equal(tables[True], tables[False])
    assert peaks[False] - peaks[True] >= U * d * 4
