"""The lookup's backward at value, size and grid edges, and against the forward.

tests/test_gpu_backward.py checks the order and the chunking of the sums on well-behaved batches.  This file goes where a
kernel goes wrong without such a batch noticing.  Every comparison is bit for bit (`edge_fixture.same_bits`: NaN positions equal,
payloads not compared); outputs go into the guarded buffers of tests/test_gpu_backward.py (64 guard rows, NaN and -7 prefill);
`table.status()` is read after every case; expectations come from tests/backward_fixture.py (numpy) and oracle/ref_port.py,
never through HIP code -- except in section 8, where the forward kernel is the stated oracle of the id lists.  Preconditions are
asserted on the CPU before the GPU's answer is read.  All cases but section 5 use CSR lists on a table built without an index.

1. The instance matrix.  `k_bwd_chunks<DT, NT, MEAN>` has 18 instances; NT follows from pieces = d / E (E = 4 for fp32, 8 for
   fp16 / bf16): <= 64 -> 1, <= 128 -> 2, else 4.  One CSR batch with rows of exactly 1, 3, 4, 7, 8, 15, 16, 17, 23, 31, C - 1,
   C, C + 1, 2 C and 2 C + 1 references (every tail of the walk's three loops -- blocks of 16 / NT, blocks of 4, singles --
   for every NT) and a list with an id three times, at widths whose last column tile is ragged:

       dtype        NT = 1         NT = 2    NT = 4     NT = 4, several column tiles
       fp32         d = 8, 200     d = 392   d = 520    d = 16384
       fp16, bf16   d = 8, 200     d = 776   d = 1032   d = 16384

   each with the mean and the sum: <fp32 | fp16 | bf16, 1 | 2 | 4, mean | sum> are all reached
   (tests/test_backward_host.py recomputes NT from this table with the launcher's rule).  The gradients are normals times
   2^(-10 .. 10), so that the order of a sum shows in fp16 and bf16 sums too; the `reverse` model gives other bits in every case.
2. Edge values in grad_out, d = 64, rows named in `_edge_batch`: -0 alone / in one chunk / in three chunks (want +0), +Inf and
   -Inf alone, both in one chunk, +Inf in chunk 0 and -Inf in chunk 2 (NaN made only by k_bwd_combine), max + max overflowing in
   the middle of a chain, NaN in one column, sums of the smallest denormals in one chunk and across the combine, means with
   K = 3 and K = 7 whose products are fp32 denormals or round to zero, and (X, s, -X) across the references C - 1, C, C + 1.
   What a dtype cannot express is left out and said so there: fp16 inputs cannot overflow an fp32 sum or reach an fp32
   denormal; the smallest bf16 subnormal over K does not round to zero.
3. Table sizes 1, 2, 255, 256, 257, 65535, 65536, 65537 (the sort runs over bits_for(n_rows + 1) bits, the pad key is n_rows),
   with the ids n_rows and n_rows + 1 in the lists; the one-row shards at both ends of 256 and 65536.
4. Capacity edges: one owned row of 5 C + 1 references among foreign ids; three references on 65536 owned rows; every row with
   exactly C + 1 references; all lists empty.
5. 4 * 2^20 + 2048 rows with one chunk each: more chunks than the capped grid (2^20 blocks of 4 waves, pinned by
   tests/test_backward_host.py) has waves, so the chunk loop of k_bwd_chunks runs a second time.  Every row is compared.
   Left out on purpose: the stride loop of k_bwd_combine needs more than 4 M (row, column tile) items -- at any width more
   than 10 GB of partials.
6. The caller's offsets: decreasing, negative, above offsets[ntok] in the middle (the header's clamp, tests/backward_fixture.py
   `clamp_offsets`); lists that overlap so that the references outnumber offsets[ntok] (the plan is sized by the counted
   references, not by offsets[ntok]), and so far that they reach 2^32 (refused); the Python wrapper's refusal of host offsets
   whose end lies outside ids.
7. Placement (pinned host in place, staged), three `rows()` calls enqueued back to back on one plan, a plan made on a side
   stream.
8. The forward kernel as the oracle of the lists: with the fp32 table W = [I | 0], embed(tok, reduce="sum")[p, r] is how often
   row r is in L_p (A); integer gradients make A.T @ G exact in int64 and in fp32, so it is the whole expectation of
   rows(G, "sum").  Two roads of the forward, each asserted with the launcher's rule: k_embed_fused (SCONE_FUSED_MAX_TOKENS at
   its default, d = 768) and k_match_ell + a large-batch kernel (the variable at 0, d = 64 / 200); `embed_partial` of the shard
   handles has the second road only.
9. `TrainableFGramTable`: accumulation onto a gradient that is there, `reduce="sum"`, the longest-suffix varlen base path,
   `commit()` on fp16 / bf16 / int4 / mxfp4 caches.
"""

import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import test_gpu_backward as GB  # noqa: E402  (helpers only: tables, guarded outputs, batches, lists)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, rounding, bit views)

pytestmark = pytest.mark.gpu

VOCAB, N_ROWS, DTYPES, RECTS = WS.VOCAB, WS.N_ROWS, WS.DTYPES, GB.RECTS
TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.asarray([i for x in lists for i in x], dtype=np.int64)


def _run_csr(table, off, ids, g_t, reduce, want, tag, status=0):
    """Plan the caller's lists, check U, the rows, the counts (the clamped list lengths) and the status."""
    lo, hi = BW.clamp_offsets(off)
    with table.backward_plan_csr(torch.from_numpy(np.asarray(off)), torch.from_numpy(np.asarray(ids))) as plan:
        assert plan.n_rows == len(want[0]), f"{tag}: U = {plan.n_rows}, want {len(want[0])}"
        got = GB._rows(plan, g_t, reduce, table.dim)
        counts = plan.counts().cpu().numpy()
    GB._check(got, want, tag)
    assert counts.dtype == np.int32 and np.array_equal(counts, hi - lo), f"{tag}: K_p is the clamped list length"
    assert table.status() == status and table.status() == 0
    return got


# ------------------------------------------------------------------ 1. the instance matrix
INSTANCE_WIDTHS = {"fp32": (8, 200, 392, 520, 16384), "fp16": (8, 200, 776, 1032, 16384), "bf16": (8, 200, 776, 1032, 16384)}
INSTANCE_CASES = [(dtype, d, reduce) for dtype in ("fp32", "fp16", "bf16") for d in INSTANCE_WIDTHS[dtype] for reduce in ("mean", "sum")]
MATRIX_ROWS = 40


def matrix_lengths(C):
    return (1, 3, 4, 7, 8, 15, 16, 17, 23, 31, C - 1, C, C + 1, 2 * C, 2 * C + 1)


@functools.lru_cache(maxsize=None)
def _matrix_lists(C):
    """Row 2 j + 1 is in the list of every position p < matrix_lengths(C)[j] (the rows share their positions: ntok stays small
    at d = 16384); row 36 three times in the list of position 2 and once in that of position 9; two empty lists at the end."""
    lens = matrix_lengths(C)
    ntok = max(lens) + 2
    lists = [[2 * j + 1 for j, n in enumerate(lens) if p < n] for p in range(ntok)]
    lists[2] = lists[2][:3] + [36, 36] + lists[2][3:] + [36]
    lists[9].insert(0, 36)
    return _csr(lists)


@functools.lru_cache(maxsize=4)
def _spread_grad(ntok, d, dtype):
    """Normals times 2^(-10 .. 10), rounded once to the dtype: sums of these round in fp32 whatever the dtype."""
    rng = np.random.default_rng(31 * d + ntok)
    g = rng.standard_normal((ntok, d)).astype(np.float32) * np.exp2(rng.integers(-10, 11, size=(ntok, d))).astype(np.float32)
    return WS._to(g, DTYPES[dtype])


@pytest.mark.parametrize("dtype,d,reduce", INSTANCE_CASES, ids=[f"{a}-d{b}-{c}" for a, b, c in INSTANCE_CASES])
def test_every_instance_of_the_chunk_kernel(dtype, d, reduce):
    C = GB._chunk()
    off, ids = _matrix_lists(C)
    ntok = len(off) - 1
    rid, lens = BW.row_lengths(off, ids)
    assert sorted(lens.tolist()) == sorted(matrix_lengths(C) + (4,)) and ntok == 2 * C + 3
    assert BW.positions_with_a_duplicate(off, ids) == 1 and off[-1] == off[-3]
    g = _spread_grad(ntok, d, dtype)
    want = BW.backward_rows(off, ids, GB._g32(g), reduce, C, 0, None, MATRIX_ROWS)
    rev = BW.backward_rows(off, ids, GB._g32(g), reduce, C, 0, None, MATRIX_ROWS, reverse=True)[1]
    differ = (_u32(rev) != _u32(want[1])).any(axis=1)
    assert differ[lens >= 15].all() and not differ[lens == 1].any(), "the order inside a row does not show"
    table = GB._table(3, d, n_rows=MATRIX_ROWS, with_index=False)
    _run_csr(table, off, ids, g, reduce, want, f"matrix-{dtype}-d{d}-{reduce}")


# ------------------------------------------------------------------ 2. edge values
EDGE_ROWS, EDGE_FILL = 40, 30          # scenario rows 0 .. 15; rows 30 .. 35 fill the lists of the K = 3 and K = 7 positions


@functools.lru_cache(maxsize=None)
def _edge_batch(dtype, C):
    """(off, ids, g [ntok, 64] as a torch tensor of the dtype, names: scenario -> row).  A position lists one scenario row
    (and K - 1 filler rows).  Columns 0 .. 31 hold the scenario (small integers where it says nothing), columns 32 .. 63
    standard normals: the control next to every NaN and Inf."""
    rng = np.random.default_rng(5)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    big = {"fp32": np.finfo(np.float32).max, "bf16": np.asarray([0x7F7F0000], dtype=np.uint32).view(np.float32)[0],
           "fp16": np.float32(65504.0)}[dtype]
    unit = np.float32({"fp32": 2.0 ** -149, "bf16": 2.0 ** -133, "fp16": 2.0 ** -24}[dtype])   # the dtype's smallest subnormal
    X, s = {"fp32": (2.0 ** 24, 1.0), "bf16": (2.0 ** 24, 1.0), "fp16": (2.0 ** 15, 2.0 ** -9)}[dtype]   # s is half an ulp of X
    g3 = np.float32(1.5 * 2.0 ** -126 if dtype != "fp16" else 3 * 2.0 ** -24)       # g3 / 3 and g7 / 7: fp32 denormals (not fp16)
    g7 = np.float32(1.25 * 2.0 ** -125 if dtype != "fp16" else 5 * 2.0 ** -24)
    lists, grads, names = [], [], {}

    def add(name, v, K=1):
        names[name] = row = len(names)
        for x in v:
            lists.append([row] + [EDGE_FILL + k for k in range(K - 1)])
            grads.append(x)

    def base(n):
        v = rng.standard_normal((n, 64)).astype(np.float32)
        v[:, :32] = rng.integers(-8, 9, size=(n, 32))
        return v

    def filled(n, value):
        v = base(n)
        v[:, :32] = value
        return v

    add("negzero_single", filled(1, -0.0))
    add("negzero_chunk", filled(5, -0.0))
    add("negzero_three_chunks", filled(2 * C + 5, -0.0))
    v = base(1)
    v[0, 0:8], v[0, 8:16] = inf, -inf
    add("inf_alone", v)
    v = base(6)
    v[1, 0:16], v[4, 0:8] = inf, -inf
    add("inf_both_one_chunk", v)        # 0:8 NaN, 8:16 +Inf
    v = base(2 * C + 3)
    v[3, 0:16], v[2 * C + 1, 0:8] = inf, -inf
    add("inf_chunk0_neginf_chunk2", v)
    v = base(5)
    v[:, 0:8] = np.asarray([big, big, -big, 1, 1])[:, None]
    v[:, 8:16] = np.asarray([big, -big, big, -big, 1])[:, None]
    add("overflow_mid_chain", v)
    v = base(4)
    v[2, 17] = nan
    add("nan_one_column", v)
    add("denormal_sums", filled(9, rng.integers(-14, 15, size=(9, 32)).astype(np.float32) * unit))
    add("denormal_three_chunks", filled(2 * C + 1, rng.integers(-1, 2, size=(2 * C + 1, 32)).astype(np.float32) * unit))
    signs = np.asarray([1.0, -1.0, 1.0], dtype=np.float32)[:, None] * np.where(np.arange(32) % 2, -1.0, 1.0).astype(np.float32)
    add("mean_k3", filled(3, signs * g3), K=3)            # x - x + x: every partial sum is the denormal product or zero
    add("mean_k7", filled(3, signs * g7), K=7)
    add("mean_to_zero_k3", filled(2, rng.choice([-1.0, 1.0], size=(2, 32)).astype(np.float32) * unit), K=3)
    add("mean_to_zero_k7", filled(2, rng.choice([-1.0, 1.0], size=(2, 32)).astype(np.float32) * unit), K=7)
    v = base(C + 3)
    v[:, 0:16] = 0.0
    v[C - 1, 0:16], v[C, 0:16], v[C + 1, 0:16] = X, s, -X
    add("order_triple", v)
    raw = np.stack(grads).astype(np.float32)
    g_t = WS._to(raw, DTYPES[dtype])
    assert E.same_bits(GB._g32(g_t)[:, :32], raw[:, :32]), "a scenario value is not representable in the dtype"
    off, ids = _csr(lists)
    return off, ids, g_t, names, float(s)


@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_edge_values_in_grad_out(dtype, reduce):
    C = GB._chunk()
    off, ids, g_t, row, s = _edge_batch(dtype, C)
    g32 = GB._g32(g_t)
    want = BW.backward_rows(off, ids, g32, reduce, C, 0, None, EDGE_ROWS)
    wid, w = want
    assert np.array_equal(wid[:len(row)], np.arange(len(row))), "a scenario row is missing"
    bits = _u32(w)
    # -0 contributions give +0, alone, in a chunk and through the combine; a model whose partials start at -0 does not
    for name in ("negzero_single", "negzero_chunk", "negzero_three_chunks"):
        assert (bits[row[name], :32] == 0).all(), name
    start = BW.backward_rows(off, ids, g32, reduce, C, 0, None, EDGE_ROWS, neg_zero_start=True)[1]
    for name in ("negzero_single", "negzero_chunk"):
        assert (_u32(start)[row[name], :32] == 0x80000000).all(), name
    # Inf, Inf - Inf inside a chunk and made by the combine only, NaN in one column, all next to finite columns
    r = w[row["inf_alone"]]
    assert (r[0:8] == np.inf).all() and (r[8:16] == -np.inf).all() and np.isfinite(r[16:]).all()
    for name in ("inf_both_one_chunk", "inf_chunk0_neginf_chunk2"):
        r = w[row[name]]
        assert np.isnan(r[0:8]).all() and (r[8:16] == np.inf).all() and np.isfinite(r[16:]).all(), name
    assert 3 < C <= 2 * C + 1 - C, "+Inf (reference 3) lies in chunk 0, -Inf (reference 2 C + 1) in chunk 2: no partial is NaN"
    r = w[row["nan_one_column"]]
    assert np.isnan(r[17]) and np.isfinite(np.delete(r, 17)).all()
    r = w[row["overflow_mid_chain"]]
    if dtype == "fp16":                      # 65504 + 65504 is far below FLT_MAX: fp16 inputs cannot overflow an fp32 sum
        assert np.isfinite(r).all()
    else:                                    # max + max = +Inf, and -max does not bring it back; max - max + max - max + 1 = 1
        assert (r[0:8] == np.inf).all() and (r[8:16] == 1.0).all()
    # the order-sensitive triple: X + s rounds to X in one chain (0 at the end); the chunks give X + (s - X) = s
    r = w[row["order_triple"]]
    flat = BW.backward_rows(off, ids, g32, reduce, C, 0, None, EDGE_ROWS, chunked=False)[1]
    assert (r[0:16] == np.float32(s)).all() and (flat[row["order_triple"], 0:16] == 0).all()
    # denormals: present in the answer, and a model that flushes them gives other bits
    den = (w != 0) & (np.abs(w) < TINY)
    ftz = BW.backward_rows(off, ids, g32, reduce, C, 0, None, EDGE_ROWS, flush_denormals=True)[1]
    if dtype == "fp16":                      # the smallest fp16 subnormal is 2^-24: no product or sum of a few is an fp32 denormal
        assert not den.any()
    else:
        for name in ("denormal_sums", "denormal_three_chunks"):
            assert den[row[name], :32].sum() >= 16, name
            assert (_u32(ftz)[row[name], :32] != bits[row[name], :32]).sum() >= 16, name
        if reduce == "mean":
            for name in ("mean_k3", "mean_k7"):
                assert den[row[name], :32].all() and (ftz[row[name], :32] == 0).all(), name
            if dtype == "fp32":              # 2^-149 / 3 and / 7 are below half of 2^-149 (2^-133 / 7 is not: bf16 stays non-zero)
                for name in ("mean_to_zero_k3", "mean_to_zero_k7"):
                    at = np.flatnonzero(ids[off[:-1]] == row[name])              # the scenario's positions: its row leads their lists
                    assert len(at) == 2 and (g32[at, :32] != 0).all() and (bits[row[name], :32] == 0).all(), name
    table = GB._table(3, 64, n_rows=EDGE_ROWS, with_index=False)
    _run_csr(table, off, ids, g_t, reduce, want, f"edge-values-{dtype}-{reduce}")


# ------------------------------------------------------------------ 3. table sizes at the sort's bit edges
def _size_lists(n, C, rng):
    """Rows 0, 1, n - 2, n - 1 (where they exist), a few random rows, row n // 2 with C + 1 references, and the ids n and n + 1."""
    ntok = C + 12
    lists = [[] for _ in range(ntok)]
    for p in range(1, C + 2):
        lists[p].append(n // 2)
    for k, r in enumerate(sorted({0, 1, max(n - 2, 0), n - 1} & set(range(n)))):
        lists[k].append(r)
        lists[C + 3 + k].insert(0, r)
    for r in rng.integers(0, n, size=6).tolist():
        lists[int(rng.integers(0, ntok - 1))].append(r)
    lists[2].insert(0, n)
    lists[C + 5] += [n + 1, n]
    return _csr(lists)


def _size_cases():
    out = [(n, None) for n in (1, 2, 255, 256, 257, 65535, 65536, 65537)]
    for n in (256, 65536):
        out += [(n, (0, 1)), (n, (n - 1, n))]
    return [pytest.param(n, own, id=f"n{n}" + (f"-own{own[0]}_{own[1]}" if own else "")) for n, own in out]


@pytest.mark.parametrize("n,own", _size_cases())
def test_table_sizes_at_the_bit_edges_of_the_sort(n, own):
    from scone_amd import _lib
    C, d = GB._chunk(), 8
    off, ids = _size_lists(n, C, np.random.default_rng(n))
    lo, hi = own if own else (0, n)
    g = GB._grad(len(off) - 1, d, "fp16", seed=n % 7)
    want = BW.backward_rows(off, ids, GB._g32(g), "mean", C, lo, hi, n)
    rid, lens = BW.row_lengths(off, ids, lo, hi, n)
    assert (ids == n).sum() == 2 and (ids == n + 1).sum() == 1 and len(rid) and rid.max() < n
    if own is None:
        assert {0, n - 1} <= set(rid.tolist()) and lens.max() >= C + 1
    else:
        assert rid.tolist() == [lo] and ((ids < lo) | (ids >= hi)).sum() > C
    table = GB._table(3, d, own=own, fmt="fp16", n_rows=n, with_index=False)
    _run_csr(table, off, ids, g, "mean", want, f"size-{n}-{own}", status=_lib.ST_BAD_ID)


# ------------------------------------------------------------------ 4. capacity edges
def test_one_owned_row_among_foreign_ids():
    """owned = 1: every capacity of the plan is at its smallest; the row has 5 C + 1 references (six chunks)."""
    C, n, d, k = GB._chunk(), 90, 64, 37
    rng = np.random.default_rng(41)
    lists = [[k] for _ in range(5 * C + 1)] + [[], []]
    foreign = np.concatenate([np.arange(0, k), np.arange(k + 1, n)])
    for x in lists:
        for f in rng.choice(foreign, size=int(rng.integers(1, 3))).tolist():
            x.insert(int(rng.integers(0, len(x) + 1)), f)
    off, ids = _csr(lists)
    g = GB._grad(len(off) - 1, d, "fp16")
    want = BW.backward_rows(off, ids, GB._g32(g), "mean", C, k, k + 1, n)
    assert want[0].tolist() == [k] and (ids == k).sum() == 5 * C + 1 and (np.diff(off) >= 1).all()
    flat = BW.backward_rows(off, ids, GB._g32(g), "mean", C, k, k + 1, n, chunked=False)[1]
    assert (_u32(flat) != _u32(want[1])).any()
    table = GB._table(3, d, own=(k, k + 1), n_rows=n, with_index=False)
    _run_csr(table, off, ids, g, "mean", want, "one-owned-row")


def test_three_references_on_65536_owned_rows():
    """max_refs < owned: the segment capacity is the reference count."""
    C, n, d = GB._chunk(), 65536, 8
    off, ids = _csr([[65535], [], [0, 40000]])
    g = GB._grad(3, d, "bf16")
    want = BW.backward_rows(off, ids, GB._g32(g), "mean", C, 0, n, n)
    assert want[0].tolist() == [0, 40000, 65535]
    _run_csr(GB._table(3, d, fmt="fp16", n_rows=n, with_index=False), off, ids, g, "mean", want, "three-references")


def test_every_row_has_exactly_one_chunk_and_one_reference_more():
    """The most rows with several chunks a reference count allows: n_multi = refs / (C + 1), every chunk pair is (C, 1)."""
    C, n, d, rows = GB._chunk(), 40, 200, 12
    lists = [list(range(3, 3 + rows)) for _ in range(C + 1)]
    off, ids = _csr(lists)
    rid, lens = BW.row_lengths(off, ids)
    assert len(rid) == rows and (lens == C + 1).all()
    g = GB._grad(C + 1, d, "fp32")
    want = BW.backward_rows(off, ids, GB._g32(g), "sum", C, 0, n, n)
    rev = BW.backward_rows(off, ids, GB._g32(g), "sum", C, 0, n, n, reverse=True)[1]     # (C + 1 references in one chain give the same bits)
    assert (_u32(rev) != _u32(want[1])).any(axis=1).all(), "the order inside a row does not show"
    _run_csr(GB._table(3, d, n_rows=n, with_index=False), off, ids, g, "sum", want, "all-rows-c-plus-1")


def test_all_lists_empty():
    d, ntok = 64, 7
    off, ids = np.zeros(ntok + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    table = GB._table(3, d, n_rows=40, with_index=False)
    ids_buf = torch.full((GB.GUARD,), -7, dtype=torch.int64, device="cuda")                    # U = 0: every row is a guard row
    rows_buf = torch.full((GB.GUARD, d), float("nan"), dtype=torch.float32, device="cuda")
    with table.backward_plan_csr(torch.from_numpy(off), torch.from_numpy(ids)) as plan:
        assert plan.n_rows == 0 and plan.n_refs == 0 and plan.ntok == ntok
        got_ids, got_rows = plan.rows(GB._grad(ntok, d, "fp16"), "mean", out=(ids_buf, rows_buf))
        counts = plan.counts().cpu().numpy()
    assert tuple(got_ids.shape) == (0,) and tuple(got_rows.shape) == (0, d)
    assert bool((ids_buf == -7).all()) and bool(torch.isnan(rows_buf).all()), "rows() wrote with U = 0"
    assert counts.dtype == np.int32 and np.array_equal(counts, np.zeros(ntok, dtype=np.int32))
    assert table.status() == 0


# ------------------------------------------------------------------ 5. more chunks than the capped grid has waves
GRID_WAVES = 4 * 2 ** 20               # SCONE_MAX_BLOCKS blocks of BWD_THREADS / 64 waves: tests/test_backward_host.py pins both
GRID_ROWS = GRID_WAVES + 2048


def grid_lists(n, extra, rng):
    """Position p lists row perm[p]; `extra` positions list a second row (K = 2), which then has two references."""
    perm = rng.permutation(n).astype(np.int64)
    two = np.sort(rng.choice(n, size=extra, replace=False))
    second = rng.choice(n, size=extra, replace=False).astype(np.int64)
    K = np.ones(n, dtype=np.int64)
    K[two] = 2
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(K, out=off[1:])
    ids = np.empty(int(off[-1]), dtype=np.int64)
    ids[off[:-1]] = perm
    ids[off[:-1][two] + 1] = second
    return off, ids


def test_more_chunks_than_the_capped_grid_has_waves():
    n, d = GRID_ROWS, 8
    rng = np.random.default_rng(55)
    off, ids = grid_lists(n, 3000, rng)
    g = WS._to(rng.standard_normal((n, d), dtype=np.float32), torch.float16)
    want = BW.backward_rows_short(off, ids, GB._g32(g), "mean", 0, n, n)
    assert len(want[0]) == n > GRID_WAVES and (np.diff(off) == 2).sum() == 3000, "every row is one chunk: more chunks than waves"
    table = GB._table(3, d, fmt="fp16", n_rows=n, with_index=False)
    with table.backward_plan_csr(torch.from_numpy(off), torch.from_numpy(ids)) as plan:
        assert plan.n_rows == n and plan.n_refs == n + 3000
        got = GB._rows(plan, g, "mean", d)
    GB._check(got, want, "grid-stride")           # every row, not a sample
    assert table.status() == 0


# ------------------------------------------------------------------ 6. the caller's offsets
def _offset_cases(C):
    """Well-formed lists over 40 rows, then offsets bent in the middle.  offsets[ntok] stays the length of `ids` (or below it),
    so the clamp of csr_range (scone_backward.hip: lo into [0, total], hi into [lo, total]) keeps every read inside `ids`."""
    rng = np.random.default_rng(66)
    lists = [rng.integers(0, 40, size=int(rng.integers(0, 5))).tolist() for _ in range(30)]
    lists[4] = [7] * 9
    off, ids = _csr(lists)
    total = int(off[-1])
    out = {}
    o = off.copy(); o[10], o[11] = off[12], off[9]; out["decreasing"] = o
    o = off.copy(); o[3], o[4], o[15] = -5, -(2 ** 31), -1; out["negative"] = o
    o = off.copy(); o[6], o[20], o[21] = total + 1, 2 ** 31 - 1, total + 40; out["above_the_end"] = o
    o = off.copy(); o[1::2] = total; o[2::2] = 0; o[-1] = total; out["every_other_list_is_all_of_ids"] = o
    o = off.copy(); o[-1] = total - 9; out["end_below_ids"] = o
    return off, ids, out


@pytest.mark.parametrize("case", ["decreasing", "negative", "above_the_end", "every_other_list_is_all_of_ids", "end_below_ids"])
def test_offsets_are_clamped_as_the_header_says(case):
    C, d, n = GB._chunk(), 64, 40
    good, ids, bent = _offset_cases(C)
    off = bent[case]
    total = int(off[-1])
    lo, hi = BW.clamp_offsets(off)
    assert 0 <= total <= len(ids), "no read leaves ids: the clamp's end is inside it"
    assert not (np.array_equal(lo, good[:-1]) and np.array_equal(hi, good[1:])), "the bent offsets change no list"
    assert (lo >= 0).all() and (hi >= lo).all() and (hi <= total).all()
    if case != "end_below_ids":
        assert (off[:-1] != lo).any() or (off[1:] != hi).any(), "nothing is clamped"
    if case == "every_other_list_is_all_of_ids":
        assert (hi - lo).sum() > 10 * total, "the references do not outnumber offsets[ntok]"
    g = GB._grad(len(off) - 1, d, "fp16")
    want = BW.backward_rows(off, ids, GB._g32(g), "mean", C, 0, n, n)
    if case == "every_other_list_is_all_of_ids":
        assert BW.row_lengths(off, ids, 0, n, n)[1].max() > C
    _run_csr(GB._table(3, d, n_rows=n, with_index=False), off, ids, g, "mean", want, f"offsets-{case}")


def test_overlapping_lists_of_2_32_references_are_refused():
    """65536 lists that are each all of 65536 ids: the references are numbered in 32 bits, so the plan is refused (and the
    handle serves the next plan)."""
    from scone_amd.hip_backend import SconeInvalidArgument
    total, ntok = 65536, 2 * 65536
    off = np.zeros(ntok + 1, dtype=np.int64)
    off[1::2] = total
    off[-1] = total
    lo, hi = BW.clamp_offsets(off)
    assert int((hi - lo).sum()) == 2 ** 32
    table = GB._table(3, 8, n_rows=40, with_index=False)
    with pytest.raises(SconeInvalidArgument, match="too many references"):
        table.backward_plan_csr(torch.from_numpy(off), torch.zeros(total, dtype=torch.int32))
    with table.backward_plan_csr(torch.tensor([0, 2, 3]), torch.tensor([5, 6, 5])) as plan:
        assert plan.n_rows == 2 and plan.n_refs == 3
    assert table.status() == 0


@pytest.mark.parametrize("end", [11, -1])
def test_host_offsets_whose_end_is_outside_ids_are_refused_in_python(monkeypatch, end):
    from scone_amd import _lib
    table = GB._table(3, 64, n_rows=40, with_index=False)

    def called(*args):
        pytest.fail("scone_backward_plan_csr was called with offsets[-1] outside ids")

    monkeypatch.setattr(_lib.lib(), "scone_backward_plan_csr", called)
    with pytest.raises(ValueError, match="offsets"):
        table.backward_plan_csr(torch.tensor([0, 3, 7, end]), torch.arange(10))
    assert table.status() == 0


# ------------------------------------------------------------------ 7. placement, reuse, streams
@functools.lru_cache(maxsize=None)
def _small_rectangle(max_n):
    """The batch "small" as a rectangle: its first B * 37 tokens as [B, 37]."""
    tok, _ = GB._batch("small", max_n)
    B = len(tok) // 37
    return tok[:B * 37].reshape(B, 37)


def _placed(max_n, d, **kw):
    from scone_amd.hip_backend import SconeTable
    t = SconeTable(max_n, N_ROWS[max_n], dim=d, table_format="int8", **kw)
    t.index_build(*WS._vocabulary(max_n))
    return t


def test_plans_on_pinned_host_and_staged_tables():
    from scone_amd.hip_backend import SconeInvalidArgument
    max_n, d, C = 4, 768, GB._chunk()
    rect = _small_rectangle(max_n)
    B, T = rect.shape
    r_off, r_ids = GB._lists_of(rect.reshape(-1), np.arange(B + 1, dtype=np.int64) * T, max_n, "cover")
    tok, cu = GB._batch("small", max_n)
    v_off, v_ids = GB._lists("small", max_n, "cover")
    g_r, g_v = GB._grad(B * T, d, "fp16", seed=5), GB._grad(len(tok), d, "fp16", seed=6)
    want_r = BW.backward_rows(r_off, r_ids, GB._g32(g_r), "mean", C, 0, None, N_ROWS[max_n])
    want_v = BW.backward_rows(v_off, v_ids, GB._g32(g_v), "mean", C, 0, None, N_ROWS[max_n])
    assert BW.row_lengths(r_off, r_ids)[1].max() > C and not np.array_equal(r_off, v_off[:len(r_off)])
    tables = {"hbm": _placed(max_n, d), "pinned_host": _placed(max_n, d, placement="pinned_host", hot_rows=16),
              "staged": _placed(max_n, d, placement="pinned_host", hot_rows=16, stage_tokens=1024)}
    for name, table in tables.items():
        with table.backward_plan(torch.from_numpy(rect)) as plan:
            assert plan.n_refs == int(r_off[-1])
            GB._check(GB._rows(plan, g_r, "mean", d), want_r, f"rectangle on {name}")
            assert np.array_equal(plan.counts().cpu().numpy(), np.diff(r_off))
        if name == "staged":
            with pytest.raises(SconeInvalidArgument, match="stage_tokens"):
                table.backward_plan(torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32)))
        else:
            with table.backward_plan(torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32))) as plan:
                GB._check(GB._rows(plan, g_v, "mean", d), want_v, f"packed on {name}")
                assert np.array_equal(plan.counts().cpu().numpy(), np.diff(v_off))
        assert table.status() == 0


def test_three_calls_enqueued_back_to_back_share_the_partials():
    max_n, d, C = 4, 200, GB._chunk()
    off, ids = GB._lists("small", max_n, "cover")
    ntok = len(off) - 1
    assert (BW.row_lengths(off, ids)[1] > C).sum() >= 2, "no row goes through the partials"
    g1, g2 = GB._grad(ntok, d, "fp16", seed=1), GB._grad(ntok, d, "bf16", seed=2)
    want1 = BW.backward_rows(off, ids, GB._g32(g1), "mean", C, 0, None, N_ROWS[max_n])
    want2 = BW.backward_rows(off, ids, GB._g32(g2), "sum", C, 0, None, N_ROWS[max_n])
    assert not E.same_bits(want1[1], want2[1])
    table = GB._table(max_n, d)
    with GB._plan(table, "small", max_n) as plan:
        U = plan.n_rows
        d1, d2 = g1.cuda(), g2.cuda()
        bufs = [(torch.full((U + GB.GUARD,), -7, dtype=torch.int64, device="cuda"),
                 torch.full((U + GB.GUARD, d), float("nan"), dtype=torch.float32, device="cuda")) for _ in range(3)]
        torch.cuda.synchronize()
        for (gd, reduce), out in zip(((d1, "mean"), (d2, "sum"), (d1, "mean")), bufs):       # nothing is read back in between
            plan.rows(gd, reduce, out=out)
        got = [(i.cpu().numpy(), r.cpu().numpy()) for i, r in bufs]
    for (gi, gr), want, tag in zip(got, (want1, want2, want1), ("first", "second", "third")):
        assert (gi[U:] == -7).all() and np.isnan(gr[U:]).all(), "a guard row behind the output was written"
        GB._check((gi[:U], gr[:U]), want, f"back to back, {tag} call")
    assert E.same_bits(got[0][1], got[2][1])
    assert table.status() == 0


def test_a_plan_made_on_a_side_stream_serves_the_default_stream():
    """The plan call synchronises its own stream before it returns, so the plan is complete for every stream."""
    max_n, d = 4, 200
    off, _ = GB._lists("small", max_n, "cover")
    g = GB._grad(len(off) - 1, d, "fp16", seed=1)
    want = GB._want("small", max_n, "cover", "mean", d, "fp16", None, 1)
    table = GB._table(max_n, d)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan = GB._plan(table, "small", max_n)
    assert torch.cuda.current_stream() != side
    with plan:
        GB._check(GB._rows(plan, g, "mean", d), want, "side-stream plan")
        assert np.array_equal(plan.counts().cpu().numpy(), np.diff(off))
    assert table.status() == 0


# ------------------------------------------------------------------ 8. the forward kernel as the oracle of the lists
ORACLE_DIM = {3: 64, 4: 200}            # N = 60 and N = 200 rows: k_match_ell + the large-batch kernels whatever the batch size
FUSED_DIM = 768                         # a width k_embed_fused has (768, 1024, 1280): the road of a small batch at the default


def _identity_table(max_n, mode, own=None, d=None):
    """The fp32 table W = [I | 0]: the forward's sum over L_p is the count of every row in L_p."""
    n, d = N_ROWS[max_n], d or ORACLE_DIM[max_n]
    lo, hi = own if own else (0, n)
    W = np.zeros((n, d), dtype=np.float32)
    W[np.arange(n), np.arange(n)] = 1.0
    table = GB._table(max_n, d, mode, own=own)
    table.store_f32(torch.from_numpy(W[lo:hi]), row0=lo)
    return table


@functools.lru_cache(maxsize=None)
def _oracle_batch(batch, max_n):
    if batch == "r37bad":                        # token ids -1 and >= vocab sprinkled in
        tok, cu = GB._batch("r37", max_n)
        tok = tok.copy()
        bad = np.random.default_rng(88).choice(len(tok), size=30, replace=False)
        tok[bad[:15]], tok[bad[15:]] = -1, VOCAB + 1
        return tok, cu
    return GB._batch(batch, max_n)


@functools.lru_cache(maxsize=None)
def _int_grad(ntok, d):
    return torch.from_numpy(np.random.default_rng(ntok + d).integers(-8, 9, size=(ntok, d)).astype(np.float16))


def _counts_matrix(out, n):
    """A [ntok, n] int64 from the forward's fp32 output [.., d]: small non-negative integers, nothing beyond column n."""
    a = out.float().cpu().numpy().reshape(-1, out.shape[-1])
    assert np.array_equal(a, np.round(a)) and (a >= 0).all() and (a[:, n:] == 0).all(), "the forward's sums are no counts"
    return a[:, :n].astype(np.int64)


def _want_from_counts(A, G):
    rows = np.flatnonzero(A.any(axis=0))
    exact = A[:, rows].T @ G.numpy().astype(np.int64)
    assert np.abs(exact).max(initial=0) < 2 ** 24
    return rows.astype(np.int64), exact.astype(np.float32)


def _forward_road(monkeypatch, road, max_n, ntok):
    """The width at which the forward takes the road, asserted with the launcher's rule (walk_geometry.takes_one_launch is
    scone_embed_takes_one_launch).  SCONE_FUSED_MAX_TOKENS is read when a handle is created.  "one_launch": the variable at its
    default and d = 768, where embed / embed_varlen of these small batches run k_embed_fused, which matches inside the
    kernel.  "workspace": the variable at 0 and the widths 64 / 200, k_match_ell into the stream's workspace and a large-batch
    kernel -- the matcher the backward's plan always takes."""
    if road == "one_launch":
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
        assert WS.G.takes_one_launch("fp32", FUSED_DIM, ntok)
        return FUSED_DIM
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    d = ORACLE_DIM[max_n]
    assert not WS.G.takes_one_launch("fp32", d, ntok, fused_max_tokens=0) and not WS.G.takes_one_launch("fp32", d, ntok)
    return d


@pytest.mark.parametrize("road", ["one_launch", "workspace"])
@pytest.mark.parametrize("mode", GB.MODES)
@pytest.mark.parametrize("max_n", [3, 4])
@pytest.mark.parametrize("batch", ["r37", "r3", "small", "r37bad"])
def test_the_backward_takes_the_lists_the_forward_takes(monkeypatch, batch, max_n, mode, road):
    tok, cu = _oracle_batch(batch, max_n)
    n, d = N_ROWS[max_n], _forward_road(monkeypatch, road, max_n, len(tok))
    table = _identity_table(max_n, mode, d=d)
    if batch == "small":
        tok_t, cu_t = torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32))
        A = _counts_matrix(table.embed_varlen(tok_t, cu_t, reduce="sum"), n)
        plan = table.backward_plan(tok_t, cu_t)
    else:
        tok_t = torch.from_numpy(tok.reshape(RECTS["r37" if batch == "r37bad" else batch]))
        A = _counts_matrix(table.embed(tok_t, reduce="sum"), n)
        plan = table.backward_plan(tok_t)
    assert (A.sum(axis=1) == 0).any() and (A.sum(axis=0) == 0).any(), "no empty list, or no row without a reference"
    if mode == "cover" and batch != "r3":
        assert (A >= 2).any(), "no list holds an id twice"
    if mode == "longest_suffix":
        assert A.sum(axis=1).max() == 1
    if batch == "r37bad":
        assert (tok == -1).sum() == 15 and (tok == VOCAB + 1).sum() == 15
    G = _int_grad(len(tok), d)
    want = _want_from_counts(A, G)
    with plan:
        assert plan.n_rows == len(want[0]) and plan.n_refs == int(A.sum())
        got = GB._rows(plan, G, "sum", d)
        counts = plan.counts().cpu().numpy()
    GB._check(got, want, f"forward-oracle-{batch}-n{max_n}-{mode}-{road}")
    assert np.array_equal(counts, A.sum(axis=1))
    assert table.status() == 0


@pytest.mark.parametrize("max_n", [3, 4])
def test_shard_handles_take_the_lists_their_forward_takes(max_n):
    """A shard's forward is `embed_partial`, which has one road (k_match_ell and the workspace) whatever
    SCONE_FUSED_MAX_TOKENS holds; the unsharded A beside it comes from `embed` at a width without a one-launch kernel."""
    n, d = N_ROWS[max_n], ORACLE_DIM[max_n]
    assert not WS.G.takes_one_launch("fp32", d, RECTS["r37"][0] * RECTS["r37"][1])
    tok, _ = GB._batch("r37", max_n)
    tok_t = torch.from_numpy(tok.reshape(RECTS["r37"]))
    G = _int_grad(len(tok), d)
    whole = _counts_matrix(_identity_table(max_n, "cover").embed(tok_t, reduce="sum"), n)
    parts = np.zeros_like(whole)
    for own in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
        table = _identity_table(max_n, "cover", own)
        sums = torch.full((len(tok), d), float("nan"), dtype=torch.float32, device="cuda")
        kfull = torch.full((len(tok),), -7, dtype=torch.int32, device="cuda")
        table.embed_partial(tok_t, out=(sums, kfull))
        A = _counts_matrix(sums, n)
        assert A.any() and not A[:, :own[0]].any() and not A[:, own[1]:].any()
        want = _want_from_counts(A, G)
        with table.backward_plan(tok_t) as plan:
            assert plan.n_rows == len(want[0]) and plan.n_refs == int(A.sum())
            got = GB._rows(plan, G, "sum", d)
            counts = plan.counts().cpu().numpy()
        GB._check(got, want, f"forward-oracle-shard{own}-n{max_n}")
        assert np.array_equal(counts, whole.sum(axis=1)) and np.array_equal(counts, kfull.cpu().numpy()), "K_p is the full count"
        assert table.status() == 0
        parts += A
    assert np.array_equal(parts, whole) and (whole >= 2).any()


# ------------------------------------------------------------------ 9. the module
def _module(fmt, mode, max_n=3, d=768, seed=21):
    from scone_amd import TrainableFGramTable
    w0 = torch.from_numpy(np.random.default_rng(seed).standard_normal((N_ROWS[max_n], d)).astype(np.float32))
    cache = GB._cache(fmt, d, max_n, mode, w0)
    return cache, TrainableFGramTable(cache, w0.clone()), w0


def _sparse(grad):
    assert grad.is_sparse and grad.is_coalesced()
    return grad.indices()[0].cpu().numpy(), grad.values().cpu().numpy()


def _two_backwards(module, max_n, d, reduce="mean"):
    """r37, then the packed "small" with cu_seqlens=, with no zeroing in between; returns the two fixture results."""
    C = GB._chunk()
    B, T = RECTS["r37"]
    tok1, _ = GB._batch("r37", max_n)
    tok2, cu2 = GB._batch("small", max_n)
    g1, g2 = GB._grad(B * T, d, "fp32", seed=11), GB._grad(len(tok2), d, "fp32", seed=12)
    module(torch.from_numpy(tok1.reshape(B, T)), reduce=reduce).backward(g1.reshape(B, T, d).cuda())
    module(torch.from_numpy(tok2), cu_seqlens=cu2, reduce=reduce).backward(g2.cuda())
    mode = module.cache.lookup_mode
    return [BW.backward_rows(*GB._lists(b, max_n, mode), GB._g32(g), reduce, C, 0, None, N_ROWS[max_n])
            for b, g in (("r37", g1), ("small", g2))]


def _added_once(n, d, first, second):
    """The union of two sparse results; a row both have is first + second in fp32 (two addends: no order to choose)."""
    ids = np.union1d(first[0], second[0])
    have = [np.isin(ids, x[0]) for x in (first, second)]
    dense = [np.zeros((n, d), dtype=np.float32) for _ in range(2)]
    dense[0][first[0]], dense[1][second[0]] = first[1], second[1]
    rows = np.where((have[0] & have[1])[:, None], dense[0][ids] + dense[1][ids], np.where(have[0][:, None], dense[0][ids], dense[1][ids]))
    return ids, rows.astype(np.float32), have


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_module_accumulates_onto_a_gradient_that_is_there(reduce):
    max_n, d = 3, 768
    cache, module, _ = _module("fp32", "cover")
    first, second = _two_backwards(module, max_n, d, reduce)
    ids, rows, have = _added_once(N_ROWS[max_n], d, first, second)
    assert (have[0] & have[1]).any(), "no row is in both results"      # (at max_n = 3 the two batches touch the same 25 rows)
    assert len(ids) < N_ROWS[max_n]
    GB._check(_sparse(module.weight.grad), (ids, rows), f"module-accumulation-{reduce}")
    assert cache.table.status() == 0


def test_module_longest_suffix_with_a_base_and_cu_seqlens():
    max_n, d, C = 3, 768, GB._chunk()
    cache, module, _ = _module("fp32", "longest_suffix")
    tok, cu = GB._batch("small", max_n)
    off, ids = GB._lists("small", max_n, "longest_suffix")
    K = np.diff(off)
    assert set(np.unique(K).tolist()) == {0, 1}
    tok_t = torch.from_numpy(tok)
    base = GB._grad(len(tok), d, "fp16", seed=3).cuda().requires_grad_(True)
    g = GB._grad(len(tok), d, "fp16", seed=4)
    out = module(tok_t, base=base, cu_seqlens=cu)
    served = cache.table.embed_base_varlen(tok_t, cu, base.detach())
    assert out.dtype == torch.float16 and E.same_bits(WS._bits(out), WS._bits(served))
    out.backward(g.cuda())
    want = BW.backward_rows(off, ids, GB._g32(g), "mean", C, 0, None, N_ROWS[max_n])
    GB._check(_sparse(module.weight.grad), want, "module-longest-suffix-varlen")
    want_base = (g.float() * torch.from_numpy(K == 0)[:, None].float()).half()          # a product: -x * 0 is -0
    assert base.grad.dtype == torch.float16 and E.same_bits(WS._bits(base.grad), WS._bits(want_base))
    assert cache.table.status() == 0


@pytest.mark.parametrize("fmt", ["fp16", "bf16", "int4", "mxfp4"])
def test_commit_after_two_backwards(fmt):
    max_n, d = 3, 768
    cache, module, w0 = _module(fmt, "cover")
    first, second = _two_backwards(module, max_n, d)
    union = np.union1d(first[0], second[0])
    assert 0 < len(union) < len(first[0]) + len(second[0]), "no row is touched twice: the union is no smaller than the lists"
    assert np.array_equal(_sparse(module.weight.grad)[0], union)
    torch.optim.SGD([module.weight], lr=0.5).step()
    assert module.commit() == len(union) and module.commit() == 0
    fresh = GB._cache(fmt, d, max_n, "cover", module.weight.detach().cpu())
    tok = torch.from_numpy(GB._batch("r37", max_n)[0].reshape(RECTS["r37"]))
    tok2, cu2 = GB._batch("small", max_n)
    stale = GB._cache(fmt, d, max_n, "cover", w0)
    assert E.same_bits(WS._bits(module(tok)), WS._bits(fresh.embed_tokens(tok)))
    assert E.same_bits(WS._bits(module(torch.from_numpy(tok2), cu_seqlens=cu2)), WS._bits(fresh.embed_tokens(torch.from_numpy(tok2), cu_seqlens=cu2)))
    assert not E.same_bits(WS._bits(module(tok)), WS._bits(stale.embed_tokens(tok))), "the step did not reach the served table"
    assert cache.table.status() == 0
