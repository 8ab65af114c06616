"""The lookup's backward (`scone_backward_*`, `SconeTable.backward_plan*`, `TrainableFGramTable`) against its numpy statement.

The contract (include/scone_hip.h, "backward") fixes every rounding and the order of every sum, so there is no tolerance:
`row_ids` equal tests/backward_fixture.py's and `grad_rows` equal its bits (`edge_fixture.same_bits`), with the chunk length C
read from the library.  The expectation never passes through HIP code: the id lists come from oracle/ref_port.py, every sequence
matched on its own.  Outputs are written into buffers of U + 64 rows pre-filled with NaN (row ids: with -7); the 64 guard rows
must be untouched afterwards, and `table.status()` must be 0.

Set-up as in tests/test_gpu_select.py: the vocabularies and alphabet of tests/test_gpu_walk_shapes.py, the rectangles 9 x 37,
33 x 3 (T below max_n = 4) and 50 x 1 drawn by `np.random.default_rng(77 * T + max_n)`, the packed batches "tiny" and "small" of
tests/test_gpu_varlen.py.  `grad_out` is standard normal, rounded once to its dtype.

Preconditions, asserted on the CPU before the GPU's answer is read (cover mode): fewer distinct rows than the vocabulary has
(U < N), positions that list one id twice, and on "small" a row of more than C references; a model that walks every row's
references backwards and -- on "small" -- a model that sums a row in one chain instead of chunks give other bits.  So neither
another order nor another chunk length can pass.  50 x 1 has K in {0, 1} and exact sums: the degenerate case.  None of these
batches has a row with a single reference; the CSR case builds rows of exactly 1, C, C + 1 and 3 C + 5 references.
"""

import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches and their per-sequence id lists)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, alphabet, rounding, bit views)

pytestmark = pytest.mark.gpu

VOCAB, TOKEN_P, N_ROWS, DTYPES = WS.VOCAB, WS.TOKEN_P, WS.N_ROWS, WS.DTYPES
GUARD = 64
RECTS = {"r37": (9, 37), "r3": (33, 3), "r1": (50, 1)}
MODES = ("cover", "longest_suffix")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _chunk():
    from scone_amd.hip_backend import backward_chunk
    return backward_chunk()


# ------------------------------------------------------------------ inputs and expectations (host only)
@functools.lru_cache(maxsize=None)
def _batch(batch, max_n):
    """(tokens [total] int64, cu [n + 1] int64); a rectangle is cu = arange(B + 1) * T."""
    if batch in RECTS:
        B, T = RECTS[batch]
        rng = np.random.default_rng(77 * T + max_n)
        tok = rng.choice(VOCAB + 1, size=(B, T), p=TOKEN_P).astype(np.int64).reshape(-1)
        return tok, np.arange(B + 1, dtype=np.int64) * T
    tok, cu, _ = VL._batch(batch)
    return tok, cu


def _lists_of(tok, cu, max_n, mode):
    """CSR id lists over the flattened positions, every sequence matched on its own."""
    if mode == "cover":
        offs, ids, base = [np.zeros(1, dtype=np.int64)], [], 0
        for s in range(len(cu) - 1):
            if cu[s + 1] == cu[s]:
                continue
            off, i = VL._csr_of(tok[None, cu[s]:cu[s + 1]], max_n)
            offs.append(np.asarray(off[1:], dtype=np.int64) + base)
            ids.append(np.asarray(i, dtype=np.int64))
            base += int(off[-1])
        return np.concatenate(offs), (np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64))
    f2id = R._key_dict(*WS._vocabulary(max_n))       # the paper's lookup: zero or one id per position
    hit = []
    for s in range(len(cu) - 1):
        hit += R.paper_lookup(f2id, max_n, tok[cu[s]:cu[s + 1]].tolist())
    hit = np.asarray(hit, dtype=np.int64).reshape(-1)
    off = np.zeros(len(hit) + 1, dtype=np.int64)
    np.cumsum(hit >= 0, out=off[1:])
    return off, hit[hit >= 0]


@functools.lru_cache(maxsize=None)
def _lists(batch, max_n, mode):
    return _lists_of(*_batch(batch, max_n), max_n, mode)


@functools.lru_cache(maxsize=None)
def _grad(ntok, d, dtype, seed=0):
    """grad_out [ntok, d]: standard normal, rounded once to the dtype (a torch CPU tensor)."""
    g = np.random.default_rng(1000 * d + 7 * ntok + seed).standard_normal((ntok, d)).astype(np.float32)
    return WS._to(g, DTYPES[dtype])


def _g32(g_t):
    return g_t.float().numpy()


@functools.lru_cache(maxsize=None)
def _want(batch, max_n, mode, reduce, d, dtype, own=None, seed=0):
    off, ids = _lists(batch, max_n, mode)
    lo, hi = own if own else (0, None)
    return BW.backward_rows(off, ids, _g32(_grad(len(off) - 1, d, dtype, seed)), reduce, _chunk(), lo, hi, N_ROWS[max_n])


@functools.lru_cache(maxsize=None)
def _assert_preconditions(batch, max_n, d):
    """Cover mode, the mean of fp16 gradients (sums of a few hundred fp16 values are exact in fp32, whatever their order: the
    order shows through the mean's rounded products); see the module docstring."""
    C, reduce, dtype = _chunk(), "mean", "fp16"
    off, ids = _lists(batch, max_n, "cover")
    K = np.diff(off)
    rid, lens = BW.row_lengths(off, ids)
    if batch == "r1":
        assert set(np.unique(K).tolist()) == {0, 1}
        return
    assert 0 < len(rid) < N_ROWS[max_n]
    if batch not in ("r37", "small"):
        return
    assert lens.min() > 1, "a row with a single reference"
    assert BW.positions_with_a_duplicate(off, ids) > 0
    kmax = max_n * (max_n + 1) // 2
    if batch == "small":
        assert set(np.unique(K).tolist()) == set(range(kmax + 1))
    g32 = _g32(_grad(len(off) - 1, d, dtype))
    want = _want(batch, max_n, "cover", reduce, d, dtype)[1]
    rev = BW.backward_rows(off, ids, g32, reduce, C, reverse=True)[1]
    assert (rev.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum() > len(rid) // 2, "the order inside a row does not show"
    if batch == "small":
        assert lens.max() > C and (lens > C).sum() >= 2
        flat = BW.backward_rows(off, ids, g32, reduce, C, chunked=False)[1]
        assert (flat.view(np.uint32) != want.view(np.uint32)).any(), "the chunking does not show"


def _table(max_n, d, mode="cover", own=None, fmt="fp32", n_rows=None, with_index=True):
    from scone_amd.hip_backend import SconeTable
    n = N_ROWS[max_n] if n_rows is None else n_rows
    lo, hi = own if own else (0, n)
    t = SconeTable(max_n, n, dim=d, table_format=fmt, lookup_mode=mode, row_begin=lo, row_end=hi)
    if with_index:
        t.index_build(*WS._vocabulary(max_n))
    return t


def _plan(table, batch, max_n):
    tok, cu = _batch(batch, max_n)
    if batch in RECTS:
        return table.backward_plan(torch.from_numpy(tok.reshape(RECTS[batch])))
    return table.backward_plan(torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32)))


def _rows(plan, g_t, reduce, d):
    """The GPU's answer out of guarded buffers: (row_ids, grad_rows) as numpy."""
    U = plan.n_rows
    ids_buf = torch.full((U + GUARD,), -7, dtype=torch.int64, device="cuda")
    rows_buf = torch.full((U + GUARD, d), float("nan"), dtype=torch.float32, device="cuda")
    ids, rows = plan.rows(g_t.cuda(), reduce, out=(ids_buf, rows_buf))
    assert ids.data_ptr() == ids_buf.data_ptr() and rows.data_ptr() == rows_buf.data_ptr()
    assert tuple(ids.shape) == (U,) and tuple(rows.shape) == (U, d)
    assert bool((ids_buf[U:] == -7).all()) and bool(torch.isnan(rows_buf[U:]).all()), "a guard row behind the output was written"
    return ids.cpu().numpy(), rows.cpu().numpy()


def _differing(got, want):
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=1)).reshape(-1)
    return f"{len(bad)} of {got.shape[0]} rows differ; first: {bad[:8].tolist()}"


def _check(got, want, tag):
    (gid, grows), (wid, wrows) = got, want
    assert gid.dtype == np.int64 and np.array_equal(gid, wid), f"{tag}: row ids differ"
    assert E.same_bits(grows, wrows), f"{tag}: {_differing(grows, wrows)}"


# ------------------------------------------------------------------ 1. batches, modes, reduces, dtypes, widths
def _cases():
    out = []
    for batch in ("r37", "r3", "r1", "tiny", "small"):
        for max_n in (3, 4):
            out.append((batch, max_n, "cover", "mean", "fp16", 768))
    for batch in ("r37", "small"):                                  # both lookup modes and both reduces
        for max_n in (3, 4):
            for mode in MODES:
                for reduce in ("mean", "sum"):
                    out.append((batch, max_n, mode, reduce, "fp16", 200))
    for max_n in (3, 4):                                            # grad_out dtypes
        for dtype in ("fp32", "fp16", "bf16"):
            out.append(("r37", max_n, "cover", "mean", dtype, 768))
    for max_n in (3, 4):                                            # a partial wave, a ragged tile, the headline, above 4096 and ragged
        for d in (8, 200, 768, 4104):
            out.append(("small", max_n, "cover", "mean", "fp16", d))
    out += [("small", 3, "cover", "mean", "fp32", 200), ("small", 4, "cover", "sum", "fp32", 768),
            ("small", 3, "cover", "mean", "fp32", 4104), ("small", 4, "cover", "mean", "bf16", 4104),
            ("small", 3, "longest_suffix", "mean", "bf16", 8)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return [pytest.param(*c, id="-".join(str(x) for x in c)) for c in uniq]


@pytest.mark.parametrize("batch,max_n,mode,reduce,dtype,d", _cases())
def test_rows_equal_the_fixture(batch, max_n, mode, reduce, dtype, d):
    _assert_preconditions(batch, max_n, d)
    want = _want(batch, max_n, mode, reduce, d, dtype)
    off, _ = _lists(batch, max_n, mode)
    table = _table(max_n, d, mode)
    with _plan(table, batch, max_n) as plan:
        assert plan.n_rows == len(want[0]) and plan.n_refs == int(off[-1])
        got = _rows(plan, _grad(len(off) - 1, d, dtype), reduce, d)
        counts = plan.counts().cpu().numpy()
    _check(got, want, f"{batch}-n{max_n}-{mode}-{reduce}-{dtype}-d{d}")
    assert counts.dtype == np.int32 and np.array_equal(counts, np.diff(off))
    assert table.status() == 0


def test_public_calls_and_refusals():
    """`EmbeddingCache.embed_tokens_backward`, an empty batch, a buffer that is too small, a plan of another handle."""
    from scone_amd import EmbeddingCache, NGramExtractor, _lib
    from scone_amd.hip_backend import SconeInvalidArgument
    max_n, d = 3, 200
    keys, lens = WS._vocabulary(max_n)
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format="fp16")
    cache.cache_embeddings(list(range(N_ROWS[max_n])), torch.zeros(N_ROWS[max_n], d), verbose=False)
    for batch in ("r37", "small"):
        tok, cu = _batch(batch, max_n)
        g = _grad(len(tok), d, "bf16")
        if batch in RECTS:
            ids, rows = cache.embed_tokens_backward(torch.from_numpy(tok.reshape(RECTS[batch])), g.reshape(*RECTS[batch], d).cuda(), reduce="sum")
        else:
            ids, rows = cache.embed_tokens_backward(torch.from_numpy(tok), g.cuda(), reduce="sum", cu_seqlens=cu)
        _check((ids.cpu().numpy(), rows.cpu().numpy()), _want(batch, max_n, "cover", "sum", d, "bf16"), batch)
    table = cache.table
    with table.backward_plan(torch.zeros((0, 5), dtype=torch.int32)) as empty:
        assert empty.n_rows == 0 and empty.n_refs == 0
        ids, rows = empty.rows(torch.zeros((0, d)), "mean")
        assert ids.numel() == 0 and tuple(rows.shape) == (0, d) and empty.counts().numel() == 0
    other = _table(max_n, d)
    with _plan(table, "r37", max_n) as plan:
        small_ids = torch.full((plan.n_rows - 1,), -7, dtype=torch.int64, device="cuda")
        small_rows = torch.full((plan.n_rows - 1, d), float("nan"), device="cuda")
        with pytest.raises(IndexError):
            plan.rows(_grad(plan.ntok, d, "fp16"), "mean", out=(small_ids, small_rows))
        assert bool((small_ids == -7).all()) and bool(torch.isnan(small_rows).all()), "a refused call wrote"
        rc = _lib.lib().scone_backward_counts(other._h, plan._p, None, None)
        assert rc == _lib.EINVAL and b"another handle" in _lib.lib().scone_last_error(other._h)
    with pytest.raises(SconeInvalidArgument, match="d % 8"):
        _table(max_n, 12).backward_plan(torch.zeros((2, 3), dtype=torch.int32))
    assert table.status() == 0


# ------------------------------------------------------------------ 2. the caller's lists
def _csr_lists(C, n_rows, own, rng):
    """~4 C positions; in the owned third rows of exactly 1, C, C + 1 and 3 C + 5 references, one list with an id three times,
    ids of the other thirds everywhere, empty lists at both ends."""
    ntok = 4 * C + 10
    lo, hi = own
    lists = [[] for _ in range(ntok)]
    single, exact, over, long_, triple = lo + 1, lo + 10, lo + 11, hi - 5, lo + 3
    lists[5].append(single)
    for p in range(1, C + 1):
        lists[p].append(exact)
    for p in range(1, C + 2):
        lists[p].append(over)
    for p in range(1, 3 * C + 6):
        lists[p].append(long_)
    lists[7] += [triple] * 3
    lists[9].append(triple)
    foreign = np.concatenate([np.arange(0, lo), np.arange(hi, n_rows)])
    for p in range(1, ntok - 1):
        for f in (rng.choice(foreign, size=int(rng.integers(0, 3))) if len(foreign) else ()):
            lists[p].insert(int(rng.integers(0, len(lists[p]) + 1)), int(f))
    off = np.zeros(ntok + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids = np.asarray([i for x in lists for i in x], dtype=np.int64)
    return off, ids, dict(single=single, exact=exact, over=over, long=long_, triple=triple)


@pytest.mark.parametrize("reduce,dtype", [("mean", "fp16"), ("sum", "fp32")])
def test_csr_lists_on_a_middle_third(reduce, dtype):
    C, n_rows, d = _chunk(), 90, 200
    own = (30, 60)
    off, ids, names = _csr_lists(C, n_rows, own, np.random.default_rng(3))
    ntok = len(off) - 1
    rid, lens = BW.row_lengths(off, ids, *own)
    length = dict(zip(rid.tolist(), lens.tolist()))
    assert off[1] == 0 and off[-1] == off[-2], "the lists at both ends are not empty"
    assert length[names["single"]] == 1 and length[names["exact"]] == C
    assert length[names["over"]] == C + 1 and length[names["long"]] == 3 * C + 5 and length[names["triple"]] == 4
    assert len(rid) < own[1] - own[0] and BW.positions_with_a_duplicate(off, ids) > 0
    assert ((ids < own[0]) | (ids >= own[1])).any(), "no id of another shard"
    g = _grad(ntok, d, dtype)
    want = BW.backward_rows(off, ids, _g32(g), reduce, C, *own, n_rows)
    rev = BW.backward_rows(off, ids, _g32(g), reduce, C, *own, n_rows, reverse=True)[1]
    flat = BW.backward_rows(off, ids, _g32(g), reduce, C, *own, n_rows, chunked=False)[1]
    assert (rev.view(np.uint32) != want[1].view(np.uint32)).any() and (flat.view(np.uint32) != want[1].view(np.uint32)).any()
    table = _table(3, d, own=own, n_rows=n_rows, with_index=False)
    with table.backward_plan_csr(torch.from_numpy(off), torch.from_numpy(ids)) as plan:
        assert plan.n_rows == len(want[0]) and plan.n_refs == int(lens.sum())
        got = _rows(plan, g, reduce, d)
        counts = plan.counts().cpu().numpy()
    _check(got, want, f"csr-{reduce}-{dtype}")
    assert np.array_equal(counts, np.diff(off)), "K_p is the list length"
    assert table.status() == 0


def test_csr_ids_outside_the_table_are_skipped_and_reported():
    from scone_amd import _lib
    C, n_rows, d = _chunk(), 90, 64
    off, ids, _ = _csr_lists(C, n_rows, (0, n_rows), np.random.default_rng(4))
    ids = ids.copy()
    ids[[3, 40, 41, len(ids) - 1]] = [-1, n_rows, 2 ** 31 - 1, -(2 ** 31)]
    g = _grad(len(off) - 1, d, "fp16")
    want = BW.backward_rows(off, ids, _g32(g), "mean", C, 0, n_rows, n_rows)
    table = _table(3, d, n_rows=n_rows, with_index=False)
    with table.backward_plan_csr(torch.from_numpy(off), torch.from_numpy(ids)) as plan:
        got = _rows(plan, g, "mean", d)
        assert np.array_equal(plan.counts().cpu().numpy(), np.diff(off))
    _check(got, want, "csr-bad-ids")
    assert table.status() == _lib.ST_BAD_ID
    assert table.status() == 0


# ------------------------------------------------------------------ 3. ownership
@pytest.mark.parametrize("max_n", [3, 4])
def test_three_handles_own_thirds(max_n):
    d, n = 200, N_ROWS[max_n]
    off, _ = _lists("small", max_n, "cover")
    g = _grad(len(off) - 1, d, "fp16")
    whole = _want("small", max_n, "cover", "mean", d, "fp16")
    parts = []
    for own in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
        want = _want("small", max_n, "cover", "mean", d, "fp16", own)
        table = _table(max_n, d, own=own)
        with _plan(table, "small", max_n) as plan:
            got = _rows(plan, g, "mean", d)
            assert np.array_equal(plan.counts().cpu().numpy(), np.diff(off)), "K_p is the full count on every shard"
        _check(got, want, f"own{own}")
        assert len(got[0]) and got[0].min() >= own[0] and got[0].max() < own[1]
        assert table.status() == 0
        parts.append(got)
    union = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    _check(union, whole, "union of the thirds")


# ------------------------------------------------------------------ 4. plan lifetime
def test_a_plan_outlives_later_lookups_and_bad_token_ids(monkeypatch):
    """Lookups of OTHER tokens through the stream's workspace between the plan and its use; tokens of -1 and == vocab in the
    planned batch.  The vocabularies' f-grams are over the tokens {0, 1, 2}, so a window that holds -1 (matches nothing) or 4
    (>= vocab: matched like any token, and in no f-gram) has the list it has with token 3 (in no f-gram) in that place."""
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")         # read at create: every lookup takes the workspace road
    max_n, d = 4, 768
    tok, cu = _batch("small", max_n)
    tok = tok.copy()
    rng = np.random.default_rng(9)
    bad = rng.choice(len(tok), size=40, replace=False)
    tok[bad[:20]], tok[bad[20:]] = -1, VOCAB + 1
    assert (tok == -1).sum() == 20 and (tok == VOCAB + 1).sum() == 20
    off, ids = _lists_of(np.where((tok < 0) | (tok > VOCAB), VOCAB, tok), cu, max_n, "cover")
    assert not np.array_equal(off, _lists("small", max_n, "cover")[0]), "the bad ids change no list"
    table = _table(max_n, d)
    table.store_f32(torch.randn(N_ROWS[max_n], d))
    plan = table.backward_plan(torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32)))
    assert plan.n_refs == int(off[-1])
    other, other_cu = _batch("r37", max_n), _batch("tiny", max_n)
    table.embed(torch.from_numpy(other[0].reshape(RECTS["r37"])))
    table.embed_varlen(torch.from_numpy(other_cu[0]), torch.from_numpy(other_cu[1].astype(np.int32)))
    for seed, reduce, dtype in ((1, "mean", "fp16"), (2, "sum", "bf16")):
        g = _grad(len(tok), d, dtype, seed)
        want = BW.backward_rows(off, ids, _g32(g), reduce, _chunk(), 0, None, N_ROWS[max_n])
        _check(_rows(plan, g, reduce, d), want, f"lifetime-{reduce}-{dtype}")
    assert np.array_equal(plan.counts().cpu().numpy(), np.diff(off))
    plan.close()
    plan.close()                                                # idempotent
    assert table.status() == 0


# ------------------------------------------------------------------ 5. the module
def _cache(fmt, d, max_n, mode, rows):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = WS._vocabulary(max_n)
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt, lookup_mode=mode)
    cache.cache_embeddings(list(range(rows.shape[0])), rows, verbose=False)
    return cache


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", ["fp32", "int8"])
def test_trainable_module(fmt, mode):
    from scone_amd import TrainableFGramTable
    max_n, d = 3, 768
    B, T = RECTS["r37"]
    tok_np, _ = _batch("r37", max_n)
    tok = torch.from_numpy(tok_np.reshape(B, T))
    off, ids = _lists("r37", max_n, mode)
    K = np.diff(off)
    w0 = torch.from_numpy(np.random.default_rng(21).standard_normal((N_ROWS[max_n], d)).astype(np.float32))
    cache = _cache(fmt, d, max_n, mode, w0)
    module = TrainableFGramTable(cache, w0.clone())
    assert isinstance(module.weight, torch.nn.Parameter) and module.weight.is_cuda
    base = _grad(B * T, d, "fp16", seed=3).reshape(B, T, d).cuda().requires_grad_(True)
    g = _grad(B * T, d, "fp16", seed=4).reshape(B, T, d).cuda()

    def forward_reference(c):
        if mode == "longest_suffix":                             # the paper's lookup onto a dense base is the table's call
            return c.table.embed_base(tok, base.detach())
        return c.embed_tokens(tok, base=base.detach())

    out = module(tok, base=base)
    assert out.dtype == torch.float16 and E.same_bits(WS._bits(out), WS._bits(forward_reference(cache)))
    plain = module(tok)                                          # without a base: the f-gram part alone, fp32
    assert E.same_bits(WS._bits(plain), WS._bits(cache.embed_tokens(tok)))
    out.backward(g)
    grad = module.weight.grad
    assert grad.is_sparse and grad.is_coalesced() and tuple(grad.shape) == (N_ROWS[max_n], d)
    want = BW.backward_rows(off, ids, _g32(g.cpu().reshape(B * T, d)), "mean", _chunk(), 0, None, N_ROWS[max_n])
    got = (grad.indices()[0].cpu().numpy(), grad.values().cpu().numpy())
    _check(got, want, f"module-{fmt}-{mode}")
    with cache.table.backward_plan(tok) as plan:
        pid, prows = plan.rows(g, "mean")
    assert np.array_equal(pid.cpu().numpy(), got[0]) and E.same_bits(prows.cpu().numpy(), got[1])
    keep = np.ones(B * T, dtype=bool) if mode == "cover" else K == 0
    assert (~keep).any() == (mode == "longest_suffix")
    want_base = g.cpu().reshape(B * T, d)
    if mode == "longest_suffix":                                 # the definition: grad_out * (K == 0), a product (-x * 0 is -0)
        want_base = (want_base.float() * torch.from_numpy(keep)[:, None].float()).half()
    assert base.grad.dtype == torch.float16 and E.same_bits(WS._bits(base.grad.reshape(B * T, d)), WS._bits(want_base))
    # a second backward through the same module: the same bits
    module.weight.grad = None
    module(tok, base=base).backward(g)
    again = module.weight.grad
    assert np.array_equal(again.indices()[0].cpu().numpy(), got[0]) and E.same_bits(again.values().cpu().numpy(), got[1])
    # one optimiser step, commit: the served table equals a table built from the updated weights
    torch.optim.SGD([module.weight], lr=0.5).step()
    assert not torch.equal(module.weight.detach().cpu(), w0)
    assert module.commit() == len(got[0]) and module.commit() == 0
    fresh = _cache(fmt, d, max_n, mode, module.weight.detach().cpu())
    assert E.same_bits(WS._bits(module(tok, base=base)), WS._bits(forward_reference(fresh)))
    assert E.same_bits(WS._bits(module(tok)), WS._bits(fresh.embed_tokens(tok)))
    assert not E.same_bits(WS._bits(module(tok)), WS._bits(plain)), "the step did not reach the served table"
    assert cache.table.status() == 0
