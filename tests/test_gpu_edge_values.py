"""Every kernel that computes the mean, at the edges of the fp32 / fp16 / bf16 range (tests/edge_fixture.py: subnormal quotients,
sums that overflow to +-inf, literal inf / NaN, values on the half-precision rounding boundaries, -0.0 / inf / 65504 in wte and
wpe).  Run with ``-m gpu`` on an MI355X.

The bar is the project's own, without a tolerance: the output equals the oracle's (oracle/ref_port.py, itself held to what the
reference computed on the same values by tests/test_oracle_golden.py and tests/golden/edge.npz) BIT FOR BIT -- equal NaN
positions, every other element with equal bits, sign of zero and of infinity included.  Half-precision outputs are torch's
``.half()`` / ``.to(torch.bfloat16)`` of the fp32 expectation (one round-to-nearest-even); wte / wpe are given in the output
dtype and enter the expectation through their fp32 upcasts.  The arithmetic of the division itself is guarded on the CPU
(tests/test_mean_div_cpu.py); what these tests add is that the device executes it the same way: fp32 subnormals kept, nothing
contracted, one rounding to the output type, in every kernel family:

  k_embed_fused                       d = 768 / 1024 / 1280, batches up to 32768 tokens
  k_embed_wave (position row in LDS)  the same dims with SCONE_FUSED_MAX_TOKENS=0, default positions
  k_embed_wave (per-token positions)  the same with explicit position_ids
  k_embed_wave_any                    d = 64 and d = 2048
  k_embed (plain `/`: the control)    fp32 table, d = 100 (a multiple of 4, not of 8)
  k_embed_csr_wave                    SconeTable.gather_reduce and embed_tokens(base=...)
  partial sums + k_finalize_wave      embed_partial on two row shards, add, finalize
  K <= 1 (no mean)                    lookup_mode="longest_suffix": rows go through unchanged, non-finite ones included
"""

import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_fixture as E  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


@pytest.fixture(params=["one_launch", "two_kernels"])
def lookup_form(request, monkeypatch):
    """As in test_gpu_parity.py: SCONE_FUSED_MAX_TOKENS=0 (read when a handle is created) sends every batch through
    k_match_ell + k_embed_wave instead of k_embed_fused."""
    if request.param == "two_kernels":
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    else:
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    return request.param


def _bits(t):
    """torch tensor -> numpy array that edge_fixture.same_bits compares (bf16 as its uint16 bit patterns)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def _to(x32, dtype):
    """One round-to-nearest-even of an fp32 numpy array to the output dtype, by torch."""
    return torch.from_numpy(np.ascontiguousarray(x32)).to(dtype)


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want.reshape(got.shape))
    assert E.same_bits(g, w), (what, E.first_difference(g, w))


def _cache(keys, lens, max_n, table, fmt, **kw):
    from scone_amd import EmbeddingCache, NGramExtractor
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    c = EmbeddingCache(ex, table.shape[1], table_format=fmt, **kw)
    c.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    return c


def _stored(table, fmt):
    """What the table format holds, as fp32 (the oracle runs on this)."""
    if fmt == "fp32":
        return table
    if fmt == "fp16":
        with np.errstate(over="ignore", invalid="ignore"):
            return table.astype(np.float16).astype(np.float32)
    if fmt == "int8":
        return R.dequantize_i8(*R.quantize_i8(table))
    return R.dequantize_i4(*R.quantize_i4(table))


def _oracle(stored, off, ids, reduce, shape):
    with np.errstate(over="ignore", invalid="ignore"):
        return R.embed_numpy(stored, off, ids, reduce).reshape(*shape, stored.shape[1])


def _combine(tok, fg32, wte_t, wpe_t, position_ids=None):
    """(wte + mean) + wpe in fp32 from the fp32 upcasts of the wte / wpe the kernel is given."""
    return R.combine(torch.from_numpy(tok), torch.from_numpy(fg32), wte_t.float().cpu(), wpe_t.float().cpu(),
                     position_ids=position_ids).numpy()


def _check_lookups(cache, stored, keys, lens, max_n, d, seed, what):
    """Every stream of the fixture through embed_tokens: mean and sum, three output dtypes, alone / with wte + wpe at default and
    at explicit positions."""
    wte, wpe = E.wte_wpe(3, 64, d, seed=seed)
    rng = np.random.default_rng(5 + seed)
    for si, tok in enumerate(E.streams(max_n)):
        B, T = tok.shape
        off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
        pos = torch.from_numpy(rng.integers(0, 64, size=(B, T)))
        for reduce in ("mean", "sum"):
            fg = _oracle(stored, off, ids, reduce, (B, T))
            for dt in DTYPES:
                tag = (what, f"stream {si} {B}x{T}", reduce, str(dt))
                out = cache.embed_tokens(torch.from_numpy(tok), reduce=reduce, out_dtype=dt)
                assert out.dtype == dt and out.shape == (B, T, d)
                _assert_same(out, _to(fg, dt), tag + ("rows only",))
                wte_t, wpe_t = _to(wte, dt).cuda(), _to(wpe, dt).cuda()
                for position_ids in (None, pos):
                    out = cache.embed_tokens(torch.from_numpy(tok), reduce=reduce, wte=wte_t, wpe=wpe_t,
                                             position_ids=position_ids, check=True)
                    assert out.dtype == dt
                    ref = _combine(tok, fg, wte_t, wpe_t, position_ids)
                    _assert_same(out, _to(ref, dt), tag + ("wte+wpe", "default positions" if position_ids is None else "position_ids"))


# ------------------------------------------------------------------ the fixture itself, on the GPU
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_fixture_on_the_gpu_equals_the_reference(golden_dir, max_n):
    """d = 64 (k_embed_wave_any), fp32 table: directly against what the reference returned (tests/golden/edge.npz)."""
    z = np.load(os.path.join(golden_dir, "edge.npz"), allow_pickle=False)
    c = f"n{max_n}"
    keys, lens, table = z[f"{c}_keys"], z[f"{c}_lens"], z[f"{c}_table"]
    cache = _cache(keys, lens, max_n, table, "fp32")
    assert E.same_bits(cache.table.gather_rows(torch.arange(len(lens))).cpu().numpy(), table)
    wte, wpe = torch.from_numpy(z[f"{c}_wte"]).cuda(), torch.from_numpy(z[f"{c}_wpe"]).cuda()
    for si in range(int(z[f"{c}_n_streams"])):
        tok = torch.from_numpy(z[f"{c}_s{si}_tok"])
        off, ids = cache.match(tok)
        assert np.array_equal(off.cpu().numpy(), z[f"{c}_s{si}_off"]) and np.array_equal(ids.cpu().numpy(), z[f"{c}_s{si}_ids"])
        _assert_same(cache.embed_tokens(tok, out_dtype=torch.float32), torch.from_numpy(z[f"{c}_s{si}_mean_f32"]), (c, si, "mean"))
        _assert_same(cache.embed_tokens(tok, out_dtype=torch.float16), torch.from_numpy(z[f"{c}_s{si}_mean_f16"]), (c, si, "half"))
        _assert_same(cache.embed_tokens(tok, wte=wte, wpe=wpe, check=True), torch.from_numpy(z[f"{c}_s{si}_embeds"]), (c, si, "embeds"))
        if f"{c}_s{si}_pos" in z.files:
            out = cache.embed_tokens(tok, wte=wte, wpe=wpe, position_ids=torch.from_numpy(z[f"{c}_s{si}_pos"]), check=True)
            _assert_same(out, torch.from_numpy(z[f"{c}_s{si}_embeds_pos"]), (c, si, "embeds at position_ids"))


# ------------------------------------------------------------------ the hit-list kernels
@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_values_specialised_dims(fmt, d, max_n, lookup_form):
    """k_embed_fused (one launch) and k_embed_wave (two kernels; position row in LDS at default positions, per-token rows with
    position_ids).  Every 64 columns hold every value class, so every lane segment -- the trailing 256-element one of 768 and
    1280 included -- divides subnormals, infinities and NaNs."""
    keys, lens = E.vocabulary(max_n)
    table = E.table(len(lens), d, seed=max_n)
    cache = _cache(keys, lens, max_n, table, fmt)
    stored = _stored(table, fmt)
    assert E.same_bits(cache.table.gather_rows(torch.arange(len(lens))).cpu().numpy(), stored), "device table differs"
    _check_lookups(cache, stored, keys, lens, max_n, d, max_n, (fmt, d, max_n, lookup_form))


@pytest.mark.parametrize("fmt,d", [("fp32", 64), ("fp16", 64), ("fp32", 2048), ("fp16", 2048), ("fp32", 100)])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_values_other_dims(fmt, d, max_n):
    """k_embed_wave_any (d = 64, 2048) and, as the control that has always divided with `/`, k_embed (fp32, d = 100)."""
    keys, lens = E.vocabulary(max_n)
    table = E.table(len(lens), d, seed=max_n)
    cache = _cache(keys, lens, max_n, table, fmt)
    stored = _stored(table, fmt)
    assert E.same_bits(cache.table.gather_rows(torch.arange(len(lens))).cpu().numpy(), stored), "device table differs"
    _check_lookups(cache, stored, keys, lens, max_n, d, max_n, (fmt, d, max_n))


# ------------------------------------------------------------------ caller-supplied lists
@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [768, 1024, 1280])
def test_edge_values_csr_lists(fmt, d):
    """k_embed_csr_wave: SconeTable.gather_reduce with lists of K = 0, 1, 2, 3, 6, 10, 37 ids (repeated ids among them) and
    embed_tokens(base=...), mean and sum, three output dtypes, with and without base rows."""
    max_n = 3
    keys, lens = E.vocabulary(max_n)
    n = len(lens)
    table = E.table(n, d, seed=9)
    cache = _cache(keys, lens, max_n, table, fmt)
    stored = _stored(table, fmt)
    rng = np.random.default_rng(3)
    ks = [0, 1, 2, 3, 6, 10, 37, 6, 10, 37, 5, 7, 9, 4, 8] + [6] * 40 + [10] * 40 + rng.integers(0, 13, size=60).tolist()
    off = np.zeros(len(ks) + 1, dtype=np.int64)
    np.cumsum(ks, out=off[1:])
    ids = rng.integers(0, n, size=int(off[-1])).astype(np.int64)
    ids[off[7]:off[8]] = ids[off[7]]                                     # one id six times
    ids[off[9]:off[9] + 20] = ids[off[9]]
    base, _ = E.wte_wpe(len(ks), 1, d, seed=4)
    for reduce in ("mean", "sum"):
        fg = _oracle(stored, off, ids, reduce, (len(ks),))
        for dt in DTYPES:
            got = cache.table.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, out_dtype=dt)
            _assert_same(got, _to(fg, dt), (fmt, d, reduce, str(dt), "lists"))
            b = _to(base, dt)
            got = cache.table.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, base=b, out_dtype=dt)
            _assert_same(got, _to(b.float().numpy() + fg, dt), (fmt, d, reduce, str(dt), "lists + base"))
    assert cache.table.status() == 0
    for si, tok in enumerate(E.streams(max_n)):
        B, T = tok.shape
        o, i = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
        bb, _ = E.wte_wpe(B * T, 1, d, seed=20 + si)
        for reduce in ("mean", "sum"):
            fg = _oracle(stored, o, i, reduce, (B, T))
            for dt in DTYPES:
                b = _to(bb.reshape(B, T, d), dt)
                got = cache.embed_tokens(torch.from_numpy(tok), base=b.cuda(), reduce=reduce)
                assert got.dtype == dt
                _assert_same(got, _to(b.float().numpy() + fg, dt), (fmt, d, reduce, str(dt), "embed_tokens(base)", si))


# ------------------------------------------------------------------ row shards
@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_values_partial_sums_and_finalize(fmt, d, max_n):
    """embed_partial on two row shards, the add of the reduce-scatter, k_finalize_wave.  The expectation adds the two shards'
    sequential sums (each in list order over the rows the shard owns) and divides once: (s0 + s1) / K."""
    from scone_amd.hip_backend import SconeTable
    keys, lens = E.vocabulary(max_n)
    n = len(lens)
    table = E.table(n, d, seed=30 + max_n)
    stored = _stored(table, fmt)
    wte, wpe = E.wte_wpe(3, 64, d, seed=max_n)
    cut = n // 3
    shards = []
    for a, b in ((0, cut), (cut, n)):
        s = SconeTable(max_n, n, d, fmt, row_begin=a, row_end=b)
        s.index_build(keys, lens)
        s.store_f32(torch.from_numpy(table[a:b]), row0=a)
        shards.append(s)
    for si, tok in enumerate(E.streams(max_n)):
        B, T = tok.shape
        ntok = B * T
        off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
        seg = np.repeat(np.arange(ntok), np.diff(off))
        want_parts = []
        for a, b in ((0, cut), (cut, n)):
            own = (ids >= a) & (ids < b)
            o = np.zeros(ntok + 1, dtype=np.int64)
            np.cumsum(np.bincount(seg[own], minlength=ntok), out=o[1:])
            want_parts.append(_oracle(stored, o, ids[own], "sum", (ntok,)))
        parts = [s.embed_partial(torch.from_numpy(tok)) for s in shards]
        for p, w in zip(parts, want_parts):
            _assert_same(p[0], torch.from_numpy(w), (fmt, d, max_n, si, "partial sums"))
            assert np.array_equal(p[1].cpu().numpy(), np.diff(off))
        total = parts[0][0] + parts[1][0]
        with np.errstate(over="ignore", invalid="ignore"):
            sums = want_parts[0] + want_parts[1]
            K = np.diff(off).astype(np.float32)[:, None]
            mean = np.where(K > 1, sums / np.maximum(K, np.float32(1)), sums).astype(np.float32)
        _assert_same(total, torch.from_numpy(sums), (fmt, d, max_n, si, "added sums"))
        for reduce, fg in (("mean", mean), ("sum", sums)):
            for dt in DTYPES:
                wte_t, wpe_t = _to(wte, dt).cuda(), _to(wpe, dt).cuda()
                cuts = ((0, ntok // 2), (ntok // 2, ntok))
                halves = [shards[r].finalize(total[a:b], parts[0][1][a:b], torch.from_numpy(tok), a, b, wte=wte_t, wpe=wpe_t,
                                             reduce=reduce, out_dtype=dt) for r, (a, b) in enumerate(cuts) if b > a]
                out = torch.cat(halves).reshape(B, T, d)
                ref = _combine(tok, fg.reshape(B, T, d), wte_t, wpe_t)
                _assert_same(out, _to(ref, dt), (fmt, d, max_n, si, reduce, str(dt), "finalize"))


# ------------------------------------------------------------------ K <= 1: no mean
@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [64, 768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_values_longest_suffix_rows_pass_through(fmt, d, max_n, lookup_form):
    """lookup_mode='longest_suffix': one row or the token embedding, never a division -- subnormals, infinities and NaNs go
    through unchanged (then + wpe, one rounding)."""
    keys, lens = E.vocabulary(max_n)
    table = E.table(len(lens), d, seed=40 + max_n)
    cache = _cache(keys, lens, max_n, table, fmt, lookup_mode="longest_suffix")
    stored = _stored(table, fmt)
    f2id = R._key_dict(keys, lens)
    wte, wpe = E.wte_wpe(3, 64, d, seed=max_n)
    for si, tok in enumerate(E.streams(max_n)):
        for dt in DTYPES:
            with np.errstate(over="ignore", invalid="ignore"):
                only = R.paper_embed(f2id, max_n, tok, stored)
            _assert_same(cache.embed_tokens(torch.from_numpy(tok), out_dtype=dt), _to(only, dt), (fmt, d, max_n, si, str(dt), "rows"))
            wte_t, wpe_t = _to(wte, dt), _to(wpe, dt)
            with np.errstate(over="ignore", invalid="ignore"):
                ref = R.paper_embed(f2id, max_n, tok, stored, wte=wte_t.float().numpy(), wpe=wpe_t.float().numpy())
            got = cache.embed_tokens(torch.from_numpy(tok), wte=wte_t.cuda(), wpe=wpe_t.cuda(), check=True)
            _assert_same(got, _to(ref, dt), (fmt, d, max_n, si, str(dt), "wte+wpe"))


# ------------------------------------------------------------------ INT8 / INT4: the edges are the scales
def _quantised_edge_table(n, d, group, qmax, seed):
    """Finite rows whose groups of `group` columns (the whole row for INT8) are, in turn: an fp16-SUBNORMAL scale (absmax =
    qmax * m * 2^-24, m = 1, 3, 511, 1023), the largest finite scale (absmax = qmax * 65504), an all-zero group, values exactly
    on the k + 0.5 quantisation ties (absmax = qmax: scale 1.0), and ordinary normals."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, d), dtype=np.float32)
    kinds = 0
    for r in range(n):
        for g in range(d // group):
            kind = (r + 7 * g) % 8                       # group g + 1 holds kind - 1: the all-zero group sits beside the largest scale
            kinds |= 1 << kind
            q = rng.integers(-qmax, qmax + 1, size=group).astype(np.float32)
            q[rng.integers(0, group)] = qmax if rng.random() < 0.5 else -qmax
            if kind < 4:
                v = q * np.float32((1, 3, 511, 1023)[kind] * 2.0 ** -24)
            elif kind == 4:
                v = q * np.float32(65504.0)
            elif kind == 5:
                v = np.zeros(group, dtype=np.float32)
            elif kind == 6:
                v = np.where(np.abs(q) == qmax, q, q + np.float32(0.5) * rng.choice([-1.0, 1.0], size=group)).astype(np.float32)
                v = np.clip(v, -qmax, qmax).astype(np.float32)
            else:
                v = rng.standard_normal(group).astype(np.float32)
            t[r, g * group:(g + 1) * group] = v
    assert kinds == 0xFF
    return t


@pytest.mark.parametrize("fmt,d", [("int8", 768), ("int8", 1024), ("int8", 1280), ("int8", 64), ("int4", 1024), ("int4", 256)])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_scales_of_the_quantised_formats(fmt, d, max_n, lookup_form):
    """Finite tables only (what the quantiser does with inf / NaN is unspecified).  First the device table equals
    R.quantize_* / R.dequantize_*, then every lookup bit for bit in fp32, fp16 and bf16."""
    keys, lens = E.vocabulary(max_n)
    n = len(lens)
    table = _quantised_edge_table(n, d, d if fmt == "int8" else R.I4_GROUP, 127 if fmt == "int8" else 7, seed=max_n + d)
    cache = _cache(keys, lens, max_n, table, fmt)
    stored = _stored(table, fmt)
    scale = (R.quantize_i8 if fmt == "int8" else R.quantize_i4)(table)[1].astype(np.float32)
    assert ((scale > 0) & (scale < 2.0 ** -14)).any() and (scale == 65504).any() and (scale == 0).any() and (scale == 1).any()
    assert np.array_equal(cache.table.gather_rows(torch.arange(n)).cpu().numpy(), stored), "device quantiser differs from oracle/ref_port.py"
    _check_lookups(cache, stored, keys, lens, max_n, d, max_n, (fmt, d, max_n, lookup_form))
