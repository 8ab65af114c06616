"""The multi-sequence walk of the large-batch lookup kernels, at every instantiation, against the oracle.

Once a batch has more (sequence, position-group) pairs than the launch target, `k_embed_wave` and `k_embed_wave_any`
(scone_amd/csrc/scone_embed_wave.h) give one workgroup SEVERAL sequences to walk.  Below that the loop body runs once, and
that is where every small-batch suite lives; tests/test_gpu_bench_shape.py reaches the walk, but only at T = 512, max_n = 3,
default positions and d = 768 / 1024 / 1280.  The cases here put every other instantiation of the walk in front of
oracle/ref_port.py, on a few ten thousand tokens each:

* explicit per-token `position_ids` that DIFFER between the sequences a workgroup walks (the carried `posv = posn`),
* the second and later iterations of `k_embed_wave_any`'s `for (b = b0; b < b1; ++b)`, in its full and its partial-sum form,
* T = 1, T < 4 and T % 4 != 0 (waves with i >= T leave, `pos_groups` rounds up), a last run shorter than the others,
* max_n = 4 (16-word records) and max_n = 1 / 2 on the max_n = 3 template, `reduce="sum"`, bf16 output,
  `lookup_mode="longest_suffix"`, a CU reserve (smaller grid, longer runs), a row shard that owns part of the ids
  (`embed_partial`, then `finalize`),
* the lane-group fallback `k_embed` (d = 100) at ~60k tokens (no walk; its flattened indices far beyond the small suites').

Every case asserts its own preconditions before it looks at the GPU's answer: tests/walk_geometry.py (a pure-Python mirror
of the two launch geometries) says that a workgroup walks >= 3 sequences and that the last run is shorter than the others,
for every register-dependent grid size k_embed_wave can pick; SCONE_FUSED_MAX_TOKENS=0 is set before the handle exists, so
the two-kernel form is taken whatever the batch size; and every id-list length the kernel's `switch (kown)` can meet at that
(T, max_n) occurs in the batch.  Every lookup writes into a caller's buffer pre-filled with NaN (counts: with -7), so a
token the walk never visits cannot hold a previous call's correct value.

The bar has no tolerance: fp32 output equals the oracle's bit for bit; fp16 / bf16 output equals the oracle's fp32 result
rounded once (the claim tests/test_gpu_bench_shape.py and tests/test_gpu_edge_values.py make).  Tables are quantised on the
host by oracle/ref_port.py (`quantize_*` / `dequantize_*`), so the expectation never passes through HIP code.

`tools/mutation_check.sh` breaks the walk in ways the older suites cannot see (`stale_position`: the carried position id is
never refreshed; `any_no_advance`: k_embed_wave_any stays on its first sequence; `stale_count`: the partial-sum form writes
the first token's hit count for every token of the run) and shows that this file fails on each while
test_gpu_bench_shape.py / test_gpu_parity.py's many-sequence tests still pass; its output is in profiles/r07b/.
"""

import collections
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_fixture as E  # noqa: E402
import walk_geometry as G  # noqa: E402

pytestmark = pytest.mark.gpu

VOCAB = 3                    # the f-grams are over the tokens {0, 1, 2}; token 3 is in wte but in no f-gram (K = 0)
TOKEN_P = (0.31, 0.31, 0.31, 0.07)
N_ROWS = {1: 40, 2: 40, 3: 60, 4: 200}          # rows of the table (ids) per max_n: every K in 0..max_n(max_n+1)/2 occurs
N_POS = 64                   # rows of wpe: more than any T here
# B per T: under BOTH geometries a workgroup walks >= 3 sequences and the last run is shorter than the others -- for
# k_embed_wave at every WAVES in 1..8 on 256 and on 240 compute units (asserted again by every case on the box's own count)
SHAPES = {1: (12301, 1), 3: (12301, 3), 5: (6203, 5), 16: (3083, 16), 37: (1243, 37)}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SENTINEL = -7

Case = collections.namedtuple("Case", "family fmt d max_n T mode reduce positions dtype wte reserve")


def _name(c):
    B, T = SHAPES[c.T]
    return (f"{c.family}-{c.fmt}-d{c.d}-n{c.max_n}-{B}x{T}-{c.mode}-{c.reduce}-pos_{c.positions}-{c.dtype}-"
            f"{'wte' if c.wte else 'nowte'}" + (f"-reserve{c.reserve}" if c.reserve else ""))


def _case(family, fmt, d, max_n, T, positions, dtype, mode="cover", reduce="mean", wte=True, reserve=0):
    c = Case(family, fmt, d, max_n, T, mode, reduce, positions, dtype, wte, reserve)
    return pytest.param(c, id=_name(c))


def _wave_cases():
    out = []
    # explicit per-token positions (and the default ones) at every T, max_n = 3 / 4, three output dtypes, with / without wte
    setups = [("int8", 768, 3, 1), ("fp16", 1024, 4, 1), ("fp32", 1280, 3, 3), ("int4", 1024, 4, 3), ("fp16", 768, 3, 5),
              ("int8", 1280, 4, 5), ("int4", 1024, 3, 16), ("fp32", 768, 4, 16), ("int8", 1024, 3, 37), ("fp16", 1280, 4, 37)]
    rot = ["fp32", "fp16", "bf16"]
    for k, (fmt, d, max_n, T) in enumerate(setups):
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "random", rot[k % 3]))
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "random", rot[(k + 1) % 3], wte=False))
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "default", rot[(k + 2) % 3]))
    # max_n = 1 and 2 run on the max_n = 3 template
    for fmt, d, max_n, T in (("int8", 768, 1, 5), ("fp16", 1024, 2, 16)):
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "random", "fp32"))
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "default", "fp16"))
    # reduce = "sum"
    for fmt, d, max_n, T in (("fp16", 768, 3, 5), ("fp16", 1280, 4, 37)):
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "random", "fp32", reduce="sum"))
        out.append(_case("k_embed_wave", fmt, d, max_n, T, "default", "bf16", reduce="sum"))
    # the paper's lookup
    for fmt, d, T in (("fp32", 768, 3), ("int8", 1024, 5), ("int4", 1024, 37)):
        out.append(_case("k_embed_wave", fmt, d, 4, T, "default", "fp32", mode="longest_suffix"))
        out.append(_case("k_embed_wave", fmt, d, 4, T, "random", "fp16", mode="longest_suffix"))
    # a CU reserve: smaller target, longer runs
    out.append(_case("k_embed_wave", "int8", 768, 3, 16, "random", "fp16", reserve=16))
    out.append(_case("k_embed_wave", "int8", 768, 3, 16, "default", "fp32", reserve=16))
    return out


def _any_cases():
    out = []
    setups = [("int8", 2048, 3, 5), ("int8", 2048, 4, 16), ("fp16", 4096, 4, 1), ("fp16", 4096, 3, 5), ("fp32", 136, 3, 37),
              ("fp32", 136, 4, 3), ("int8", 48, 4, 16), ("int8", 48, 3, 1), ("int4", 1280, 3, 16), ("int4", 1280, 4, 5),
              ("int4", 2048, 4, 37), ("int4", 2048, 3, 3), ("fp16", 64, 3, 3), ("fp16", 64, 4, 37)]
    for k, (fmt, d, max_n, T) in enumerate(setups):
        out.append(_case("k_embed_wave_any", fmt, d, max_n, T, "default", "fp32"))
        out.append(_case("k_embed_wave_any", fmt, d, max_n, T, "random", ("fp16", "bf16")[k % 2]))
        if k % 3 == 0:
            out.append(_case("k_embed_wave_any", fmt, d, max_n, T, "random", "fp32", wte=False, reduce="sum"))
    for fmt, d, max_n, T in (("int8", 2048, 4, 5), ("fp32", 136, 3, 37), ("int4", 1280, 4, 3)):
        out.append(_case("k_embed_wave_any", fmt, d, max_n, T, "default", "fp32", mode="longest_suffix"))
        out.append(_case("k_embed_wave_any", fmt, d, max_n, T, "random", "bf16", mode="longest_suffix"))
    return out


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


@pytest.fixture(autouse=True)
def two_kernels(monkeypatch):
    """SCONE_FUSED_MAX_TOKENS=0 is read when a handle is created: every handle of this file sends every batch through
    k_match_ell + the large-batch kernel, never through the one-launch kernel."""
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")


# ------------------------------------------------------------------ inputs and expectations (host only)
@functools.lru_cache(maxsize=None)
def _vocabulary(max_n):
    rng = np.random.default_rng(100 + max_n)
    n = N_ROWS[max_n]
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, VOCAB, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    return keys, lens


def _stored(table, fmt):
    """What the table format holds, as fp32 (the oracle runs on this)."""
    if fmt == "fp32":
        return table
    if fmt == "fp16":
        return table.astype(np.float16).astype(np.float32)
    if fmt == "int8":
        return R.dequantize_i8(*R.quantize_i8(table))
    return R.dequantize_i4(*R.quantize_i4(table))


@functools.lru_cache(maxsize=None)
def _tables(fmt, d, max_n):
    """(fp32 rows given to the handle, the same rows as the format stores them, wte[VOCAB + 1, d], wpe[N_POS, d])."""
    rng = np.random.default_rng(7 * d + max_n)
    table = rng.standard_normal((N_ROWS[max_n], d)).astype(np.float32)
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return table, _stored(table, fmt), wte, wpe


@functools.lru_cache(maxsize=None)
def _batch(max_n, T):
    """Tokens [B, T], random positions [B, T], the batch's hits and CSR id lists."""
    B, T = SHAPES[T]
    rng = np.random.default_rng(1000 * T + max_n)
    tok = rng.choice(VOCAB + 1, size=(B, T), p=TOKEN_P).astype(np.int64)
    pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
    keys, lens = _vocabulary(max_n)
    hits = R.match_hits(keys, lens, tok, max_n)
    off, ids = R.hits_to_csr(hits)
    return tok, pos, hits, off, ids


@functools.lru_cache(maxsize=2)        # consecutive cases share a setup; an entry is up to a few hundred MB
def _fgram_oracle(fmt, d, max_n, T, mode, reduce):
    """The f-gram part of the expectation, fp32 [B, T, d].  cover: the reduced rows.  longest_suffix (R.paper_embed without
    wte / wpe): the row of the longest f-gram ending at the token, zeros where none does -- and that mask [B, T]."""
    stored = _tables(fmt, d, max_n)[1]
    tok, _, _, off, ids = _batch(max_n, T)
    B, T = tok.shape
    if mode == "cover":
        return R.embed_numpy(stored, off, ids, reduce).reshape(B, T, d)
    f2id = R._key_dict(*_vocabulary(max_n))
    matched = np.asarray([R.paper_lookup(f2id, max_n, row.tolist()) for row in tok]) >= 0
    return R.paper_embed(f2id, max_n, tok, stored), matched


def _to(x32, dtype):
    """One round-to-nearest-even of an fp32 numpy array to the output dtype, by torch."""
    return torch.from_numpy(np.ascontiguousarray(x32)).to(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def _expected(c, wte_t, wpe_t):
    """fp32 [B, T, d]: (wte + f-gram) + wpe from the fp32 upcasts of the wte / wpe the kernel is given."""
    tok, pos, _, _, _ = _batch(c.max_n, c.T)
    fg = _fgram_oracle(c.fmt, c.d, c.max_n, c.T, c.mode, c.reduce)
    wpe32 = wpe_t.float().cpu().numpy()
    pid = pos if c.positions == "random" else np.broadcast_to(np.arange(tok.shape[1]), tok.shape)
    if c.mode == "cover":
        wte32 = wte_t.float().cpu() if c.wte else torch.zeros((VOCAB + 1, c.d))
        return R.combine(torch.from_numpy(tok), torch.from_numpy(fg), wte32, torch.from_numpy(wpe32),
                         position_ids=torch.from_numpy(np.ascontiguousarray(pid))).numpy()
    # Algorithm 2: e = F(f-gram) where one ends at the token, T(token) elsewhere; the model then adds the position row
    e, matched = fg
    if c.wte:
        e = np.where(matched[:, :, None], e, wte_t.float().cpu().numpy()[tok])
    return e + wpe32[pid]


def _suffix_lengths(max_n, T):
    """[B, T]: length of the longest f-gram (>= 2) that ENDS at the token, 0 where none does."""
    tok, _, hits, _, _ = _batch(max_n, T)
    B, T = tok.shape
    best = np.zeros((B, T), dtype=np.int64)
    for n in range(2, min(max_n, T) + 1):
        ends = hits[n - 1, :, :T - n + 1] >= 0              # window starting at s ends at s + n - 1
        best[:, n - 1:] = np.where(ends, n, best[:, n - 1:])
    return best


def _differing(got, want, B, T):
    view = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = (got.view(view).reshape(B, T, -1) != want.view(view).reshape(B, T, -1)).any(axis=2)
    where = np.argwhere(bad)
    return f"{len(where)} of {B * T} tokens differ; first (b, i): {[tuple(int(x) for x in w) for w in where[:6]]}"


# ------------------------------------------------------------------ preconditions
def _assert_regime(family, fmt, d, B, T, reserve=0):
    """The batch makes a workgroup of `family` walk >= 3 sequences, with a shorter last run, in the two-kernel form."""
    assert G.kernel_family(fmt, d) == family
    assert os.environ.get("SCONE_FUSED_MAX_TOKENS") == "0" and not G.takes_one_launch(fmt, d, B * T, fused_max_tokens=0)
    if family == "k_embed":
        return None
    if family == "k_embed_wave_any":
        geoms = [G.wave_any(B, T)]
    else:
        cus = torch.cuda.get_device_properties(0).multi_processor_count - reserve
        geoms = G.wave_all(B, T, cus)
        assert geoms[-1] == G.wave(B, T, cus)                # WAVES = 8: the bound every instantiation stays above
    for g in geoms:
        assert g.seqs_per_block >= 3, (family, B, T, g)
        assert 0 < g.last_run < g.seqs_per_block, (family, B, T, g)
        assert g.pos_groups == (T + 3) // 4 and (g.chunks - 1) * g.seqs_per_block + g.last_run == B
    return geoms


def _assert_lists(c):
    """Every id-list length the kernel can meet at this (T, max_n, mode) occurs in the batch."""
    tok, pos, _, off, _ = _batch(c.max_n, c.T)
    if c.mode == "cover":
        kmax = G.max_list_length(c.T, c.max_n)
        if c.T >= 2 * c.max_n - 1:
            assert kmax == c.max_n * (c.max_n + 1) // 2                   # the full cover: every case of the kernel's switch
        hist = np.bincount(np.diff(off), minlength=kmax + 1)
        assert len(hist) == kmax + 1 and (hist > 0).all(), f"list lengths 0..{kmax}: {hist.tolist()}"
    else:
        lengths = _suffix_lengths(c.max_n, c.T)
        assert set(np.unique(lengths).tolist()) == {0} | set(range(2, min(c.max_n, c.T) + 1))
        assert np.array_equal(lengths > 0, _fgram_oracle(c.fmt, c.d, c.max_n, c.T, c.mode, c.reduce)[1])
    if c.positions == "random":
        assert tok.shape[0] >= 2 and (pos[1:] != pos[:-1]).mean() > 0.9       # rows differ between sequences at the same i


def _handle(fmt, d, max_n, mode="cover", reserve=0):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = _vocabulary(max_n)
    table = _tables(fmt, d, max_n)[0]
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    cache = EmbeddingCache(ex, d, table_format=fmt, lookup_mode=mode)
    cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    if reserve:
        cache.table.set_cu_reserve(reserve)
        assert cache.table.cu_reserve()[0] == reserve
    return cache


# ------------------------------------------------------------------ the full lookup
def _run_lookup(c):
    B, T = SHAPES[c.T]
    _assert_regime(c.family, c.fmt, c.d, B, T, c.reserve)
    _assert_lists(c)
    tok, pos, _, _, _ = _batch(c.max_n, c.T)
    _, _, wte, wpe = _tables(c.fmt, c.d, c.max_n)
    dt = DTYPES[c.dtype]
    wte_t, wpe_t = _to(wte, dt).cuda(), _to(wpe, dt).cuda()
    cache = _handle(c.fmt, c.d, c.max_n, c.mode, c.reserve)
    out = torch.full((B, T, c.d), float("nan"), dtype=dt, device="cuda")
    got = cache.embed_tokens(torch.from_numpy(tok), reduce=c.reduce, wte=wte_t if c.wte else None, wpe=wpe_t,
                             position_ids=torch.from_numpy(pos) if c.positions == "random" else None, out_dtype=dt, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = _expected(c, wte_t, wpe_t)
    assert want.shape == (B, T, c.d) and want.dtype == np.float32 and np.isfinite(want).all()
    g, w = _bits(out), _bits(_to(want, dt))
    assert E.same_bits(g, w), f"{_name(c)}: {_differing(g, w, B, T)}"
    assert cache.table.status() == 0


@pytest.mark.parametrize("c", _wave_cases())
def test_wave_kernel_walks_several_sequences(c):
    """k_embed_wave (d = 768 / 1024 / 1280): explicit positions that differ between the walked sequences, the high-occupancy
    variant with default positions, every T class, max_n 1..4, mean / sum, three output dtypes, with and without wte, the
    paper's lookup, a CU reserve."""
    _run_lookup(c)


@pytest.mark.parametrize("c", _any_cases())
def test_any_dim_kernel_walks_several_sequences(c):
    """k_embed_wave_any (every other d % 8 == 0, and INT4 at 768 / 1280): the second and later iterations of its sequence loop."""
    _run_lookup(c)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_lane_group_fallback_at_sixty_thousand_tokens(dtype):
    """k_embed (d = 100: a multiple of 4, not of 8), fp32 table, explicit positions.  It has no walk; what grows with the batch is
    its flattened indices `group * d`, which the small suites never take beyond a few thousand tokens."""
    d, max_n = 100, 3
    B, T = 1621, 37
    assert B * T > 59_000
    _assert_regime("k_embed", "fp32", d, B, T)
    keys, lens = _vocabulary(max_n)
    rng = np.random.default_rng(4242)
    table = rng.standard_normal((N_ROWS[max_n], d)).astype(np.float32)
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    tok = rng.choice(VOCAB + 1, size=(B, T), p=TOKEN_P).astype(np.int64)
    pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
    hist = np.bincount(np.diff(off), minlength=7)
    assert len(hist) == 7 and (hist > 0).all(), hist.tolist()
    from scone_amd import EmbeddingCache, NGramExtractor
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format="fp32")
    cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    dt = DTYPES[dtype]
    wte_t, wpe_t = _to(wte, dt).cuda(), _to(wpe, dt).cuda()
    fg = R.embed_numpy(table, off, ids, "mean").reshape(B, T, d)
    want = R.combine(torch.from_numpy(tok), torch.from_numpy(fg), wte_t.float().cpu(), wpe_t.float().cpu(),
                     position_ids=torch.from_numpy(pos)).numpy()
    out = torch.full((B, T, d), float("nan"), dtype=dt, device="cuda")
    cache.embed_tokens(torch.from_numpy(tok), wte=wte_t, wpe=wpe_t, position_ids=torch.from_numpy(pos), out_dtype=dt, out=out)
    assert np.isfinite(want).all()
    g, w = _bits(out), _bits(_to(want, dt))
    assert E.same_bits(g, w), f"k_embed-fp32-d{d}-n{max_n}-{B}x{T}-cover-mean-pos_random-{dtype}: {_differing(g, w, B, T)}"
    assert cache.table.status() == 0


# ------------------------------------------------------------------ row shards: partial sums, then finalize
def _own_sums(stored, off, ids, lo, hi):
    """The oracle's list-order fp32 sums over the ids in [lo, hi) only (the other ids of a list are another shard's)."""
    ntok = len(off) - 1
    own = (ids >= lo) & (ids < hi)
    seg = np.repeat(np.arange(ntok), np.diff(off))
    kown = np.bincount(seg[own], minlength=ntok)
    off_own = np.zeros(ntok + 1, dtype=np.int64)
    np.cumsum(kown, out=off_own[1:])
    return R.embed_numpy(stored, off_own, ids[own], "sum"), kown


def _shard_case(family, fmt, d, max_n, T, ranges, dtype):
    B, T_ = SHAPES[T]
    rows = "+".join(f"rows{lo}_{hi}" for lo, hi in ranges)
    return pytest.param(family, fmt, d, max_n, T, ranges, dtype, id=f"{family}-{fmt}-d{d}-n{max_n}-{B}x{T_}-{rows}-pos_random-{dtype}")


@pytest.mark.parametrize("family,fmt,d,max_n,T,ranges,dtype", [
    _shard_case("k_embed_wave", "int8", 768, 3, 5, ((15, 40),), "fp16"),                   # one shard strictly inside the table
    _shard_case("k_embed_wave", "fp32", 1024, 4, 37, ((50, 140),), "fp32"),
    _shard_case("k_embed_wave", "int4", 1024, 4, 3, ((50, 140),), "bf16"),
    _shard_case("k_embed_wave_any", "int8", 2048, 3, 5, ((0, 20), (20, 60)), "fp32"),      # a two-shard split: the sums are added
    _shard_case("k_embed_wave_any", "fp16", 64, 4, 16, ((0, 70), (70, 200)), "fp16"),
    _shard_case("k_embed_wave_any", "int4", 1280, 4, 1, ((0, 6), (6, 200)), "bf16"),       # T = 1: the unigram ids are 5, 6 and 10
])
def test_partial_sums_of_a_row_shard_walk_several_sequences(family, fmt, d, max_n, T, ranges, dtype):
    """`embed_partial` on handles that own only rows [lo, hi): the PARTIAL instantiation of both kernels writes the fp32 sum over
    the OWNED ids of every token (kown < kfull) and the full hit count per walked token.  Then `finalize` of the added sums --
    k_finalize_wave at d = 768 / 1024 / 1280, k_embed's finalize mode elsewhere -- against the oracle's sum / K and combine."""
    from scone_amd.hip_backend import SconeTable
    B, T = SHAPES[T]
    _assert_regime(family, fmt, d, B, T)
    keys, lens = _vocabulary(max_n)
    table, stored, wte, wpe = _tables(fmt, d, max_n)
    tok, pos, _, off, ids = _batch(max_n, T)
    n = table.shape[0]
    kfull = np.diff(off)
    kmax = G.max_list_length(T, max_n)
    assert (np.bincount(kfull, minlength=kmax + 1) > 0).all()
    tag = f"{family}-{fmt}-d{d}-n{max_n}-{B}x{T}-partial-{dtype}"
    parts, want_total, handles = [], np.zeros((B * T, d), dtype=np.float32), []
    for lo, hi in ranges:
        t = SconeTable(max_n, n, d, fmt, row_begin=lo, row_end=hi)
        t.index_build(keys, lens)                                    # the index is replicated
        t.store_f32(torch.from_numpy(table[lo:hi]), row0=lo)
        want, kown = _own_sums(stored, off, ids, lo, hi)
        assert (kown < kfull).any() and (np.bincount(kown, minlength=1) > 0).all()      # part of a list, every owned length
        sums = torch.full((B * T, d), float("nan"), dtype=torch.float32, device="cuda")
        counts = torch.full((B * T,), SENTINEL, dtype=torch.int32, device="cuda")
        t.embed_partial(torch.from_numpy(tok), out=(sums, counts))
        got_k = counts.cpu().numpy()
        bad = np.argwhere((got_k != kfull).reshape(B, T))
        assert len(bad) == 0, (f"{tag} rows [{lo}, {hi}): counts differ at {len(bad)} of {B * T} tokens, first (b, i) "
                               f"{bad[:6].tolist()}: got {got_k.reshape(B, T)[tuple(bad[0])]}, K = {kfull.reshape(B, T)[tuple(bad[0])]}")
        g = sums.cpu().numpy()
        assert np.isfinite(want).all()
        assert E.same_bits(g, want), f"{tag} rows [{lo}, {hi}): partial sums: {_differing(g, want, B, T)}"
        assert t.status() == 0
        parts.append(sums)
        handles.append(t)
        want_total = want_total + want                                # what the reduce-scatter computes, shard order
    total = parts[0] if len(parts) == 1 else parts[0] + parts[1]
    kf = kfull.astype(np.float32)[:, None]
    mean = np.where(kf > 1, want_total / np.maximum(kf, np.float32(1)), want_total).astype(np.float32).reshape(B, T, d)
    dt = DTYPES[dtype]
    wte_t, wpe_t = _to(wte, dt).cuda(), _to(wpe, dt).cuda()
    want = R.combine(torch.from_numpy(tok), torch.from_numpy(mean), wte_t.float().cpu(), wpe_t.float().cpu(),
                     position_ids=torch.from_numpy(pos)).numpy()
    out = torch.full((B * T, d), float("nan"), dtype=dt, device="cuda")
    counts = torch.from_numpy(kfull.astype(np.int32)).cuda()
    half = (B * T) // 2 + 1
    for a, b in ((0, half), (half, B * T)):
        handles[-1].finalize(total[a:b], counts[a:b], torch.from_numpy(tok), a, b, wte=wte_t, wpe=wpe_t,
                             position_ids=torch.from_numpy(pos), out_dtype=dt, out=out[a:b])
    assert np.isfinite(want).all()
    g, w = _bits(out), _bits(_to(want.reshape(B * T, d), dt))
    assert E.same_bits(g, w), f"{tag}: finalize: {_differing(g, w, B, T)}"
    assert handles[-1].status() == 0
