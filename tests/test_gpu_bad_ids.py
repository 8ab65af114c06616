"""Out-of-range token and position ids through every copy of the lookup kernels' guard, against the oracle.

`wte[tok]` / `wpe[pos]` are read only for ids inside `[0, vocab)` / `[0, n_pos)`; any other id contributes a row of +0.0 and raises
bit 0 of `status()`.  That guard is written out in k_embed_wave (the FIXED_POS prologue and the walk with its prefetched ids),
k_embed_fused (rectangular and packed), k_embed_wave_any, k_finalize_wave, k_embed_select (specialised and any d) and the
lane-group fallback k_embed, and the kernels are also launched on SLICES of a batch (staged chunks, the SCONE_VARLEN_T
traversal and its remainder, the shard halves, finalize with tok_begin > 0), where the ids must move with the slice.  It is the
only thing between a padded batch (-1, -100, == vocab) and a read outside wte.

Inputs and expectation come from tests/bad_ids_fixture.py (host only; its properties are asserted by
tests/test_bad_ids_host.py): `(token_term + fg) + position_term` in fp32 numpy with every bad id mapped to a row of zeros, fg from
oracle/ref_port.py on the RAW tokens.  The bar has no tolerance -- fp32 output is bit-equal, fp16 / bf16 output equals the
expectation rounded once -- and it is the WHOLE output that is compared, so a bad id must leave every other row alone.

No case can fault when a guard is wrong: wte and wpe are the rows `buf[G : G + rows]` of an allocation whose G = 64 leading and
trailing rows hold the sentinel 12345, and no id lies farther than G rows outside its table, so a kernel that lost a test reads
the sentinel from memory this file owns and fails the comparison.  Outputs go into NaN-filled buffers with 64 guard rows.

After every lookup: `status()` is exactly the expected bit (bit 0 iff a position OF THE CALL has a bad id whose table was given;
a dense base has no vocabulary), reading cleared it, and a following clean call leaves it 0.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bad_ids_fixture as BI  # noqa: E402
import edge_fixture as E  # noqa: E402
import test_gpu_varlen as VL  # noqa: E402  (helpers only)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: rounding, bit views, the launch geometry)

pytestmark = pytest.mark.gpu

DTYPES = WS.DTYPES
GUARD = 64
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _form(monkeypatch, form):
    """SCONE_FUSED_MAX_TOKENS / SCONE_VARLEN_T are read when a handle is created.  "two_kernels_37": the packed traversal in rows
    of 37 tokens plus a remainder launch."""
    if form == "one_launch":
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    else:
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    if form == "two_kernels_37":
        monkeypatch.setenv("SCONE_VARLEN_T", "37")
    else:
        monkeypatch.delenv("SCONE_VARLEN_T", raising=False)


# ------------------------------------------------------------------ device buffers
def _between_sentinels(rows32, dt):
    """(the allocation, its rows [G : G + n] holding `rows32` in dt): what lies within G rows of the table is the sentinel."""
    n, d = rows32.shape
    buf = torch.full((n + 2 * BI.G, d), SENTINEL, dtype=dt, device="cuda")
    buf[BI.G:BI.G + n] = WS._to(rows32, dt).cuda()
    view = buf[BI.G:BI.G + n]
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + BI.G * d * buf.element_size()
    return buf, view


def _guarded(n, d, dt):
    buf = torch.full((n + GUARD, d), float("nan"), dtype=dt, device="cuda")
    return buf, buf[:n]


def _f32(t):
    return None if t is None else t.float().cpu().numpy().reshape(-1, t.shape[-1])


def _assert_bits(out, want32, dt, tag):
    assert want32.dtype == np.float32 and np.isfinite(want32).all()
    g, w = WS._bits(out.reshape(want32.shape)), WS._bits(WS._to(want32, dt))
    assert E.same_bits(g, w), f"{tag}: {VL._differing(g, w)}"


def _tables(fmt, d, max_n, mode="cover", **kw):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = BI.vocabulary(max_n)
    table = BI.tables(fmt, d, max_n)[0]
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt, lookup_mode=mode, **kw)
    cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    return cache


class _Inputs:
    """What a case hands to the lookup: the scenario's ids on the device, wte / wpe between sentinels, a dense base."""

    def __init__(self, sc, fmt, d, dtype, road, wpe, n_base=None):
        self.sc, self.dt = sc, DTYPES[dtype]
        _, _, wte32, wpe32 = BI.tables(fmt, d, sc.max_n)
        self.keep = []
        self.wte = self.wpe = self.base = None
        if road == "wte":
            buf, self.wte = _between_sentinels(wte32, self.dt)
            self.keep.append(buf)
        if wpe:
            buf, self.wpe = _between_sentinels(wpe32[:sc.n_pos], self.dt)
            self.keep.append(buf)
        if road == "base":
            n = len(sc.tok) if n_base is None else n_base
            self.base = WS._to(np.random.default_rng(5000 + n + d).standard_normal((n, d)).astype(np.float32), self.dt).cuda()
        self.packed = sc.batch in BI.PACKED
        shape = (-1,) if self.packed else BI.RECTS[sc.batch]
        self.tok = torch.from_numpy(sc.tok.astype(np.int32)).view(*shape).cuda()
        self.pos = None if (sc.pos is None or not wpe) else torch.from_numpy(sc.pos.astype(np.int32)).view(*shape).cuda()
        self.cu = torch.from_numpy(sc.cu.astype(np.int32)).cuda() if self.packed else None


def _after(table, want_bit, inp):
    """The status is exactly the expected bit; reading cleared it; a clean call leaves it 0."""
    got = table.status()
    assert got == want_bit, f"status {got:#x}, expected {want_bit:#x}"
    assert table.status() == 0
    tok = torch.tensor([[0, 1, 2, 3, 0], [2, 2, 1, 0, 3]], dtype=torch.int32, device="cuda")
    out = table.embed(tok, wte=inp.wte, wpe=inp.wpe, out_dtype=inp.dt)
    assert bool(torch.isfinite(out).all())
    assert table.status() == 0


def _run(batch, max_n, positions, fmt, d, mode, reduce, dtype, road="wte", wpe=True, inplace=False, table=None, then=None,
         **handle_kw):
    """One full lookup (scone_embed / _varlen / _base / _base_varlen by batch and road) against the expectation; `then()` runs
    right behind the lookup, before the clean call."""
    sc = BI.used(batch, max_n, positions)
    inp = _Inputs(sc, fmt, d, dtype, road, wpe)
    dt, total = inp.dt, len(sc.tok)
    t = _tables(fmt, d, max_n, mode, **handle_kw).table if table is None else table
    buf, out = _guarded(total, d, dt)
    base32 = _f32(inp.base)
    base = inp.base
    if inplace:
        out.copy_(base)
        base = out
    if road == "base":
        if inp.packed:
            got = t.embed_base_varlen(inp.tok, inp.cu, base, wpe=inp.wpe, position_ids=inp.pos, reduce=reduce, out=out)
        else:
            got = t.embed_base(inp.tok, base, wpe=inp.wpe, position_ids=inp.pos, reduce=reduce, out=out)
    elif inp.packed:
        got = t.embed_varlen(inp.tok, inp.cu, wte=inp.wte, wpe=inp.wpe, position_ids=inp.pos, reduce=reduce, out_dtype=dt, out=out)
    else:
        got = t.embed(inp.tok, wte=inp.wte, wpe=inp.wpe, position_ids=inp.pos, reduce=reduce, out_dtype=dt, out=out)
    assert got.data_ptr() == out.data_ptr()
    if then is not None:
        then()
    want = BI.expected(sc, fmt, d, mode, reduce, wte32=_f32(inp.wte), wpe32=_f32(inp.wpe), base32=base32)
    tag = f"{batch}-n{max_n}-pos_{positions}-{fmt}-d{d}-{mode}-{reduce}-{dtype}-{road}-wpe{int(wpe)}"
    _assert_bits(out, want, dt, tag)
    assert bool(torch.isnan(buf[total:]).all()), "a guard row behind the output was written"
    for b in inp.keep:                                           # nothing wrote into the sentinel rows either
        assert bool((b[:BI.G] == SENTINEL).all()) and bool((b[-BI.G:] == SENTINEL).all())
    _after(t, BI.status_bit(sc, road == "wte", wpe), inp)
    return t


def _rotate(setups):
    """Every set-up in cover mode and every second one in longest_suffix mode as well; reduce, output dtype and max_n in turn."""
    out, rot = [], ("fp32", "fp16", "bf16")
    for k, s in enumerate(setups):
        max_n, reduce = (3, 4)[k % 2], ("mean", "sum")[(k // 2) % 2]
        out.append(s + (max_n, "cover", reduce, rot[k % 3]))
        if k % 2 == 0:
            out.append(s + (max_n, "longest_suffix", "mean", rot[(k + 1) % 3]))
    return [pytest.param(*c, id="-".join(str(x) for x in c)) for c in out]


# ------------------------------------------------------------------ 1. scone_embed, one launch (k_embed_fused)
ONE_LAUNCH = [("fp32", 768, "9x37", "explicit", "wte"), ("fp16", 768, "9x37", "default", "wte"), ("int8", 768, "9x37", "short", "wte"),
              ("bf16", 768, "33x3", "explicit", "wte"), ("fp16", 768, "33x3", "default", "wte"),
              ("fp16", 1024, "9x37", "explicit", "wte"), ("int4", 1024, "9x37", "default", "wte"),
              ("mxfp4", 1024, "9x37", "short", "wte"), ("fp32", 1024, "33x3", "explicit", "none"),
              ("int8", 1024, "33x3", "default", "wte"),
              ("fp32", 1280, "9x37", "explicit", "none"), ("fp16", 1280, "9x37", "default", "wte"),
              ("fp32", 1280, "9x37", "short", "none"), ("int8", 1280, "33x3", "explicit", "wte"), ("fp16", 1280, "33x3", "default", "wte")]


@pytest.mark.parametrize("fmt,d,batch,positions,road,max_n,mode,reduce,dtype", _rotate(ONE_LAUNCH))
def test_embed_one_launch(monkeypatch, fmt, d, batch, positions, road, max_n, mode, reduce, dtype):
    """k_embed_fused, rectangular: explicit ids (negative, >= n_pos), default positions, default positions with n_pos < T."""
    _form(monkeypatch, "one_launch")
    assert WS.G.takes_one_launch(fmt, d, len(BI.used(batch, max_n, positions).tok))
    _run(batch, max_n, positions, fmt, d, mode, reduce, dtype, road)


# ------------------------------------------------------------------ 2. scone_embed, two kernels (k_embed_wave)
TWO_KERNELS = [("int8", 768, "1243x37", "explicit", "wte"), ("fp16", 768, "1243x37", "default", "wte"),
               ("fp32", 768, "1243x37", "short", "wte"), ("fp16", 768, "7x5", "explicit", "wte"), ("bf16", 768, "7x5", "default", "wte"),
               ("fp16", 1024, "1243x37", "short", "wte"), ("int4", 1024, "7x5", "explicit", "wte"),
               ("mxfp4", 1024, "7x5", "default", "wte"), ("fp32", 1024, "9x37", "short", "none"),
               ("fp16", 1280, "1243x37", "explicit", "wte"), ("int8", 1280, "7x5", "explicit", "none"),
               ("fp32", 1280, "7x5", "default", "wte"), ("fp16", 1280, "9x37", "short", "wte")]


@pytest.mark.parametrize("fmt,d,batch,positions,road,max_n,mode,reduce,dtype", _rotate(TWO_KERNELS))
def test_embed_two_kernels(monkeypatch, fmt, d, batch, positions, road, max_n, mode, reduce, dtype):
    """k_embed_wave: 1243 x 37 makes a workgroup walk several sequences (the bad ids of the later ones arrive through the
    prefetched tokn / posn); default positions take the FIXED_POS prologue, whose position i >= n_pos is bad for the whole run."""
    _form(monkeypatch, "two_kernels")
    assert WS.G.kernel_family(fmt, d) == "k_embed_wave"
    if batch == "1243x37":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert all(g.seqs_per_block >= 3 for g in WS.G.wave_all(1243, 37, cus))
    _run(batch, max_n, positions, fmt, d, mode, reduce, dtype, road)


# ------------------------------------------------------------------ 3. any d (k_embed_wave_any) and the lane-group fallback (k_embed)
ANY_D = [("int8", 2048, "9x37", "explicit", "wte"), ("fp16", 2048, "9x37", "short", "wte"), ("int4", 2048, "7x5", "default", "wte"),
         ("fp32", 136, "9x37", "explicit", "wte"), ("fp32", 136, "1243x37", "explicit", "wte"), ("fp16", 136, "9x37", "short", "none"),
         ("fp32", 136, "7x5", "default", "wte")]


@pytest.mark.parametrize("fmt,d,batch,positions,road,max_n,mode,reduce,dtype", _rotate(ANY_D))
def test_embed_any_dim(monkeypatch, fmt, d, batch, positions, road, max_n, mode, reduce, dtype):
    _form(monkeypatch, "two_kernels")
    assert WS.G.kernel_family(fmt, d) == "k_embed_wave_any"
    if batch == "1243x37":
        assert WS.G.wave_any(1243, 37).seqs_per_block >= 3
    _run(batch, max_n, positions, fmt, d, mode, reduce, dtype, road)


@pytest.mark.parametrize("batch,positions,road,max_n,reduce,dtype", [
    ("9x37", "explicit", "wte", 3, "mean", "fp32"), ("9x37", "short", "wte", 4, "sum", "fp16"),
    ("9x37", "default", "wte", 4, "mean", "fp32"), ("33x3", "explicit", "none", 3, "mean", "fp32"),
    ("7x5", "explicit", "wte", 4, "sum", "fp32")])
def test_embed_lane_group_fallback(batch, positions, road, max_n, reduce, dtype):
    """k_embed (d % 8 != 0): fp32 table, d = 100, rectangular; cover mode (the paper's lookup needs d % 8 == 0)."""
    assert WS.G.kernel_family("fp32", 100) == "k_embed"
    _run(batch, max_n, positions, "fp32", 100, "cover", reduce, dtype, road)


# ------------------------------------------------------------------ 4. packed batches (scone_embed_varlen)
VARLEN = [("one_launch", "int8", 768, "small", "explicit"), ("one_launch", "fp16", 1024, "small", "short"),
          ("one_launch", "fp32", 1280, "tiny", "explicit"), ("one_launch", "bf16", 768, "tiny", "short"),
          ("one_launch", "fp16", 768, "small", "default"),
          ("two_kernels", "fp16", 768, "small", "explicit"), ("two_kernels", "int8", 1024, "small", "short"),
          ("two_kernels", "int8", 2048, "small", "explicit"), ("two_kernels", "fp32", 768, "tiny", "explicit"),
          ("two_kernels", "fp32", 136, "tiny", "short"),
          ("two_kernels_37", "int8", 768, "small", "explicit"), ("two_kernels_37", "fp16", 1280, "small", "short"),
          ("two_kernels_37", "fp16", 2048, "small", "default"), ("two_kernels_37", "fp32", 1024, "small", "explicit")]


@pytest.mark.parametrize("form,fmt,d,batch,positions,max_n,mode,reduce,dtype", _rotate(VARLEN))
def test_embed_varlen(monkeypatch, form, fmt, d, batch, positions, max_n, mode, reduce, dtype):
    """k_embed_fused<VARLEN>, and the two-kernel traversal: the stream as one row, or (SCONE_VARLEN_T = 37) rows of 37 tokens plus
    a remainder launch that holds the batch's last bad ids.  "short": a sequence longer than n_pos with default positions
    (p - cu[s] >= n_pos)."""
    _form(monkeypatch, form)
    sc = BI.used(batch, max_n, positions)
    total = len(sc.tok)
    if form == "two_kernels_37":
        main = total - total % 37
        assert total > 3 * 37 and total % 37 and (sc.bad_tok | sc.bad_pos)[main:].any() and (sc.bad_tok | sc.bad_pos)[:main].any()
    if positions == "short":
        assert (np.diff(sc.cu) > sc.n_pos).any()
    _run(batch, max_n, positions, fmt, d, mode, reduce, dtype, "wte")


# ------------------------------------------------------------------ 5. a dense base: positions only
BASE = [("one_launch", "int8", 768, "9x37", "explicit"), ("one_launch", "fp16", 1024, "9x37", "short"),
        ("one_launch", "fp32", 1280, "small", "explicit"), ("one_launch", "fp16", 768, "small", "short"),
        ("two_kernels", "fp16", 768, "1243x37", "explicit"), ("two_kernels", "int8", 1024, "9x37", "short"),
        ("two_kernels", "int8", 2048, "7x5", "explicit"), ("two_kernels_37", "fp32", 768, "small", "explicit"),
        ("two_kernels", "fp16", 1280, "small", "short"), ("two_kernels", "fp32", 768, "9x37", "default")]


@pytest.mark.parametrize("form,fmt,d,batch,positions,max_n,mode,reduce,dtype", _rotate(BASE))
def test_embed_base(monkeypatch, form, fmt, d, batch, positions, max_n, mode, reduce, dtype):
    """scone_embed_base / _base_varlen: negative and >= n_pos position ids raise the bit and read zeros; the scenario's bad TOKENS
    serve the match only -- with clean positions ("default") the status stays 0."""
    _form(monkeypatch, form)
    _run(batch, max_n, positions, fmt, d, mode, reduce, dtype, "base")


@pytest.mark.parametrize("form,batch", [("two_kernels", "9x37"), ("one_launch", "small")])
def test_embed_base_in_place(monkeypatch, form, batch):
    _form(monkeypatch, form)
    _run(batch, 3, "explicit", "int8", 768, "cover", "mean", "fp16", "base", inplace=True)


# ------------------------------------------------------------------ 6. chosen positions (scone_embed_select)
def _run_select(batch, max_n, positions, fmt, d, mode, reduce, dtype, road, clean_only=False):
    sc = BI.used(batch, max_n, positions)
    sel = BI.selection(batch, max_n, positions, clean_only)
    n_sel = len(sel)
    inp = _Inputs(sc, fmt, d, dtype, road, True, n_base=n_sel)
    dt = inp.dt
    t = _tables(fmt, d, max_n, mode).table
    buf, out = _guarded(n_sel, d, dt)
    pos = None if sc.pos is None else torch.from_numpy(sc.pos[sel].astype(np.int32))
    got = t.embed_select(inp.tok, torch.from_numpy(sel), cu_seqlens=inp.cu, wte=inp.wte, base=inp.base, wpe=inp.wpe, position_ids=pos,
                         reduce=reduce, out_dtype=dt, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = BI.expected(sc, fmt, d, mode, reduce, wte32=_f32(inp.wte), wpe32=_f32(inp.wpe), base32=_f32(inp.base), rows=sel)
    _assert_bits(out, want, dt, f"select-{batch}-n{max_n}-pos_{positions}-{fmt}-d{d}-{mode}-{reduce}-{dtype}-{road}-clean{int(clean_only)}")
    assert bool(torch.isnan(buf[n_sel:]).all()), "a guard row behind the output was written"
    bit = BI.status_bit(sc, road == "wte", True, rows=sel)
    if clean_only:
        assert bit == 0 and sc.bad_tok.any()              # the batch holds bad tokens; none of them is selected
    elif road == "wte" or positions != "default":
        assert bit == 1
    _after(t, bit, inp)


SELECT = [("int8", 768, "9x37", "explicit", "wte"), ("fp16", 768, "small", "explicit", "wte"), ("fp32", 768, "9x37", "explicit", "base"),
          ("fp16", 1024, "small", "short", "wte"), ("mxfp4", 1024, "9x37", "short", "base"), ("bf16", 1024, "small", "explicit", "base"),
          ("fp16", 1280, "9x37", "default", "wte"), ("int8", 1280, "tiny", "explicit", "wte"),
          ("int8", 2048, "9x37", "explicit", "wte"), ("fp16", 2048, "small", "explicit", "base"), ("int4", 2048, "small", "short", "wte"),
          ("fp32", 136, "small", "explicit", "wte"), ("fp32", 136, "9x37", "short", "base"), ("fp16", 136, "tiny", "default", "wte")]


@pytest.mark.parametrize("fmt,d,batch,positions,road,max_n,mode,reduce,dtype", _rotate(SELECT))
def test_embed_select(fmt, d, batch, positions, road, max_n, mode, reduce, dtype):
    """k_embed_select, specialised (768 / 1024 / 1280) and any d: the selection holds every bad position and its neighbours; the
    token, the position id and the base row are those of OUTPUT j."""
    _run_select(batch, max_n, positions, fmt, d, mode, reduce, dtype, road)


@pytest.mark.parametrize("fmt,d,batch,mode", [("int8", 768, "9x37", "cover"), ("fp16", 1024, "small", "longest_suffix"),
                                              ("int8", 2048, "small", "cover"), ("fp32", 136, "9x37", "longest_suffix")])
def test_embed_select_bad_token_at_an_unselected_position_raises_nothing(fmt, d, batch, mode):
    _run_select(batch, 3, "explicit", fmt, d, mode, "mean", "fp16" if fmt != "fp32" else "fp32", "wte", clean_only=True)


# ------------------------------------------------------------------ 7. scone_embed_partial + scone_finalize on a slice
@pytest.mark.parametrize("fmt,d,positions,max_n,mode,reduce,dtype", [
    ("int8", 768, "explicit", 3, "cover", "mean", "fp16"), ("fp16", 768, "short", 4, "cover", "sum", "fp32"),
    ("fp32", 1024, "default", 3, "cover", "mean", "bf16"),
    ("int8", 768, "explicit", 4, "longest_suffix", "mean", "fp32"), ("fp16", 1024, "short", 3, "longest_suffix", "mean", "fp16"),
    ("fp32", 1280, "default", 3, "longest_suffix", "sum", "bf16"),
    ("fp32", 100, "explicit", 4, "cover", "mean", "fp32"), ("fp32", 100, "short", 3, "cover", "mean", "fp16")])
def test_finalize_of_a_slice(monkeypatch, fmt, d, positions, max_n, mode, reduce, dtype):
    """finalize(tok_begin > 0): k_finalize_wave at d = 768 / 1024, k_embed's finalize mode at d = 100.  The middle third holds bad
    ids (and so does the rest of the batch); the clean sequence holds none although the batch around it does: only the ids
    INSIDE the slice may raise the bit, and tok / pos are those of the slice.  On a longest_suffix handle (k_finalize_wave has its
    own `use_wte`; d = 100 cannot run in that mode, it needs d % 8 == 0) the partial sums hold the one f-gram row of the paper's
    lookup, the counts are 0 / 1, and the slice starts in front of a bad token on a MATCHED position: it gets the f-gram row
    and the bit is raised all the same."""
    _form(monkeypatch, "two_kernels")
    batch = "9x37"
    sc = BI.used(batch, max_n, positions)
    B, T = BI.RECTS[batch]
    total = B * T
    inp = _Inputs(sc, fmt, d, dtype, "wte", True)
    dt = inp.dt
    t = _tables(fmt, d, max_n, mode).table
    sums = torch.full((total, d), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    t.embed_partial(inp.tok, out=(sums, counts))
    matched = BI.suffix_ids(batch, max_n, positions) >= 0
    K = np.diff(BI.lists(batch, max_n, positions)[0]) if mode == "cover" else matched.astype(np.int64)
    assert np.array_equal(counts.cpu().numpy(), K)
    assert t.status() == 0                                        # no wte / wpe: nothing to be out of
    want = BI.expected(sc, fmt, d, mode, reduce, wte32=_f32(inp.wte), wpe32=_f32(inp.wpe))
    bad = sc.bad_tok | sc.bad_pos
    a = total // 3
    if mode == "longest_suffix":                                  # start two tokens in front of a bad token on a matched position
        on_match = np.nonzero(sc.bad_tok & matched)[0]
        a = min(a, int(on_match[on_match >= 3][0]) - 2)
        assert (sc.bad_tok & matched)[a:2 * total // 3].any() and (sc.bad_tok & ~matched)[a:2 * total // 3].any()
    slices = [(a, 2 * total // 3, 1)]
    if sc.clean_seq is not None:
        slices.append(sc.clean_seq + (0,))
    for a, b, bit in slices:
        assert a > 0 and bool(bad[a:b].any()) == bool(bit) and bad[:a].any() and bad[b:].any()
        buf, out = _guarded(b - a, d, dt)
        t.finalize(sums[a:b], counts[a:b], inp.tok, a, b, wte=inp.wte, wpe=inp.wpe, position_ids=inp.pos, reduce=reduce,
                   out_dtype=dt, out=out)
        _assert_bits(out, want[a:b], dt, f"finalize-[{a}, {b})-{fmt}-d{d}-n{max_n}-pos_{positions}-{mode}-{reduce}-{dtype}")
        assert bool(torch.isnan(buf[b - a:]).all())
        assert BI.status_bit(sc, True, True, rows=np.arange(a, b)) == bit
        _after(t, bit, inp)


# ------------------------------------------------------------------ 8. a staged pinned-host table: every chunk is a slice
@pytest.mark.parametrize("positions,max_n,mode,dtype", [("explicit", 3, "cover", "fp16"), ("default", 4, "cover", "fp32"),
                                                        ("explicit", 4, "longest_suffix", "bf16")])
def test_staged_pinned_host_table(positions, max_n, mode, dtype):
    """stage_tokens = 128, T = 37: chunks of 3 sequences, B = 7 -> 3 chunks, the last of one sequence -- which holds bad ids, as
    do the chunks before it.  Every chunk's tok / pos start t0 tokens in."""
    sc = BI.used("7x37", max_n, positions)
    bad = sc.bad_tok | sc.bad_pos
    assert bad[6 * 37:].any() and bad[:3 * 37].any() and bad[3 * 37:6 * 37].any()
    t = _tables("int8", 768, max_n, mode, placement="pinned_host", hot_rows=16, stage_tokens=128).table
    before = t.stage_counters()["chunks"]

    def three_chunks():
        c = t.stage_counters()
        assert c["chunk_tokens"] // 37 == 3 and c["chunks"] - before == 3, c
    _run("7x37", max_n, positions, "int8", 768, mode, "mean", dtype, "wte", table=t, then=three_chunks)


# ------------------------------------------------------------------ 9. the shard halves on a range of sequences
def _shard_table(fmt, d, max_n, mode="cover"):
    from scone_amd.hip_backend import SconeTable
    keys, lens = BI.vocabulary(max_n)
    table = BI.tables(fmt, d, max_n)[0]
    t = SconeTable(max_n, len(lens), d, fmt, lookup_mode=mode)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(table))
    return t


def _ranges(sc, B, T):
    """[1, c): sequences with bad ids, seq_begin > 0; [c, c + 1): the clean sequence, bad ids on either side of it."""
    c = sc.clean_seq[0] // T
    bad = sc.bad_tok | sc.bad_pos
    assert c >= 2 and bad[T:c * T].any() and bad[:T].any() and bad[(c + 1) * T:].any() and not bad[c * T:(c + 1) * T].any()
    matched = BI.suffix_ids(sc.batch, sc.max_n, sc.positions) >= 0
    assert (sc.bad_tok & matched)[T:c * T].any()            # the paper's lookup: a bad token on a matched position in the range
    return [(1, c, 1), (c, c + 1, 0)]


@pytest.mark.parametrize("fmt,d,positions,max_n,mode,reduce,dtype", [
    ("int8", 768, "explicit", 3, "cover", "mean", "fp16"), ("fp16", 2048, "explicit", 4, "cover", "sum", "fp32"),
    ("int8", 1024, "default", 4, "cover", "mean", "fp16"),
    ("int8", 768, "explicit", 4, "longest_suffix", "mean", "fp32"), ("fp16", 2048, "default", 3, "longest_suffix", "mean", "fp16")])
def test_shard_gather_embed_range(fmt, d, positions, max_n, mode, reduce, dtype):
    """scone_shard_gather_embed_range at world 1 (one handle plans, packs and receives its own records): d_tok + t0, d_pos + t0.
    On a longest_suffix handle the plan holds the paper's lists and the range a bad token on a matched position."""
    batch = "9x37"
    B, T = BI.RECTS[batch]
    sc = BI.used(batch, max_n, positions)
    inp = _Inputs(sc, fmt, d, dtype, "wte", True)
    dt = inp.dt
    t = _shard_table(fmt, d, max_n, mode)
    m = t.shard_gather_plan_chunks(inp.tok, 1)[0]
    assert m > 0
    records = torch.empty((m, t.shard_record_bytes()), dtype=torch.uint8, device="cuda")
    t.shard_gather_pack_range(0, m, records)
    t.shard_gather_add_records(records, 0, m)
    want = BI.expected(sc, fmt, d, mode, reduce, wte32=_f32(inp.wte), wpe32=_f32(inp.wpe))
    for s0, s1, bit in _ranges(sc, B, T):
        buf, out = _guarded(B * T, d, dt)
        t.shard_gather_embed_range(inp.tok, s0, s1, records, out, wte=inp.wte, wpe=inp.wpe, position_ids=inp.pos, reduce=reduce)
        _assert_bits(out[s0 * T:s1 * T], want[s0 * T:s1 * T], dt, f"gather range [{s0}, {s1})-{fmt}-d{d}-n{max_n}-pos_{positions}-{mode}")
        assert bool(torch.isnan(buf[:s0 * T]).all()) and bool(torch.isnan(buf[s1 * T:]).all()), "a row outside the range was written"
        assert BI.status_bit(sc, True, True, rows=np.arange(s0 * T, s1 * T)) == bit
        _after(t, bit, inp)


@pytest.mark.parametrize("fmt,d,positions,max_n,mode,reduce,dtype", [
    ("int8", 768, "explicit", 3, "cover", "mean", "fp16"), ("fp16", 1280, "explicit", 4, "cover", "sum", "fp32"),
    ("int8", 2048, "default", 3, "cover", "mean", "fp32"),
    ("fp16", 1024, "explicit", 3, "longest_suffix", "mean", "fp16"), ("int8", 2048, "explicit", 4, "longest_suffix", "mean", "fp32")])
def test_shard_cols_embed(fmt, d, positions, max_n, mode, reduce, dtype):
    """scone_shard_cols_embed at world 1 (columns on the wire, lists resolved through the handle's own fragment)."""
    batch = "9x37"
    B, T = BI.RECTS[batch]
    sc = BI.used(batch, max_n, positions)
    inp = _Inputs(sc, fmt, d, dtype, "wte", True)
    dt = inp.dt
    t = _shard_table(fmt, d, max_n, mode)
    n = t.shard_gather_plan_chunks(inp.tok, 1)[0]
    assert n > 0
    slots, sb = t.cols_frag_slots(n), t.scale_bytes()
    rows = torch.empty((n, t.payload_bytes()), dtype=torch.uint8, device="cuda")
    scales = torch.empty((n, sb), dtype=torch.uint8, device="cuda") if sb else None
    frags = torch.empty(slots, dtype=torch.int64, device="cuda")
    t.shard_cols_pack(0, n, rows, scales, frags)
    want = BI.expected(sc, fmt, d, mode, reduce, wte32=_f32(inp.wte), wpe32=_f32(inp.wpe))
    for s0, s1, bit in _ranges(sc, B, T):
        buf, out = _guarded(B * T, d, dt)
        t.shard_cols_embed(inp.tok, s0, s1, rows, n, scales, frags, [0], [slots], [0], out, wte=inp.wte, wpe=inp.wpe,
                           position_ids=inp.pos, reduce=reduce)
        _assert_bits(out[s0 * T:s1 * T], want[s0 * T:s1 * T], dt, f"cols range [{s0}, {s1})-{fmt}-d{d}-n{max_n}-pos_{positions}-{mode}")
        assert bool(torch.isnan(buf[:s0 * T]).all()) and bool(torch.isnan(buf[s1 * T:]).all()), "a row outside the range was written"
        assert BI.status_bit(sc, True, True, rows=np.arange(s0 * T, s1 * T)) == bit
        _after(t, bit, inp)


# ------------------------------------------------------------------ 10. embed_tokens(check=True)
@pytest.mark.parametrize("form", ["one_launch", "two_kernels"])
def test_check_raises_index_error_on_each_road(monkeypatch, form):
    """plain, cu_seqlens=, base= (positions only) and select=: IndexError with the bad ids, none with clean ones."""
    _form(monkeypatch, form)
    fmt, d, max_n, dtype = "int8", 768, 3, "fp16"
    cache = _tables(fmt, d, max_n)
    for batch in ("9x37", "tiny"):
        sc = BI.used(batch, max_n, "explicit")
        tok0, _, pos0 = BI.clean_batch(batch, max_n)
        total = len(sc.tok)
        shape = (-1,) if batch in BI.PACKED else BI.RECTS[batch]
        inp = _Inputs(sc, fmt, d, dtype, "wte", True)
        base = torch.zeros((total, d), dtype=inp.dt, device="cuda")
        sel = torch.from_numpy(BI.selection(batch, max_n, "explicit"))
        kw = dict(cu_seqlens=None if inp.cu is None else inp.cu)
        good_tok, good_pos = torch.from_numpy(tok0).view(*shape), torch.from_numpy(pos0).view(*shape)
        roads = [
            ("plain / packed", dict(wte=inp.wte, wpe=inp.wpe), False),
            ("base", dict(base=base.view(*shape, d) if inp.cu is None else base, wpe=inp.wpe), False),
            ("select", dict(wte=inp.wte, wpe=inp.wpe, select=sel), True),
        ]
        for name, extra, selected in roads:
            def ids(t):
                return t.reshape(-1)[sel] if selected else t
            for tok, pos, raises in ((inp.tok, good_pos, "base" not in extra), (good_tok, inp.pos.cpu(), True), (good_tok, good_pos, False)):
                call = dict(kw, position_ids=ids(pos), check=True, **extra)
                if raises:
                    with pytest.raises(IndexError):
                        cache.embed_tokens(tok, **call)
                else:
                    cache.embed_tokens(tok, **call)
                assert cache.table.status() == 0, (batch, name)
