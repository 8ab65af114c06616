"""Every row-walking kernel at rows wider than d = 4096, against the oracle.  Run with ``-m gpu`` on an MI355X.

include/scone_hip.h allows any width that the format's divisibility rule allows; the other suites stop at d = 4096 (fp16 / bf16 /
MXFP4) or 2048 (fp32 / int8 / INT4).  Beyond that the lanes stride further through a row, a row carries more scale bytes (MXFP4
d / 32, INT4 d / 64), the records of the shard exchange grow and `embed_units` walks more than 64 units.  The (format, d) pairs,
the batches and the expectations are tests/wide_rows_fixture.py's; tests/test_wide_rows_host.py checks what is taken for
granted about them.

As in the other oracle suites: tables are quantised on the HOST, the expectation is oracle/ref_port.py on the fp32 values the
format stands for and never passes through HIP code, every output buffer is pre-filled with NaN (counts: with -7), fp32 output
equals the oracle's bit for bit, fp16 / bf16 output equals the oracle's fp32 result rounded once, there is NO tolerance, and
`status() == 0` after every case.  SCONE_FUSED_MAX_TOKENS=0 is set before a handle exists (none of these widths has a
one-launch kernel anyway).

Roads, for every (format, d):
  quantiser and raw rows   store_f32 + gather_rows, download, upload, store_f32_ids
  synthetic fill           fill_synthetic against its host twin (oracle/ref_port.py `synth_rows_*` / `synth_scale_f16`; fp32 /
                           fp16 / bf16 rows are the int8 fill's dequantised values, rounded; MXFP4: tests/mxfp4_fixture.py) --
                           every format has a twin, none is skipped
  two-kernel embed         k_match_ell + k_embed_wave_any (the lane-group k_embed at d = 4100): cover and longest_suffix, mean
                           and sum, default and explicit positions, fp32 and one half-precision output, with and without wte;
                           the 8200-sequence batch in which a workgroup walks 3 sequences, once per format
  embed_varlen, embed_base (also out == base), embed_select (rectangular and packed, unsorted and repeated selections);
                           fp32 4100: embed_varlen and embed_select refuse d % 8 != 0, as the header documents -- asserted
  gather_reduce            lists of 0, 1, 10, 11 and 40 ids (these widths take the lane-group CSR road), a dense base, a handle
                           that owns only rows [20, 60)
  embed_partial + finalize two row shards whose sums are added
and for the formats with scales at d >= 5120 plus fp16 8192 (the control without scales):
  pinned host, in place    rows >= 16 read over PCIe by the lookup kernel
  pinned host, staged      through the HBM cache of cold rows in chunks of 4, 4 and 1 sequences, twice: the second pass copies
                           nothing, the first exactly the distinct cold rows the batch references
  shard exchange           three shards on one GPU, a replicated head of 0 and of 5 rows, records and columns
and, where the cached rows carry scales, two small tables whose cache (84 slots) is smaller than what the batch references:
INT4 d = 1024 (its permuted scale order) and MXFP4 d = 5120.

The staged cases are what found k_stage_copy's one-pass copy of a row's scales (at most 128 bytes: MXFP4 above d = 4096 and
INT4 above d = 8192 lost the rest, silently); INT4 8192 (exactly 128 bytes), int8 and fp16 are the controls that pass either way.

`tools/wide_rows_mutants.sh` puts that form of k_stage_copy back and breaks three generic walks, all in bounds, and shows that
this file fails on each by comparison (profiles/r14a): `stage_copy_one_pass` 4 cases (staged MXFP4 5120 / 8192 and INT4 16384,
first differing element 4096 resp. 8192, and the MXFP4 eviction case; staged INT4 8192, int8 and fp16 pass),
`units_stop_at_64` 88, `gather_rows_slot0` 8, `cols_pack_first_pass` 6.
"""

import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_fixture as E  # noqa: E402
import mxfp4_fixture as MX  # noqa: E402
import test_gpu_walk_shapes as W  # noqa: E402
import wide_rows_fixture as F  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
ALL = [pytest.param(*c, id=F.case_id(c)) for c in F.CASES]
SCALED = [pytest.param(*c, id=F.case_id(c)) for c in F.STAGED]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


@pytest.fixture(autouse=True)
def two_kernels(monkeypatch):
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")


def _half(fmt, d):
    """The half-precision output dtype of a case: fp16 and bf16 in turn."""
    return (torch.float16, torch.bfloat16)[F.CASES.index((fmt, d)) % 2]


def _handle(fmt, d, lo=0, hi=None, **kw):
    from scone_amd.hip_backend import SconeTable
    keys, lens = F.vocabulary()
    n = F.n_rows()
    hi = n if hi is None else hi
    t = SconeTable(F.MAX_N, n, d, fmt, row_begin=lo, row_end=hi, **kw)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(F.tables(fmt, d)["table"][lo:hi]), row0=lo)
    return t


def _same(got, want32, dt, what):
    g = W._bits(got)
    w = W._bits(W._to(want32, dt).reshape(got.shape))
    assert E.same_bits(g, w), (what, E.first_difference(g, w))


def _dev(x32, dt):
    return W._to(x32, dt).cuda()


def _f32(t):
    return t.float().cpu().numpy()


def _embed(t, tok, dt, **kw):
    B, T = tok.shape
    out = torch.full((B, T, t.dim), NAN, dtype=dt, device="cuda")
    got = t.embed(torch.from_numpy(tok), out_dtype=dt, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return out


def _holds(t, payload, scales, row0=0, what=""):
    gp, gs = t.download(row0, len(payload))
    assert np.array_equal(gp, payload), (what, "payload", np.argwhere(gp != payload)[:5].tolist())
    if scales is None:
        assert gs is None
    else:
        gs, ws = np.ascontiguousarray(gs).view(np.uint8), np.ascontiguousarray(scales).view(np.uint8)
        assert gs.shape == ws.reshape(len(payload), -1).shape, (what, gs.shape)
        assert np.array_equal(gs, ws.reshape(gs.shape)), (what, "scales", np.argwhere(gs != ws.reshape(gs.shape))[:5].tolist())


# ------------------------------------------------------------------ the quantiser and the raw-row entry points
@pytest.mark.parametrize("fmt,d", ALL)
def test_quantiser_and_raw_rows(fmt, d):
    """store_f32 then gather_rows = host quantise then dequantise; download = the host payload and scales in logical order;
    upload of the host payload gives the same gather_rows; store_f32_ids writes scattered rows."""
    from scone_amd.hip_backend import SconeTable
    x = F.tables(fmt, d)
    n = F.n_rows()
    every = torch.arange(n)
    t = SconeTable(F.MAX_N, n, d, fmt)
    t.store_f32(torch.from_numpy(x["table"]))
    assert (t.payload_bytes(), t.scale_bytes()) == (F.payload_bytes(fmt, d), F.scale_bytes(fmt, d))
    got = t.gather_rows(every).cpu().numpy()
    assert E.same_bits(got, x["stored"]), ("store_f32 + gather_rows", E.first_difference(got, x["stored"]))
    _holds(t, x["payload"], x["scales"], what="store_f32")
    _holds(t, x["payload"][n - 7:], None if x["scales"] is None else x["scales"][n - 7:], row0=n - 7, what="download of the last rows")
    t2 = SconeTable(F.MAX_N, n, d, fmt)
    t2.upload(x["payload"], x["scales"])
    got = t2.gather_rows(every).cpu().numpy()
    assert E.same_bits(got, x["stored"]), ("upload + gather_rows", E.first_difference(got, x["stored"]))
    _holds(t2, x["payload"], x["scales"], what="upload")
    rng = np.random.default_rng(d)
    perm = rng.permutation(n)[:n - 9]                                  # scattered, and 9 rows stay as they were
    t3 = SconeTable(F.MAX_N, n, d, fmt)
    t3.upload(x["payload"][::-1].copy(), None if x["scales"] is None else x["scales"][::-1].copy())
    t3.store_f32(torch.from_numpy(x["table"][perm]), ids=torch.from_numpy(perm))
    want = x["stored"][::-1].copy()
    want[perm] = x["stored"][perm]
    got = t3.gather_rows(every).cpu().numpy()
    assert E.same_bits(got, want), ("store_f32_ids", E.first_difference(got, want))
    ids = torch.from_numpy(np.array([n - 1, 0, 17, n - 1, 3]))
    got = t.gather_rows(ids).cpu().numpy()
    assert E.same_bits(got, x["stored"][ids.numpy()])
    assert t.status() == 0 and t2.status() == 0 and t3.status() == 0


@pytest.mark.parametrize("fmt,d", ALL)
def test_synthetic_fill_is_its_host_twin(fmt, d):
    """Rows 0, 1, 17, 41 and the last one of a synthetic table: raw bytes and dequantised values."""
    from scone_amd.hip_backend import SconeTable
    n, seed, scale = F.n_rows(), 11, 0.02 / 127
    t = SconeTable(F.MAX_N, n, d, fmt)
    t.fill_synthetic(seed, scale)
    sample = np.array([0, 1, 17, 41, n - 1], dtype=np.int64)
    if fmt == "mxfp4":
        payload, scales = MX.synthetic(seed, sample, d, scale)
        stored = MX.dequantize(payload, scales)
    elif fmt == "int4":
        payload, scales = R.synth_rows_i4(seed, sample, d, scale)
        stored = R.dequantize_i4(payload, scales)
    else:
        q = R.synth_rows_i8(seed, sample, d)
        s = R.synth_scale_f16(seed, sample, scale)
        v = R.dequantize_i8(q, s)                                      # fp32(q) * fp32(scale): what the other formats round
        if fmt == "int8":
            payload, scales, stored = q.view(np.uint8), s.reshape(-1, 1), v
        else:
            payload, scales, stored = F.quantise(fmt, v)
    for k, r in enumerate(sample):
        _holds(t, payload[k:k + 1], None if scales is None else scales[k:k + 1], row0=int(r), what=f"row {r}")
    got = t.gather_rows(torch.from_numpy(sample)).cpu().numpy()
    assert E.same_bits(got, stored), E.first_difference(got, stored)
    assert t.status() == 0


# ------------------------------------------------------------------ the two-kernel lookup
# (reduce, positions, 0 = fp32 / 1 = the case's half precision, with wte): each rectangle meets mean and sum with default and
# explicit positions; dtype and wte alternate, and the two rectangles take complementary halves of the 16 combinations
COMBOS = {"9x37": (("mean", "default", 0, True), ("sum", "explicit", 1, False), ("mean", "explicit", 1, True), ("sum", "default", 0, False)),
          "7x5": (("mean", "explicit", 0, False), ("sum", "default", 1, True), ("mean", "default", 1, False), ("sum", "explicit", 0, True))}


# (the paper's lookup needs d % 8 == 0: fp32 4100 runs in cover mode only)
MODES = [pytest.param(*c, m, id=f"{F.case_id(c)}-{m}") for c in F.CASES for m in ("cover", "longest_suffix") if m == "cover" or c[1] % 8 == 0]


@pytest.mark.parametrize("fmt,d,mode", MODES)
def test_two_kernel_embed(fmt, d, mode):
    assert F.kernel_family(fmt, d) == ("k_embed" if d % 8 else "k_embed_wave_any")
    x = F.tables(fmt, d)
    t = _handle(fmt, d, lookup_mode=mode)
    for name in F.RECTS:
        tok, pos = F.rect(name)
        for reduce, positions, half, with_wte in COMBOS[name]:
            dt = _half(fmt, d) if half else torch.float32
            wte_t, wpe_t = _dev(x["wte"], dt) if with_wte else None, _dev(x["wpe"], dt)
            p = pos if positions == "explicit" else None
            out = _embed(t, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
            want = F.want(x["stored"], tok, reduce, mode, _f32(wte_t) if with_wte else None, _f32(wpe_t), p)
            _same(out, want, dt, (fmt, d, mode, name, reduce, positions, str(dt), "wte" if with_wte else "no wte"))
    assert t.status() == 0


@pytest.mark.parametrize("fmt,d", ALL)
def test_workgroup_walks_three_sequences(fmt, d):
    """8200 sequences: a workgroup of k_embed_wave_any walks 3 of them (the last one 1), explicit positions that differ between
    them, half-precision output.  (d = 4100: the lane-group kernel has no walk; its flattened indices reach 16400 * 4100.)"""
    B, T = F.walk_shape(d)
    if d % 8 == 0:
        g = W._assert_regime("k_embed_wave_any", F.GEOM.get(fmt, fmt), d, B, T)[0]
        assert g.seqs_per_block == 3 and g.last_run == 1
    x = F.tables(fmt, d)
    tok, pos = F.walk(T)
    dt = _half(fmt, d)
    wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
    t = _handle(fmt, d)
    out = _embed(t, tok, dt, wte=wte_t, wpe=wpe_t, position_ids=torch.from_numpy(pos))
    want = F.want(x["stored"], tok, "mean", "cover", _f32(wte_t), _f32(wpe_t), pos)
    g, w = W._bits(out), W._bits(W._to(want, dt))
    assert E.same_bits(g, w), (fmt, d, W._differing(g, w, B, T))
    assert t.status() == 0


# ------------------------------------------------------------------ packed batches, a dense base, chosen positions
def _refused(call, t):
    """fp32 d = 4100: scone_embed_varlen and scone_embed_select document that they refuse d % 8 != 0 (include/scone_hip.h: the
    lane-group fallback reads another record form) -- the road cannot run at this width; the refusal is what is checked."""
    from scone_amd.hip_backend import SconeInvalidArgument
    with pytest.raises(SconeInvalidArgument, match="d % 8 == 0"):
        call()
    assert t.status() == 0


@pytest.mark.parametrize("fmt,d", ALL)
def test_embed_varlen(fmt, d):
    x = F.tables(fmt, d)
    t = _handle(fmt, d)
    if d % 8:
        _refused(lambda: t.embed_varlen(torch.from_numpy(F.packed("7x5")[0]), F.packed("7x5")[1]), t)
        return
    for name, dt in (("9x37", torch.float32), ("7x5", _half(fmt, d))):
        flat, cu, seqs = F.packed(name)
        wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
        out = torch.full((flat.size, d), NAN, dtype=dt, device="cuda")
        t.embed_varlen(torch.from_numpy(flat), cu, wte=wte_t, wpe=wpe_t, out=out)
        want = F.want_packed(x["stored"], seqs, wte32=_f32(wte_t), wpe32=_f32(wpe_t))
        _same(out, want, dt, (fmt, d, name, "packed", str(dt)))
    assert t.status() == 0


@pytest.mark.parametrize("fmt,d", ALL)
def test_embed_base(fmt, d):
    """A dense base in the place of wte[tok]: into a fresh buffer (fp32, explicit positions, sum) and in place (half)."""
    x = F.tables(fmt, d)
    t = _handle(fmt, d)
    rng = np.random.default_rng(3 * d)
    tok, pos = F.rect("7x5")
    B, T = tok.shape
    base = _dev(rng.standard_normal((B, T, d)).astype(np.float32), torch.float32)
    wpe_t = _dev(x["wpe"], torch.float32)
    out = torch.full((B, T, d), NAN, dtype=torch.float32, device="cuda")
    t.embed_base(torch.from_numpy(tok), base, wpe=wpe_t, position_ids=torch.from_numpy(pos), reduce="sum", out=out)
    _same(out, F.want(x["stored"], tok, "sum", wpe32=_f32(wpe_t), pos=pos, base32=_f32(base)), torch.float32, (fmt, d, "base"))
    dt = _half(fmt, d)
    tok, _ = F.rect("9x37")
    B, T = tok.shape
    buf = _dev(rng.standard_normal((B, T, d)).astype(np.float32), dt)
    base32 = _f32(buf)
    wpe_t = _dev(x["wpe"], dt)
    got = t.embed_base(torch.from_numpy(tok), buf, wpe=wpe_t, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    _same(buf, F.want(x["stored"], tok, "mean", wpe32=_f32(wpe_t), base32=base32), dt, (fmt, d, "base, in place", str(dt)))
    assert t.status() == 0


@pytest.mark.parametrize("fmt,d", ALL)
def test_embed_select(fmt, d):
    """Unsorted selections with repeats: rectangular (explicit positions per selected row, fp32) and packed (half)."""
    x = F.tables(fmt, d)
    t = _handle(fmt, d)
    rng = np.random.default_rng(5 * d)
    tok, pos = F.rect("9x37")
    total = tok.size
    sel = rng.integers(0, total, size=41)
    sel[7], sel[8], sel[40] = sel[3], total - 1, 0
    assert len(np.unique(sel)) < len(sel) and (np.diff(sel) < 0).any()
    if d % 8:
        _refused(lambda: t.embed_select(torch.from_numpy(tok), sel), t)
        return
    wte_t, wpe_t = _dev(x["wte"], torch.float32), _dev(x["wpe"], torch.float32)
    out = torch.full((len(sel), d), NAN, dtype=torch.float32, device="cuda")
    t.embed_select(torch.from_numpy(tok), sel, wte=wte_t, wpe=wpe_t, position_ids=torch.from_numpy(pos.reshape(-1)[sel]), out=out)
    want = F.want(x["stored"], tok, "mean", "cover", _f32(wte_t), _f32(wpe_t), pos).reshape(total, d)[sel]
    _same(out, want, torch.float32, (fmt, d, "select"))
    dt = _half(fmt, d)
    flat, cu, seqs = F.packed("7x5")
    sel = rng.integers(0, flat.size, size=23)
    sel[5], sel[22] = sel[2], flat.size - 1
    assert len(np.unique(sel)) < len(sel) and (np.diff(sel) < 0).any()
    wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
    out = torch.full((len(sel), d), NAN, dtype=dt, device="cuda")
    t.embed_select(torch.from_numpy(flat), sel, cu_seqlens=cu, wte=wte_t, wpe=wpe_t, reduce="sum", out=out)
    want = F.want_packed(x["stored"], seqs, reduce="sum", wte32=_f32(wte_t), wpe32=_f32(wpe_t))[sel]
    _same(out, want, dt, (fmt, d, "select, packed", str(dt)))
    assert t.status() == 0


# ------------------------------------------------------------------ caller-supplied lists
@pytest.mark.parametrize("fmt,d", ALL)
def test_gather_reduce(fmt, d):
    """Lists of 0, 1, 10, 11 and 40 ids (above 10 the ordered loop, one row at a time), with and without a dense base, on the
    whole table and on a handle that owns rows [20, 60): the sum runs over the owned ids, the mean divides by all of them."""
    x = F.tables(fmt, d)
    n = F.n_rows()
    rng = np.random.default_rng(7 * d)
    ks = [0, 1, 10, 11, 40, 6, 0, 40, 3]
    off = np.zeros(len(ks) + 1, dtype=np.int64)
    np.cumsum(ks, out=off[1:])
    ids = rng.integers(0, n, size=int(off[-1])).astype(np.int64)
    ids[off[4]:off[4] + 3] = ids[off[4]]                              # a repeated id
    base = rng.standard_normal((len(ks), d)).astype(np.float32)
    kf = np.asarray(ks, dtype=np.float32)[:, None]
    for lo, hi in ((0, n), (20, n)):
        t = _handle(fmt, d, lo, hi)
        sums, kown = W._own_sums(x["stored"], off, ids, lo, hi)
        assert lo == 0 or ((kown < np.asarray(ks)).any() and (kown > 0).any())
        mean = np.where(kf > 1, sums / np.maximum(kf, np.float32(1)), sums).astype(np.float32)
        for reduce, fg in (("sum", sums), ("mean", mean)):
            for dt in (torch.float32, _half(fmt, d)):
                out = t.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, out_dtype=dt)
                _same(out, fg, dt, (fmt, d, lo, reduce, str(dt), "lists"))
                b = W._to(base, dt)
                out = t.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, base=b, out_dtype=dt)
                _same(out, b.float().numpy() + fg, dt, (fmt, d, lo, reduce, str(dt), "lists + base"))
        assert t.status() == 0


# ------------------------------------------------------------------ two row shards
@pytest.mark.parametrize("fmt,d", ALL)
def test_partial_sums_of_two_row_shards_and_finalize(fmt, d):
    x = F.tables(fmt, d)
    n = F.n_rows()
    tok, pos = F.rect("9x37")
    B, T = tok.shape
    keys, lens = F.vocabulary()
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, F.MAX_N))
    kfull = np.diff(off)
    parts, want_total, handles = [], np.zeros((B * T, d), dtype=np.float32), []
    for lo, hi in ((0, 20), (20, n)):
        t = _handle(fmt, d, lo, hi)
        want, kown = W._own_sums(x["stored"], off, ids, lo, hi)
        assert (kown < kfull).any() and (kown > 0).any()
        sums = torch.full((B * T, d), NAN, dtype=torch.float32, device="cuda")
        counts = torch.full((B * T,), W.SENTINEL, dtype=torch.int32, device="cuda")
        t.embed_partial(torch.from_numpy(tok), out=(sums, counts))
        assert np.array_equal(counts.cpu().numpy(), kfull), (fmt, d, lo, "counts")
        g = sums.cpu().numpy()
        assert E.same_bits(g, want), (fmt, d, lo, "partial sums", E.first_difference(g, want))
        assert t.status() == 0
        parts.append(sums)
        handles.append(t)
        want_total = want_total + want                                 # what the reduce-scatter computes, shard order
    total = parts[0] + parts[1]
    kf = kfull.astype(np.float32)[:, None]
    mean = np.where(kf > 1, want_total / np.maximum(kf, np.float32(1)), want_total).astype(np.float32).reshape(B, T, d)
    counts = torch.from_numpy(kfull.astype(np.int32)).cuda()
    half = (B * T) // 2 + 1
    for dt in (torch.float32, _half(fmt, d)):
        wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
        want = R.combine(torch.from_numpy(tok), torch.from_numpy(mean), wte_t.float().cpu(), wpe_t.float().cpu(),
                         position_ids=torch.from_numpy(pos)).numpy()
        out = torch.full((B * T, d), NAN, dtype=dt, device="cuda")
        for a, b in ((0, half), (half, B * T)):
            handles[-1].finalize(total[a:b], counts[a:b], torch.from_numpy(tok), a, b, wte=wte_t, wpe=wpe_t,
                                 position_ids=torch.from_numpy(pos), out_dtype=dt, out=out[a:b])
        _same(out, want.reshape(B * T, d), dt, (fmt, d, "finalize", str(dt)))
    assert handles[-1].status() == 0


# ------------------------------------------------------------------ rows in pinned host memory
@pytest.mark.parametrize("fmt,d", SCALED)
def test_pinned_host_read_in_place(fmt, d):
    x = F.tables(fmt, d)
    t = _handle(fmt, d, placement="pinned_host", hot_rows=F.HOT_ROWS)
    _holds(t, x["payload"], x["scales"], what="pinned host")
    tok, pos = F.rect("9x37")
    for dt, p in ((torch.float32, None), (_half(fmt, d), pos)):
        wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
        out = _embed(t, tok, dt, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
        torch.cuda.synchronize()
        _same(out, F.want(x["stored"], tok, "mean", "cover", _f32(wte_t), _f32(wpe_t), p), dt, (fmt, d, "in place", str(dt)))
    assert t.status() == 0


@pytest.mark.parametrize("fmt,d", SCALED)
def test_pinned_host_staged_through_the_cache(fmt, d):
    """Chunks of 4, 4 and 1 sequences.  The cache keeps its OWN copy of a cold row's scales beside the row (k_stage_copy): all
    of them, 160 / 256 bytes here, not the first 128.  The whole cold table fits the cache, so the first pass copies each
    referenced cold row once and the second pass none."""
    x = F.tables(fmt, d)
    t = _handle(fmt, d, placement="pinned_host", hot_rows=F.HOT_ROWS, stage_tokens=F.STAGE_TOKENS)
    tok, pos = F.rect("9x37")
    B, T = tok.shape
    keys, lens = F.vocabulary()
    cold = F.referenced(keys, lens, tok, F.MAX_N, F.HOT_ROWS)
    for k, (dt, p) in enumerate(((torch.float32, None), (_half(fmt, d), pos))):
        wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
        out = _embed(t, tok, dt, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
        torch.cuda.synchronize()
        c = t.stage_counters()
        print(f"{fmt}-d{d} pass {k}: {c}")
        _same(out, F.want(x["stored"], tok, "mean", "cover", _f32(wte_t), _f32(wpe_t), p), dt, (fmt, d, "staged", f"pass {k}", str(dt)))
        assert c["cache_rows"] == F.n_rows() - F.HOT_ROWS and c["chunk_tokens"] == 4 * T and c["chunks"] == 3 * (k + 1)
        assert c["rows_copied"] == len(cold), (k, c, len(cold))             # pass 1 copies nothing
    assert t.status() == 0


# ------------------------------------------------------------------ the exchange between row shards
@pytest.mark.parametrize("head", [0, 5])
@pytest.mark.parametrize("fmt,d", SCALED)
def test_row_exchange_between_three_shards_on_one_gpu(fmt, d, head):
    """Records [payload | scales | row id], received in a permuted order, and columns (payload rows | scales | hash fragments)."""
    from scone_amd.distributed import shard_range
    from scone_amd.hip_backend import SconeTable
    x = F.tables(fmt, d)
    n, world = F.n_rows(), 3
    tok_np, _ = F.rect("9x37")
    B, T = tok_np.shape
    tok = torch.from_numpy(tok_np)
    dt = _half(fmt, d)
    wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
    want = F.want(x["stored"], tok_np, "mean", "cover", _f32(wte_t), _f32(wpe_t)).reshape(B * T, d)
    shards = []
    for r in range(world):
        a, b = shard_range(n, r, world)
        s = _handle(fmt, d, a, b)
        if head:
            s.shard_set_head(head)
            s.shard_head_store_f32(torch.from_numpy(x["table"][:head]), row0=0)
        shards.append(s)
    pb, sb = F.payload_bytes(fmt, d), F.scale_bytes(fmt, d)
    assert (shards[0].payload_bytes(), shards[0].scale_bytes()) == (pb, sb)
    assert shards[0].shard_record_bytes() >= pb + sb + 8
    cnts = [s.shard_gather_plan(tok) for s in shards]
    assert sum(cnts) > 0 and all(c > 0 for c in cnts)
    sends = [s.shard_gather_pack(c) for s, c in zip(shards, cnts)]
    recv = torch.cat([sends[r] for r in (2, 0, 1)]).contiguous()
    got = torch.full((B * T, d), NAN, dtype=dt, device="cuda")
    shards[1].shard_gather_embed(tok, recv, wte=wte_t, wpe=wpe_t, out_dtype=dt, out=got)
    _same(got, want, dt, (fmt, d, "records", head))
    cnts = [s.shard_gather_plan(tok) for s in shards]
    slots = [SconeTable.cols_frag_slots(c) for c in cnts]
    rb, fo = [sum(cnts[:r]) for r in range(world)], [sum(slots[:r]) for r in range(world)]
    tot = sum(cnts)
    c_rows = torch.empty((tot, pb), dtype=torch.uint8, device="cuda")
    c_sc = torch.full((head + tot, sb), 0xA5, dtype=torch.uint8, device="cuda") if sb else None
    c_fr = torch.empty(sum(slots), dtype=torch.int64, device="cuda")
    for r, s in enumerate(shards):
        s.shard_cols_pack(0, cnts[r], c_rows[rb[r]:rb[r] + cnts[r]], None if c_sc is None else c_sc[head + rb[r]:head + rb[r] + cnts[r]],
                          c_fr[fo[r]:fo[r] + slots[r]])
    if head and c_sc is not None:
        shards[2].shard_head_scales_into(c_sc)
    got = torch.full((B * T, d), NAN, dtype=dt, device="cuda")
    shards[2].shard_cols_embed(tok, 0, B, c_rows, tot, c_sc, c_fr, fo, slots, rb, got, wte=wte_t, wpe=wpe_t)
    _same(got, want, dt, (fmt, d, "columns", head))
    assert all(s.status() == 0 for s in shards)


# ------------------------------------------------------------------ eviction where the cached rows carry scales
@pytest.mark.parametrize("fmt,d", F.EVICT_CASES)
def test_eviction_of_cached_rows_with_scales(fmt, d):
    """24 unigrams in HBM, 576 bigrams in pinned host memory behind 84 cache slots, 400 chunks of one 2-token sequence: slots
    change hands inside a pass, and a slot's scales must change hands with its row."""
    from scone_amd.hip_backend import SconeTable
    x = F.evict_inputs(fmt, d)
    keys, lens = F.evict_vocabulary()
    vocab = (keys, lens, F.EVICT_MAX_N)
    n = len(lens)
    t = SconeTable(F.EVICT_MAX_N, n, d, fmt, placement="pinned_host", hot_rows=F.EVICT_TOKENS, stage_tokens=F.EVICT_STAGE_TOKENS)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(x["table"]))
    _holds(t, x["payload"], x["scales"], what="pinned host")
    tok = x["tok"]
    cold = F.referenced(keys, lens, tok, F.EVICT_MAX_N, F.EVICT_TOKENS)
    assert len(cold) > F.EVICT_SLOTS
    copied = 0
    for k, dt in enumerate((torch.float32, torch.bfloat16)):
        wte_t, wpe_t = _dev(x["wte"], dt), _dev(x["wpe"], dt)
        out = _embed(t, tok, dt, wte=wte_t, wpe=wpe_t)
        torch.cuda.synchronize()
        c = t.stage_counters()
        print(f"{fmt}-d{d} pass {k}: {c}, {len(cold)} distinct cold rows referenced")
        _same(out, F.want(x["stored"], tok, "mean", "cover", _f32(wte_t), _f32(wpe_t), vocab=vocab), dt, (fmt, d, "eviction", f"pass {k}"))
        assert c["cache_rows"] == F.EVICT_SLOTS == 84 and c["chunks"] == 400 * (k + 1)
        if k == 0:
            assert c["rows_copied"] >= len(cold)
        else:
            assert c["rows_copied"] > copied                             # the second pass misses again
        copied = c["rows_copied"]
    assert t.status() == 0


# ------------------------------------------------------------------ every format through each of the four row-decoding bodies
# The narrow end, in the file that has the helpers: (format, d) x the body that decodes the rows there.
#   d = 768 (two segments, the second of 256 elements), 1024 (INT4 / MXFP4: the packed scale pair), 1280 (three segments):
#       embed_token under k_embed_wave (hit lists) and under k_embed_csr_wave (caller's lists up to 10 owned ids),
#       embed_token_long (caller's lists of 11 and 23 ids)
#   d = 520 (65 units: lane 0 walks two), int8 528 (d % 16 == 0), INT4 / MXFP4 640 (d % 128 == 0): embed_units under k_embed_wave_any, and the
#       lane-group k_embed for the caller's lists.  INT4 / MXFP4 take these two at 768 and 1280 as well (a trailing segment of
#       256 elements would be 2 row bytes per lane: wave_geom<>::OK is false), which is three more widths for the one kernel
#       whose INT4 decode is shared with the wave bodies, k_embed
# Lists of 0, 1, 6 (all candidates at max_n = 3), 10 (at max_n = 4), 11 and 23 ids, mean and sum, 64 tokens at the most.
NARROW_FMTS = ("fp32", "fp16", "bf16", "int8", "int4", "mxfp4")
NARROW_UNITS = {"int8": 528, "int4": 640, "mxfp4": 640}          # the smallest width of more than 64 units scone_create accepts; else 520
NARROW = [pytest.param(f, d, id=f"{f}-d{d}") for f in NARROW_FMTS for d in (768, 1024, 1280, NARROW_UNITS.get(f, 520))]
NARROW_MAX_N = 4
NARROW_KS = (0, 1, 6, 10, 11, 23, 3, 0)


def _narrow_tables(fmt, d):
    rng = np.random.default_rng(13 * d + NARROW_FMTS.index(fmt))
    n = W.N_ROWS[NARROW_MAX_N]
    table = (rng.standard_normal((n, d)) * F._magnitudes(rng, n, d)).astype(np.float32)
    wte = rng.standard_normal((F.VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((F.N_POS, d)).astype(np.float32)
    return table, F.quantise(fmt, table)[2], wte, wpe


def _narrow_batch(max_n):
    """tok [4, 16]: the first seed at which the list lengths 0, 1 and max_n (max_n + 1) / 2 all occur."""
    keys, lens = W._vocabulary(max_n)
    full = max_n * (max_n + 1) // 2
    for seed in range(9000, 9400):
        tok = np.random.default_rng(seed).choice(F.VOCAB + 1, size=(4, 16), p=W.TOKEN_P).astype(np.int64)
        hist = np.bincount(F.list_lengths(keys, lens, tok, max_n), minlength=full + 1)
        if hist[0] and hist[1] and hist[full]:
            return keys, lens, tok
    raise AssertionError(f"no seed gives the list lengths 0, 1 and {full}")


@pytest.mark.parametrize("fmt,d", NARROW)
def test_every_format_through_every_row_decoding_body(fmt, d):
    from scone_amd.hip_backend import SconeTable
    table, stored, wte, wpe = _narrow_tables(fmt, d)
    n = len(table)
    token_body = d in (768, 1024, 1280) and not (fmt in ("int4", "mxfp4") and d != 1024)
    assert F.kernel_family(fmt, d) == ("k_embed_wave" if token_body else "k_embed_wave_any")
    # hit lists, two kernels: embed_token / embed_units
    for max_n in (3, NARROW_MAX_N):
        keys, lens, tok = _narrow_batch(max_n)
        m = len(lens)
        t = SconeTable(max_n, m, d, fmt)
        t.index_build(keys, lens)
        t.store_f32(torch.from_numpy(table[:m]))
        wte_t, wpe_t = _dev(wte, torch.float32), _dev(wpe, torch.float32)
        for reduce in ("mean", "sum"):
            out = _embed(t, tok, torch.float32, reduce=reduce, wte=wte_t, wpe=wpe_t)
            want = F.want(stored[:m], tok, reduce, "cover", wte, wpe, vocab=(keys, lens, max_n))
            _same(out, want, torch.float32, (fmt, d, max_n, reduce, "hit lists"))
        assert t.status() == 0
    # the caller's lists: embed_token and embed_token_long under k_embed_csr_wave / the lane-group k_embed
    keys, lens = W._vocabulary(NARROW_MAX_N)
    rng = np.random.default_rng(17 * d)
    off = np.zeros(len(NARROW_KS) + 1, dtype=np.int64)
    np.cumsum(NARROW_KS, out=off[1:])
    ids = rng.integers(0, n, size=int(off[-1])).astype(np.int64)
    base = rng.standard_normal((len(NARROW_KS), d)).astype(np.float32)
    kf = np.asarray(NARROW_KS, dtype=np.float32)[:, None]
    for lo in (0, 20):
        t = SconeTable(NARROW_MAX_N, n, d, fmt, row_begin=lo, row_end=n)
        t.index_build(keys, lens)
        t.store_f32(torch.from_numpy(table[lo:]), row0=lo)
        sums, kown = W._own_sums(stored, off, ids, lo, n)
        assert lo == 0 or ((kown < np.asarray(NARROW_KS)).any() and kown.max() > 10)
        mean = np.where(kf > 1, sums / np.maximum(kf, np.float32(1)), sums).astype(np.float32)
        for reduce, fg in (("sum", sums), ("mean", mean)):
            out = t.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, out_dtype=torch.float32)
            _same(out, fg, torch.float32, (fmt, d, lo, reduce, "lists"))
            out = t.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, base=torch.from_numpy(base), out_dtype=torch.float32)
            _same(out, base + fg, torch.float32, (fmt, d, lo, reduce, "lists + base"))
        assert t.status() == 0
