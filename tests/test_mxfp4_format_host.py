"""The MXFP4 table format (SCONE_FMT_MXFP4 = 5: E2M1 elements, one E8M0 scale per 32) as far as it can be checked WITHOUT a GPU:

* known answers of the quantiser written out by hand, and the two host statements of it (tests/mxfp4_fixture.py: value
  arithmetic with frexp / ldexp, integer work on the fp32 bit patterns) agreeing on every edge and on a million bit patterns;
* all 16 x 256 (code, scale byte) pairs dequantised against float64: every finite product is exact;
* idempotence of the quantiser and the error bound |v - dq(v)| <= amax / 4.  The bound is derived, not measured: with
  s = 2^(X-127) and amax / s in [4, 8), the grid steps are 0.5 s below 2 s, s below 4 s and 2 s up to 6 s, so an element is at
  most s away -- and amax >= 4 s; above 6 s it saturates, at most 2 s < amax / 4 away.  It needs the scale the rule asks for: a
  block whose amax is below 2^-125 has X clamped to 0 and elements below 4 * 2^-127, where the widest step is 2^-127: an
  element is at most 2^-128 away;
* the Python surface: names, row / payload / scale sizes, the C enum value, the v2 native file's header through a host stand-in;
* hipcc cross-compiles the MXFP4 gather unit and its INT4 twin to gfx950 assembly: no k_embed_wave instantiation of the new unit
  spills, `<MXFP4, __half, 1024, 3, FIXED_POS, !PARTIAL, HIOCC>` exists and gets no fewer waves per SIMD than `<I4, ...>`
  compiled from the same tree."""

import json
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_fixture as MX  # noqa: E402
import edge_fixture as E  # noqa: E402

from scone_amd.hip_backend import SconeTable as _DeviceTable, format_code  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scone_amd", "csrc")
FLT_MAX = float(np.finfo(np.float32).max)


def _block(values, fill=0.0):
    """One row of 128: the values at the front of block 0, `fill` behind them and in the other three blocks."""
    r = np.full((1, 128), fill, dtype=np.float32)
    r[0, :len(values)] = np.asarray(values, dtype=np.float32)
    return r


def _both(x):
    a, b = MX.quantize(x), MX.quantize_bits(x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (np.argwhere(a[0] != b[0])[:5].tolist(), np.argwhere(a[1] != b[1])[:5].tolist())
    return MX.unpack(a[0]), a[1]


# ------------------------------------------------------------------ the quantiser, stated twice
def test_known_answers_of_the_quantiser():
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(99)))        # noqa: E731
    dn = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))         # noqa: E731
    # amax = 6 -> X = 127, scale 1: the element grid itself.  (value, code)
    cases = [(6.0, 7)]
    for mid, lo, hi, tie in ((0.25, 0, 1, 0), (0.75, 1, 2, 2), (1.25, 2, 3, 2), (1.75, 3, 4, 4), (2.5, 4, 5, 4), (3.5, 5, 6, 6), (5.0, 6, 7, 6)):
        cases += [(dn(mid), lo), (mid, tie), (up(mid), hi)]
    cases += [(0.0, 0), (0.5, 1), (1.0, 2), (1.5, 3), (2.0, 4), (3.0, 5), (4.0, 6)]
    pos = [c[0] for c in cases]
    codes, X = _both(_block(pos + [-v for v in pos]))
    n = len(cases)
    assert X[0, 0] == 127
    assert codes[0, :n].tolist() == [c[1] for c in cases]
    assert codes[0, n:2 * n].tolist() == [c[1] | 8 for c in cases]          # the sign is kept, -0.0 included (0x8)
    # saturation: amax in [6, 8) keeps X = 127
    codes, X = _both(_block([6.0, 6.0000005, 7.99, -6.0000005, -7.99]))
    assert X[0, 0] == 127 and codes[0, :5].tolist() == [7, 7, 7, 15, 15]
    # a block maximum exactly a power of two, and one ulp below it
    codes, X = _both(_block([4.0, 1.0]))
    assert X[0, 0] == 127 and codes[0, :2].tolist() == [6, 2]
    codes, X = _both(_block([dn(4.0), 1.0]))
    assert X[0, 0] == 126 and codes[0, :2].tolist() == [7, 4]               # 3.99.. / 0.5 = 7.99.. -> 6; 1 / 0.5 = 2
    codes, X = _both(_block([2.0 ** -20, -2.0 ** -22]))
    assert X[0, 0] == 127 - 22 and codes[0, :2].tolist() == [6, 8 | 2]
    # an all-zero block and a -0 block: X = 127, only the signs
    codes, X = _both(np.concatenate([_block([]), _block([], fill=-0.0)]))
    assert X.tolist() == [[127] * 4] * 2 and (codes[0] == 0).all() and (codes[1] == 8).all()
    # NaN / inf blocks: X = 255 for that block alone, nibbles = the signs
    r = _block([1.0, -2.0, np.nan]); r[0, 33] = np.inf; r[0, 64] = -np.inf; r[0, 65] = -1.0; r[0, 96] = 3.0
    codes, X = _both(r)
    assert X[0].tolist() == [255, 255, 255, 126]                            # the finite block: amax 3 -> floor(log2) 1 -> 126
    assert codes[0, :3].tolist()[:2] == [0, 8] and codes[0, 64:66].tolist() == [8, 8] and codes[0, 96] == 7      # 3 / 0.5 = 6
    assert np.isnan(MX.dequantize(*MX.quantize(r))[0, :96]).all()
    # a subnormal amax is clamped to X = 0 (scale 2^-127); FLT_MAX gives X = 252
    codes, X = _both(_block([2.0 ** -127, 2.0 ** -128, 2.0 ** -129, 2.0 ** -130, 3 * 2.0 ** -129, -2.0 ** -149]))
    assert X[0, 0] == 0 and codes[0, :6].tolist() == [2, 1, 0, 0, 2, 8]       # 1, 0.5, the tie 0.25 -> 0, 0.125 -> 0, the tie 0.75 -> 1.0
    codes, X = _both(_block([2.0 ** -124, 2.0 ** -125]))
    assert X[0, 0] == 1 and codes[0, :2].tolist() == [6, 4]
    codes, X = _both(_block([FLT_MAX, -FLT_MAX, 2.0 ** 127, 2.0 ** 125]))
    assert X[0, 0] == 252 and codes[0, :4].tolist() == [7, 15, 6, 2]
    assert MX.dequantize(*MX.quantize(_block([FLT_MAX])))[0, 0] == np.float32(6 * 2.0 ** 125)


def test_the_two_statements_agree_on_every_edge():
    _both(MX.edge_rows())
    _both(np.resize(E.E_CONSTANTS, 128).reshape(1, 128))
    for max_n in (3, 4):
        n = len(E.vocabulary(max_n)[1])
        _both(E.table(n, 128, seed=max_n))
        _both(E.table(n, 768, seed=40 + max_n))
    for w in E.wte_wpe(3, 64, 128):
        _both(w)


def test_the_two_statements_agree_on_a_million_bit_patterns():
    rng = np.random.default_rng(20265)
    x = rng.integers(0, 2 ** 32, size=(1_000_000 // 128 + 1, 128), dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.isnan(x).sum() > 1000 and (np.abs(x[np.isfinite(x)]) < 1.1754944e-38).sum() > 1000
    _both(x)
    # random bit patterns rarely share a block with values of their own size: blocks of one binade, at every exponent
    y = (rng.standard_normal((4096, 128)) * np.exp2(rng.integers(-149, 125, size=(4096, 4)).repeat(32, axis=1))).astype(np.float32)
    codes, X = _both(y)
    assert len(np.unique(X)) > 200 and all((codes & 7 == c).any() for c in range(8))


def test_all_4096_dequantised_values_are_the_exact_products():
    codes = np.tile(np.arange(16, dtype=np.uint8), 8)[None, :].repeat(256, axis=0)            # [256, 128]: the 16 codes cycling
    scales = np.arange(256, dtype=np.uint8)[:, None].repeat(4, axis=1)
    got = MX.dequantize(MX.pack(codes), scales)
    sign = np.where(codes & 8, -1.0, 1.0)
    exact = sign * MX.MAGNITUDES[codes & 7] * np.exp2(np.arange(256, dtype=np.float64) - 127)[:, None]
    assert np.isnan(got[255]).all() and not np.isnan(got[:255]).any()
    fin = np.isfinite(got[:255])
    assert np.array_equal(got[:255][fin].astype(np.float64), exact[:255][fin]), "a finite product is exact"
    assert np.array_equal(np.signbit(got[:255]), codes[:255] >= 8)                             # -0 stays -0
    # the only inexact ones: large codes at X >= 253 overflow to +-inf
    rows, cols = np.nonzero(~fin)
    assert rows.min() == 253 and set((codes[0, cols] & 7).tolist()) == {4, 5, 6, 7}      # 2 * 2^127 at X = 254, and 3, 4, 6
    assert (np.abs(exact[:255][~fin]) > FLT_MAX).all()
    assert got[0, 1] == np.float32(2.0 ** -128) and got[0, 2] == np.float32(2.0 ** -127)      # X = 0: the subnormal factor


def test_idempotence_and_the_error_bound():
    rng = np.random.default_rng(7)
    y = (rng.standard_normal((4096, 128)) * np.exp2(rng.integers(-149, 125, size=(4096, 4)).repeat(32, axis=1))).astype(np.float32)
    x = np.concatenate([MX.edge_rows(), y])
    p, X = MX.quantize(x)
    s = MX.dequantize(p, X)
    p2, X2 = MX.quantize(s)
    assert E.same_bits(MX.dequantize(p2, X2), s), "a stored row is a fixed point"
    zero = (s.reshape(len(s), -1, 32) == 0).all(axis=2)                    # (a block that rounded to zeros is restated with X = 127)
    assert np.array_equal(X2[~zero], X[~zero])
    num = np.repeat(X != 255, 32, axis=1)                                  # (a NaN block's nibbles are the signs of what it was given)
    assert np.array_equal(MX.unpack(p2)[num], MX.unpack(p)[num])
    b = x.reshape(len(x), -1, 32).astype(np.float64)
    live = X != 255
    amax = np.abs(b).max(axis=2)
    err = np.abs(b - s.reshape(b.shape).astype(np.float64)).max(axis=2)
    ruled = live & (amax >= 2.0 ** -125)                                    # X is what the rule asks for, not the clamp
    assert ruled.sum() > 10000 and (err[ruled] <= amax[ruled] / 4).all(), (err[ruled] / amax[ruled]).max()
    assert (err[ruled] / amax[ruled]).max() > 0.24
    clamped = live & ~ruled
    assert clamped.sum() > 100 and (X[clamped & (amax > 0)] == 0).all() and (err[clamped] <= 2.0 ** -128).all()


# ------------------------------------------------------------------ the Python surface
def test_format_names_and_sizes():
    from scone_amd import _lib as L
    from scone_amd.hip_backend import SconeTable, row_bytes
    assert L.FMT_MXFP4 == 5 and (L.FMT_F32, L.FMT_F16, L.FMT_I8, L.FMT_I4, L.FMT_BF16) == (0, 1, 2, 3, 4)
    assert format_code("mxfp4") == format_code("MXFP4") == L.FMT_MXFP4 == format_code(5)
    assert format_code("int4") == L.FMT_I4 and format_code("bf16") == L.FMT_BF16
    for bad in ("bf8", "mxfp8", "mxfp6", "nvfp4", "fp4"):
        with pytest.raises(ValueError, match="unknown table format"):
            format_code(bad)
    assert row_bytes(L.FMT_MXFP4, 1024) == 544 and row_bytes(L.FMT_I4, 1024) == 528
    for d in (128, 768, 1024, 1280, 4096):
        assert row_bytes(L.FMT_MXFP4, d) == d // 2 + d // 32
        h = types.SimpleNamespace(fmt=L.FMT_MXFP4, dim=d)
        h.scales_per_row = lambda h=h: SconeTable.scales_per_row(h)
        h.scales_dtype = lambda h=h: SconeTable.scales_dtype(h)
        assert SconeTable.payload_bytes(h) == d // 2 and SconeTable.scales_per_row(h) == d // 32 == SconeTable.scale_bytes(h)
        assert SconeTable.scales_dtype(h) == np.uint8
        h4 = types.SimpleNamespace(fmt=L.FMT_I4, dim=d)
        h4.scales_per_row = lambda h=h4: SconeTable.scales_per_row(h)
        h4.scales_dtype = lambda h=h4: SconeTable.scales_dtype(h)
        assert SconeTable.scale_bytes(h4) == 2 * (d // 128) and SconeTable.scales_dtype(h4) == np.float16
    header = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    assert re.search(r"\bSCONE_FMT_MXFP4\s*=\s*5\b", header) and re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", header)
    assert re.search(r"\bSCONE_FMT_BF16\s*=\s*4\b", header) and L.ABI_VERSION == 2


class _HostTable:
    """Stand-in for hip_backend.SconeTable in save_native / load_native: holds raw rows and scale bytes on the host."""
    made = []

    def __init__(self, max_n, n_rows, dim=0, table_format="fp32", row_begin=0, row_end=None, **kw):
        self.max_n, self.n_rows, self.dim, self.table_format = max_n, n_rows, dim, table_format
        self.fmt = format_code(table_format)
        self.row_begin, self.row_end = row_begin, n_rows if row_end is None else row_end
        self.rows = np.zeros((self.row_end - self.row_begin, self.payload_bytes()), dtype=np.uint8)
        self.scales = np.zeros((self.row_end - self.row_begin, self.scales_per_row()), dtype=self.scales_dtype())
        self.keys = None
        _HostTable.made.append(self)

    payload_bytes = lambda self: _DeviceTable.payload_bytes(self)          # noqa: E731
    scales_per_row = lambda self: _DeviceTable.scales_per_row(self)        # noqa: E731
    scales_dtype = lambda self: _DeviceTable.scales_dtype(self)            # noqa: E731

    def index_build(self, keys, lens, id0=0):
        self.keys = (np.array(keys), np.array(lens))

    def upload(self, rows, scales=None, row0=0):
        assert scales is not None and scales.dtype == np.uint8 and rows.dtype == np.uint8
        a = row0 - self.row_begin
        self.rows[a:a + rows.shape[0]], self.scales[a:a + rows.shape[0]] = rows, scales

    def download(self, row0, nrows, rows=None, scales=None):
        assert scales.dtype == np.uint8
        a = row0 - self.row_begin
        rows[:], scales[:] = self.rows[a:a + nrows], self.scales[a:a + nrows]
        return rows, scales


def test_native_file_header_round_trip_on_the_host(tmp_path, monkeypatch):
    """save_native writes "mxfp4", a [n, d/2] row section and a uint8 [n, d/32] scale section into the v2 header; load_native hands
    the same bytes to a handle of that format.  The device handle is replaced by a host stand-in: no kernel runs."""
    import scone_amd.hip_backend as HB
    from scone_amd import EmbeddingCache, NGramExtractor
    monkeypatch.setattr(HB, "SconeTable", _HostTable)
    _HostTable.made.clear()
    rng = np.random.default_rng(3)
    n, d, max_n = 200, 128, 3
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, 50, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:12] = MX.edge_rows()
    payload, scales = MX.quantize(x)
    cache = EmbeddingCache(ex, d, table_format="mxfp4", keep_host_copy=False)
    table = _HostTable(max_n, n, dim=d, table_format="mxfp4")
    table.upload(payload, scales)
    cache._table, cache._dirty, cache._present = table, False, np.ones(n, dtype=bool)
    path = str(tmp_path / "t.npy")
    cache.save_native(path, chunk_rows=64)
    mm = np.load(path, mmap_mode="r")
    hlen = int(np.frombuffer(bytes(mm[:8]), dtype=np.uint64)[0])
    meta = json.loads(bytes(mm[8:8 + hlen]).decode())
    assert meta["magic"] == EmbeddingCache.NATIVE_MAGIC_V2 and meta["table_format"] == "mxfp4"
    assert meta["sections"]["rows"] == {"dtype": "uint8", "shape": [n, d // 2]}
    assert meta["sections"]["scales"] == {"dtype": "uint8", "shape": [n, d // 32]}
    del mm
    again = EmbeddingCache.load_native(path, chunk_rows=48)
    loaded = _HostTable.made[-1]
    assert loaded is not table and again.table_format == "mxfp4" and loaded.fmt == 5 and loaded.dim == d
    assert np.array_equal(loaded.rows, payload) and np.array_equal(loaded.scales, scales)
    assert np.array_equal(loaded.keys[0], keys) and np.array_equal(loaded.keys[1], lens)


# ------------------------------------------------------------------ the MXFP4 translation unit against its INT4 twin
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("asm")
    procs = {}
    for unit in ("mxfp4", "i4"):
        cmd = ["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
               f"scone_gather_{unit}.hip", "-o", str(out / f"scone_gather_{unit}.s")]
        procs[unit] = subprocess.Popen(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    text = {}
    for unit, p in procs.items():
        _, err = p.communicate(timeout=1200)
        assert p.returncode == 0, err[-2000:]
        text[unit] = open(out / f"scone_gather_{unit}.s").read()
    return text


def _resources(asm_text):
    """{mangled kernel name: {NumVgprs, ScratchSize, Occupancy}} (as tests/test_kernel_invariants_cpu.py reads them)."""
    labels = [(m.start(), m.group(1)) for m in re.finditer(r"^(_Z\w+):[^\n]*\n; %bb\.0:", asm_text, flags=re.M)]
    out = {}
    for k, (pos, name) in enumerate(labels):
        chunk = asm_text[pos:labels[k + 1][0] if k + 1 < len(labels) else len(asm_text)]
        out[name] = {a: int(b) for a, b in re.findall(r"; (NumVgprs|ScratchSize|Occupancy): (\d+)", chunk)}
    return out


def test_no_wave_kernel_of_the_mxfp4_unit_spills(asm):
    ks = {n: r for n, r in _resources(asm["mxfp4"]).items() if "k_embed_waveI" in n}
    assert len(ks) >= 14 and all("ILi5E" in n for n in ks), len(ks)          # every (out dtype, max_n, variant) of FMT = 5 at d = 1024
    bad = {n[:90]: r for n, r in ks.items() if r.get("ScratchSize", 1) != 0}
    assert not bad, bad
    assert "v_cvt_scalef32_pk_f32_fp4" in asm["mxfp4"] and "v_cvt_scalef32_pk_f32_fp4" not in asm["i4"]


def test_headline_shaped_mxfp4_kernel_gets_no_fewer_waves_than_its_int4_twin(asm):
    tail = "6__halfLi1024ELi3ELb1ELb0ELb1E"                    # <FMT, __half, 1024, 3, FIXED_POS, !PARTIAL, HIOCC>
    mx = [r for n, r in _resources(asm["mxfp4"]).items() if "k_embed_waveILi5E" + tail in n]
    i4 = [r for n, r in _resources(asm["i4"]).items() if "k_embed_waveILi3E" + tail in n]
    assert len(mx) == 1 and len(i4) == 1, (len(mx), len(i4))              # bit 5 of SCONE_HIOCC_MASK: the variant exists
    mx, i4 = mx[0], i4[0]
    print("mxfp4", mx, "int4 twin", i4)
    assert mx["ScratchSize"] == 0
    assert mx["Occupancy"] >= i4["Occupancy"], (mx, i4)
