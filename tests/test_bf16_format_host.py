"""The bfloat16 table format (SCONE_FMT_BF16 = 4) as far as it can be checked WITHOUT a GPU:

* the two host statements of the rounding (tests/bf16_fixture.py: integer arithmetic in numpy, torch's CPU `.bfloat16()`) agree
  on every edge of the fp32 -> bf16 conversion and on a million random bit patterns -- equal NaN positions, everything else bit
  for bit -- and a handful of values are pinned to bit patterns written out by hand;
* the Python surface knows the format: names, row / payload / scale sizes, the C enum value, the v2 native file's header
  (written and read back through a stand-in for the device handle);
* hipcc cross-compiles the bf16 gather translation unit and its fp16 twin to gfx950 assembly: no `k_embed_wave` instantiation
  of the bf16 unit spills, and the instantiation the C2-shaped workload runs, `<BF16, __half, 768, 3, FIXED_POS, !PARTIAL,
  HIOCC>`, needs no more VGPRs and reaches no lower occupancy than `<F16, ...>` compiled from the same tree (the bar is the twin,
  not a number).  The build is the one of tests/test_kernel_invariants_cpu.py; two units, compiled side by side."""

import json
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import edge_fixture as E  # noqa: E402

from scone_amd.hip_backend import SconeTable as _DeviceTable, format_code  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scone_amd", "csrc")


def _bits(values):
    return np.asarray(values, dtype=np.uint32).view(np.float32)


def _agree(x, what):
    a, b = BF.to_bf16_bits(x), BF.torch_bf16_bits(x)
    assert a.dtype == np.uint16 and a.shape == np.shape(x)
    assert BF.same_bf16_bits(a, b), (what, np.argwhere(a != b)[:5].tolist())
    src_nan = np.isnan(np.asarray(x, dtype=np.float32))
    assert np.array_equal(BF.is_nan_bits(a), src_nan), (what, "a NaN became a number or a number a NaN")
    assert ((a[src_nan] & 0x0040) != 0).all(), (what, "NaN must stay a QUIET NaN")


# ------------------------------------------------------------------ the rounding, stated twice
def test_known_answers_of_the_rounding():
    cases = [
        (0x3F808000, 0x3F80), (0x3F818000, 0x3F82),          # ties: to the even upper half
        (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),
        (0x3F808001, 0x3F81), (0x3F807FFF, 0x3F80),          # one ulp beside the tie
        (0x7F7F0000, 0x7F7F), (0x7F7F7FFF, 0x7F7F),          # largest bf16; last value that stays finite
        (0x7F7F8000, 0x7F80), (0x7F7FFFFF, 0x7F80),          # first value that rounds to +inf; FLT_MAX
        (0xFF7F8000, 0xFF80),
        (0x00000001, 0x0000), (0x00008000, 0x0000), (0x00008001, 0x0001), (0x00018000, 0x0002),   # fp32 subnormals
        (0x007FFFFF, 0x0080),                                # the largest subnormal rounds up to FLT_MIN
        (0x80008000, 0x8000), (0x80000000, 0x8000), (0x00000000, 0x0000),    # -0.0 stays -0.0
        (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
    ]
    got = BF.to_bf16_bits(_bits([c[0] for c in cases]))
    assert got.tolist() == [c[1] for c in cases]
    assert BF.torch_bf16_bits(_bits([c[0] for c in cases])).tolist() == [c[1] for c in cases]
    # NaN: never an infinity (0x7F80 / 0xFF80), never a wrapped exponent (0x7FFFFFFF + 0x8000 carries into the sign bit)
    nans = BF.to_bf16_bits(_bits([0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF, 0x7FC00000]))
    assert BF.is_nan_bits(nans).all() and ((nans & 0x0040) != 0).all()
    assert (nans >> 15).tolist() == [0, 0, 1, 0, 0]


def test_the_two_statements_agree_on_every_edge():
    _agree(BF.edge_values(), "edge values")
    _agree(E.E_CONSTANTS, "edge_fixture constants")
    for max_n in (3, 4):
        n = len(E.vocabulary(max_n)[1])
        _agree(E.table(n, 64, seed=max_n), f"edge_fixture.table max_n={max_n}")
        _agree(E.table(n, 768, seed=40 + max_n), f"edge_fixture.table d=768 max_n={max_n}")
    for w in E.wte_wpe(3, 64):
        _agree(w, "edge_fixture.wte_wpe")


def test_the_two_statements_agree_on_a_million_bit_patterns():
    rng = np.random.default_rng(20260)
    x = rng.integers(0, 2 ** 32, size=1_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.isnan(x).sum() > 1000 and (np.abs(x[np.isfinite(x)]) < 1.1754944e-38).sum() > 1000      # NaNs and subnormals occur
    _agree(x, "random bit patterns")


def test_round_trip_and_exactness_of_the_stored_values():
    x = np.concatenate([BF.edge_values(), E.table(20, 64).ravel()])
    b = BF.to_bf16_bits(x)
    back = BF.from_bf16_bits(b)
    assert back.dtype == np.float32
    assert BF.same_bf16_bits(BF.to_bf16_bits(back), b), "a stored value is a fixed point of the rounding"
    t = torch.from_numpy(b.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert E.same_bits(back, t), "bits << 16 is torch's upcast"
    fin = np.isfinite(x) & np.isfinite(back)
    ulp = np.abs(back[fin]) * 2.0 ** -8 + 2.0 ** -133
    assert (np.abs(back[fin].astype(np.float64) - x[fin].astype(np.float64)) <= ulp).all()


# ------------------------------------------------------------------ the Python surface
def test_format_names_and_sizes():
    from scone_amd import _lib as L
    from scone_amd.hip_backend import SconeTable, format_code, row_bytes
    assert L.FMT_BF16 == 4 and (L.FMT_F32, L.FMT_F16, L.FMT_I8, L.FMT_I4) == (0, 1, 2, 3)
    assert format_code("bf16") == format_code("bfloat16") == format_code("BF16") == L.FMT_BF16 == format_code(4)
    assert format_code("fp16") == L.FMT_F16 and format_code("int4") == L.FMT_I4
    with pytest.raises(ValueError, match="unknown table format"):
        format_code("bf8")
    for d in (64, 768, 1024, 1280, 4096):
        assert row_bytes(L.FMT_BF16, d) == 2 * d == row_bytes(L.FMT_F16, d)
        h = types.SimpleNamespace(fmt=L.FMT_BF16, dim=d)
        h.scales_per_row = lambda h=h: SconeTable.scales_per_row(h)
        assert SconeTable.payload_bytes(h) == 2 * d and SconeTable.scales_per_row(h) == 0 and SconeTable.scale_bytes(h) == 0
    header = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    assert re.search(r"\bSCONE_FMT_BF16\s*=\s*4\b", header) and re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", header)
    assert L.ABI_VERSION == 2


class _HostTable:
    """Stand-in for hip_backend.SconeTable in save_native / load_native: holds raw rows on the host."""
    made = []

    def __init__(self, max_n, n_rows, dim=0, table_format="fp32", row_begin=0, row_end=None, **kw):
        self.max_n, self.n_rows, self.dim, self.table_format = max_n, n_rows, dim, table_format
        self.fmt = format_code(table_format)
        self.row_begin, self.row_end = row_begin, n_rows if row_end is None else row_end
        self.rows = np.zeros((self.row_end - self.row_begin, self.payload_bytes()), dtype=np.uint8)
        self.keys = None
        _HostTable.made.append(self)

    def payload_bytes(self):
        return _DeviceTable.payload_bytes(self)

    def scales_per_row(self):
        return _DeviceTable.scales_per_row(self)

    def index_build(self, keys, lens, id0=0):
        self.keys = (np.array(keys), np.array(lens))

    def upload(self, rows, scales=None, row0=0):
        assert scales is None, "a bf16 table has no scales"
        rows = np.ascontiguousarray(rows)
        self.rows[row0 - self.row_begin:row0 - self.row_begin + rows.shape[0]] = rows.view(np.uint8).reshape(rows.shape[0], -1)

    def download(self, row0, nrows, rows=None, scales=None):
        assert scales is None
        rows[:] = self.rows[row0 - self.row_begin:row0 - self.row_begin + nrows]
        return rows, None


def test_native_file_header_round_trip_on_the_host(tmp_path, monkeypatch):
    """save_native writes "bf16" and a [n, 2 d] row section without scales into the v2 header; load_native hands the same
    bytes to a handle of that format.  The device handle is replaced by a host stand-in: no kernel runs."""
    import scone_amd.hip_backend as HB
    from scone_amd import EmbeddingCache, NGramExtractor
    monkeypatch.setattr(HB, "SconeTable", _HostTable)
    _HostTable.made.clear()
    rng = np.random.default_rng(3)
    n, d, max_n = 200, 64, 3
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, 50, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    bits = BF.to_bf16_bits(np.concatenate([BF.edge_values(), rng.standard_normal(n * d).astype(np.float32)])[:n * d].reshape(n, d))
    cache = EmbeddingCache(ex, d, table_format="bfloat16", keep_host_copy=False)
    table = _HostTable(max_n, n, dim=d, table_format="bfloat16")
    table.upload(bits)
    cache._table, cache._dirty, cache._present = table, False, np.ones(n, dtype=bool)
    path = str(tmp_path / "t.npy")
    cache.save_native(path, chunk_rows=64)
    mm = np.load(path, mmap_mode="r")
    hlen = int(np.frombuffer(bytes(mm[:8]), dtype=np.uint64)[0])
    meta = json.loads(bytes(mm[8:8 + hlen]).decode())
    assert meta["magic"] == EmbeddingCache.NATIVE_MAGIC_V2 and meta["table_format"] == "bfloat16"
    assert meta["sections"]["rows"] == {"dtype": "uint8", "shape": [n, 2 * d]} and meta["sections"]["scales"]["shape"] == [n, 0]
    del mm
    again = EmbeddingCache.load_native(path, chunk_rows=48)
    loaded = _HostTable.made[-1]
    assert loaded is not table and again.table_format == "bfloat16" and loaded.fmt == 4 and loaded.dim == d
    assert np.array_equal(BF.rows_as_bits(loaded.rows), bits)
    assert np.array_equal(loaded.keys[0], keys) and np.array_equal(loaded.keys[1], lens)


# ------------------------------------------------------------------ the bf16 translation unit against its fp16 twin
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("asm")
    procs = {}
    for unit in ("bf16", "f16"):
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


def test_no_wave_kernel_of_the_bf16_unit_spills(asm):
    ks = {n: r for n, r in _resources(asm["bf16"]).items() if "k_embed_waveI" in n}
    assert len(ks) >= 40 and all("ILi4E" in n for n in ks), len(ks)          # every (out dtype, dim, max_n, variant) of FMT = 4
    bad = {n[:90]: r for n, r in ks.items() if r.get("ScratchSize", 1) != 0}
    assert not bad, bad


def test_headline_shaped_bf16_kernel_costs_no_more_than_its_fp16_twin(asm):
    tail = "6__halfLi768ELi3ELb1ELb0ELb1E"                     # <FMT, __half, 768, 3, FIXED_POS, !PARTIAL, HIOCC>
    bf = [r for n, r in _resources(asm["bf16"]).items() if "k_embed_waveILi4E" + tail in n]
    f16 = [r for n, r in _resources(asm["f16"]).items() if "k_embed_waveILi1E" + tail in n]
    assert len(bf) == 1 and len(f16) == 1, (len(bf), len(f16))            # bit 4 of SCONE_HIOCC_MASK: the variant exists
    bf, f16 = bf[0], f16[0]
    print("bf16", bf, "fp16 twin", f16)
    assert bf["ScratchSize"] == 0
    assert bf["NumVgprs"] <= f16["NumVgprs"], (bf, f16)
    assert bf["Occupancy"] >= f16["Occupancy"], (bf, f16)
