"""TEST CODE ONLY -- inputs and expectations for rows wider than d = 4096 (tests/test_gpu_wide_rows.py on the GPU,
tests/test_wide_rows_host.py for the preconditions).  Host only: nothing here touches HIP code, and nothing under scone_amd/
may import this module.

The (format, d) pairs and what each one stresses:

  fp32   4100   d % 8 != 0: the lane-group k_embed; cover mode only (longest_suffix needs d % 8 == 0)
  bf16   4104   513 units of 8 elements: more than 64 and no multiple of 64 in embed_units
  int8   4112   514 units; d % 16
  fp16   8192
  int8   8192
  int4   8192   128 scale bytes per row: exactly what one pass of a wave's 16-bit lanes copies -- the control
  int4   16384  256 scale bytes
  mxfp4  5120   160 scale bytes; 640 units
  mxfp4  8192   256 scale bytes
  fp32   16384  64-KB rows, 32 units per lane

The vocabulary, the token distribution and the rounding helpers are tests/test_gpu_walk_shapes.py's at max_n = 3 (VOCAB = 3,
60 rows, token 3 in no f-gram); tables are quantised here by oracle/ref_port.py (int8 / INT4), tests/mxfp4_fixture.py and
tests/bf16_fixture.py, and the expectation is oracle/ref_port.py's `embed_numpy` / `paper_embed` / `combine` on the fp32 values
those formats stand for.  Every block of 32 elements of a table gets its own power-of-two magnitude, so the scales differ
along a row: a kernel that takes the scale of another group gets another number.

Batches: the rectangles 9 x 37 and 7 x 5, whose seeds are searched (deterministically, from a fixed start) until every id-list
length the kernels' `switch (kown)` can meet at that T occurs; one packed batch per rectangle (the same tokens cut into ragged
sequences, an empty and a one-token sequence among them); and the "walk" batch, 8200 sequences, which makes a workgroup of
k_embed_wave_any walk 3 sequences (tests/walk_geometry.py: its grid is 4096 workgroups for T <= 4, so fewer than 8193
sequences cannot).  That batch has T = 2 below d = 8192 and T = 1 from there on: 8200 tokens of d = 16384 are 269 MB of
half-precision output.
"""

import functools
import os
import sys

import numpy as np
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import mxfp4_fixture as MX  # noqa: E402
import walk_geometry as G  # noqa: E402
import test_gpu_walk_shapes as W  # noqa: E402  (its vocabularies, token distribution, _to / _bits)

CASES = (("fp32", 4100), ("bf16", 4104), ("int8", 4112), ("fp16", 8192), ("int8", 8192), ("int4", 8192), ("int4", 16384),
         ("mxfp4", 5120), ("mxfp4", 8192), ("fp32", 16384))
# the formats with scales, and fp16 as the control without
STAGED = (("int8", 8192), ("int4", 8192), ("int4", 16384), ("mxfp4", 5120), ("mxfp4", 8192), ("fp16", 8192))
WIDEST = 16384
MAX_N = 3
VOCAB, N_POS = W.VOCAB, W.N_POS
HOT_ROWS = 16                 # pinned-host tables: rows [0, 16) stay in HBM
STAGE_TOKENS = 148            # 9 x 37: chunks of 4, 4 and 1 sequences
COPY_LANE_BYTES = 128         # scale bytes one pass of a wave moves at 2 bytes per lane
WALK_B = 8200
GEOM = {"mxfp4": "int4", "bf16": "fp16"}     # tests/walk_geometry.py names its rules by their first users


def case_id(c):
    return f"{c[0]}-d{c[1]}"


def vocabulary():
    return W._vocabulary(MAX_N)


def n_rows():
    return W.N_ROWS[MAX_N]


def payload_bytes(fmt, d):
    return {"fp32": 4 * d, "fp16": 2 * d, "bf16": 2 * d, "int8": d, "int4": d // 2, "mxfp4": d // 2}[fmt]


def scale_bytes(fmt, d):
    """Bytes of scales per row: one fp16 (int8), one fp16 per 128 elements (INT4), one E8M0 byte per 32 (MXFP4)."""
    return {"int8": 2, "int4": 2 * (d // 128), "mxfp4": d // 32}.get(fmt, 0)


def kernel_family(fmt, d):
    return G.kernel_family(GEOM.get(fmt, fmt), d)


def quantise(fmt, table):
    """(payload uint8 [n, payload bytes], scales in logical order or None, the fp32 values the format stands for)."""
    n = table.shape[0]
    if fmt == "fp32":
        return np.ascontiguousarray(table).view(np.uint8).reshape(n, -1), None, table
    if fmt == "fp16":
        h = table.astype(np.float16)
        return h.view(np.uint8).reshape(n, -1), None, h.astype(np.float32)
    if fmt == "bf16":
        b = BF.to_bf16_bits(table)
        return b.view(np.uint8).reshape(n, -1), None, BF.from_bf16_bits(b)
    if fmt == "int8":
        q, s = R.quantize_i8(table)
        return q.view(np.uint8).reshape(n, -1), s.reshape(n, 1), R.dequantize_i8(q, s)
    if fmt == "int4":
        p, s = R.quantize_i4(table)
        return p, s, R.dequantize_i4(p, s)
    p, s = MX.quantize(table)
    return p, s, MX.dequantize(p, s)


def _magnitudes(rng, n, d):
    """fp32 [n, d]: one power of two in 2^-6 .. 2^6 per block of 32 elements."""
    nb = (d + 31) // 32
    return np.exp2(rng.integers(-6, 7, size=(n, nb))).repeat(32, axis=1)[:, :d]


@functools.lru_cache(maxsize=None)
def tables(fmt, d):
    """dict: table (fp32 rows given to the handle), payload, scales, stored (fp32), wte [VOCAB + 1, d], wpe [N_POS, d]."""
    rng = np.random.default_rng(11 * d + CASES.index((fmt, d)))
    n = n_rows()
    table = (rng.standard_normal((n, d)) * _magnitudes(rng, n, d)).astype(np.float32)
    payload, scales, stored = quantise(fmt, table)
    assert payload.shape == (n, payload_bytes(fmt, d)) and stored.shape == (n, d) and stored.dtype == np.float32
    assert np.isfinite(stored).all()
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return {"table": table, "payload": payload, "scales": scales, "stored": stored, "wte": wte, "wpe": wpe}


# ------------------------------------------------------------------ batches
RECTS = {"9x37": (9, 37), "7x5": (7, 5)}


def list_lengths(keys, lens, tok, max_n=MAX_N):
    off, _ = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
    return np.diff(off)


@functools.lru_cache(maxsize=None)
def rect(name):
    """(tok [B, T], pos [B, T]): the first seed from 7000 on at which every list length 0 .. max_list_length(T) occurs."""
    B, T = RECTS[name]
    keys, lens = vocabulary()
    kmax = G.max_list_length(T, MAX_N)
    for seed in range(7000 + 100 * T, 7000 + 100 * T + 400):
        rng = np.random.default_rng(seed)
        tok = rng.choice(VOCAB + 1, size=(B, T), p=W.TOKEN_P).astype(np.int64)
        hist = np.bincount(list_lengths(keys, lens, tok), minlength=kmax + 1)
        if (hist > 0).all():
            pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
            return tok, pos
    raise AssertionError(f"no seed gives every list length at {name}")


def walk_shape(d):
    return WALK_B, (2 if d < 8192 else 1)


@functools.lru_cache(maxsize=None)
def walk(T):
    rng = np.random.default_rng(8200 + T)
    tok = rng.choice(VOCAB + 1, size=(WALK_B, T), p=W.TOKEN_P).astype(np.int64)
    pos = rng.integers(0, N_POS, size=(WALK_B, T)).astype(np.int64)
    return tok, pos


@functools.lru_cache(maxsize=None)
def packed(name):
    """The rectangle's tokens cut into ragged sequences: (tok [total], cu_seqlens [n + 1], the sequences as arrays)."""
    tok, _ = rect(name)
    flat = tok.reshape(-1)
    total = flat.size
    lengths = {"9x37": [38, 0, 1, 64, 5, 2, 60, 63, 41, 59], "7x5": [5, 1, 0, 3, 26]}[name]
    assert sum(lengths) == total and max(lengths) <= N_POS            # default positions stay inside wpe
    cu = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=cu[1:])
    return flat.copy(), cu, [flat[a:b] for a, b in zip(cu[:-1], cu[1:])]


# ------------------------------------------------------------------ expectations
def want(stored, tok, reduce="mean", mode="cover", wte32=None, wpe32=None, pos=None, base32=None, vocab=None):
    """fp32 [B, T, d]: (first + f-gram) + position, the oracle on the fp32 values the table stands for.  `first` is wte[tok], a
    dense base [B, T, d], or +0; absent terms are rows of +0.  `vocab` = (keys, lens, max_n), this module's by default."""
    keys, lens, max_n = vocab if vocab is not None else (*vocabulary(), MAX_N)
    B, T = tok.shape
    d = stored.shape[1]
    pid = np.array(pos if pos is not None else np.broadcast_to(np.arange(T), (B, T)))          # (a writable copy)
    if mode == "cover":
        off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
        fg = R.embed_numpy(stored, off, ids, reduce).reshape(B, T, d)
        if base32 is not None:
            first = base32.reshape(B, T, d) + fg
            return first + (wpe32[pid] if wpe32 is not None else np.float32(0))
        n_tok = int(tok.max()) + 1
        return R.combine(torch.from_numpy(tok), torch.from_numpy(fg),
                         torch.from_numpy(wte32) if wte32 is not None else torch.zeros((n_tok, d)),
                         torch.from_numpy(wpe32) if wpe32 is not None else torch.zeros((N_POS, d)),
                         position_ids=torch.from_numpy(pid)).numpy()
    assert base32 is None
    e = R.paper_embed(R._key_dict(keys, lens), max_n, tok, stored, wte=wte32)          # (0 + e) + 0
    return e + wpe32[pid] if wpe32 is not None else e


def want_packed(stored, seqs, **kw):
    """fp32 [total, d]: every sequence alone (no window crosses a boundary; the default position is the place inside it)."""
    parts = [want(stored, s[None, :], **kw)[0] for s in seqs if len(s)]
    return np.concatenate(parts)


def referenced(keys, lens, tok, max_n, lo):
    """The distinct row ids >= lo among the batch's hits."""
    hits = R.match_hits(keys, lens, tok, max_n)
    return np.unique(hits[hits >= lo])


def stage_chunks(B, T, stage_tokens):
    """[(first sequence, sequences)]: how a staged lookup cuts a batch (chunks of whole sequences)."""
    seqs = max(1, min(stage_tokens // T, B))
    return [(b, min(seqs, B - b)) for b in range(0, B, seqs)]


# ------------------------------------------------------------------ eviction: a cache smaller than what the batch references
EVICT_CASES = (("int4", 1024), ("mxfp4", 5120))
EVICT_TOKENS, EVICT_MAX_N, EVICT_STAGE_TOKENS, EVICT_B, EVICT_T = 24, 3, 2, 400, 2
STAGE_PROTECTED_CHUNKS = 7            # scone_stage_prepare: (STAGE_PROTECT + 1) chunks' worst case, STAGE_PROTECT = ring of 5 + 1
EVICT_SLOTS = STAGE_PROTECTED_CHUNKS * EVICT_STAGE_TOKENS * (EVICT_MAX_N * (EVICT_MAX_N + 1) // 2)


@functools.lru_cache(maxsize=None)
def evict_vocabulary():
    """The 24 unigrams (id = token), then all 576 bigrams (id = 24 + 24 a + b)."""
    v = EVICT_TOKENS
    keys = np.zeros((v + v * v, EVICT_MAX_N), dtype=np.uint32)
    lens = np.ones(v + v * v, dtype=np.uint8)
    keys[:v, 0] = np.arange(v)
    ab = np.arange(v * v)
    keys[v:, 0], keys[v:, 1] = ab // v, ab % v
    lens[v:] = 2
    return keys, lens


@functools.lru_cache(maxsize=None)
def evict_inputs(fmt, d):
    rng = np.random.default_rng(5 * d + 1)
    n = EVICT_TOKENS + EVICT_TOKENS ** 2
    table = (rng.standard_normal((n, d)) * _magnitudes(rng, n, d)).astype(np.float32)
    payload, scales, stored = quantise(fmt, table)
    tok = rng.integers(0, EVICT_TOKENS, size=(EVICT_B, EVICT_T)).astype(np.int64)
    wte = rng.standard_normal((EVICT_TOKENS, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return {"table": table, "payload": payload, "scales": scales, "stored": stored, "tok": tok, "wte": wte, "wpe": wpe}
