"""Shared by test_fit_partition_host.py and test_gpu_fit_partition.py: the 702-text Zipf corpus, its Counter, and the key
packing, the hash and the key-hash partition formula of include/scone_hip.h restated in numpy (independent of the library).
Everything is computed once and never modified.  Needs no GPU."""

import functools
from collections import Counter

import numpy as np

CHUNK_TOKENS = 2048          # many chunks and several growth events on this corpus
N_TOKENS = 204_815
N_DISTINCT = {3: 254_924, 4: 450_514}


@functools.lru_cache(maxsize=None)
def corpus():
    """700 Zipf texts of 1..599 tokens over 5000 ids (seed 4), an empty text and the text (3,): 204,815 tokens."""
    from scone_amd import synthetic as S
    rng = np.random.default_rng(4)
    cdf = S.zipf_cdf(5000)
    return tuple(tuple(S.zipf_tokens(rng, cdf, int(rng.integers(1, 600))).tolist()) for _ in range(700)) + ((), (3,))


@functools.lru_cache(maxsize=None)
def counter(max_n):
    """The reference's fit loop (n_gram_extractor.py:72-104): a Counter in insertion order."""
    c = Counter()
    for text in corpus():
        for n in range(1, min(max_n, len(text)) + 1):
            c.update(text[i:i + n] for i in range(len(text) - n + 1))
    return c


def as_arrays(grams, max_n):
    keys = np.zeros((len(grams), max_n), dtype=np.uint32)
    lens = np.fromiter((len(g) for g in grams), dtype=np.uint8, count=len(grams))
    for n in range(1, max_n + 1):
        sel = np.nonzero(lens == n)[0]
        if sel.size:
            keys[sel, :n] = np.array([grams[i] for i in sel], dtype=np.uint32).reshape(-1, n)
    return keys, lens


@functools.lru_cache(maxsize=None)
def distinct(max_n):
    """(keys [D, max_n] uint32, lens [D] uint8, counts [D] uint64) of every distinct n-gram, in insertion order."""
    c = counter(max_n)
    keys, lens = as_arrays(list(c.keys()), max_n)
    return keys, lens, np.fromiter(c.values(), dtype=np.uint64, count=len(c))


@functools.lru_cache(maxsize=None)
def host_fit(max_n, min_freq, max_f):
    """NGramExtractor.fit's list (Counter.most_common, n_gram_extractor.py:91-99) with its counts."""
    pairs = [(g, n) for g, n in counter(max_n).most_common(max_f) if n >= min_freq]
    keys, lens = as_arrays([g for g, _ in pairs], max_n)
    return keys, lens, np.array([n for _, n in pairs], dtype=np.uint64)


# ------------------------------------------------------------------ the contract of include/scone_hip.h, in numpy
def pack_key(keys, lens, max_n):
    """scone_pack_key: tokens stored + 1, absent positions 0.  Returns (lo uint64 [n], ext uint32 [n])."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, max_n)
    lens = np.asarray(lens).reshape(-1, 1)
    v = np.where(np.arange(max_n)[None, :] < lens, keys + np.uint64(1), np.uint64(0))
    v = np.concatenate([v, np.zeros((v.shape[0], 4 - max_n), dtype=np.uint64)], axis=1)
    if max_n <= 3:
        lo = v[:, 0] | (v[:, 1] << np.uint64(32))
        ext = v[:, 2]
    else:
        lo = v[:, 0] | (v[:, 1] << np.uint64(24)) | ((v[:, 2] & np.uint64(0xFFFF)) << np.uint64(48))
        ext = (v[:, 2] >> np.uint64(16)) | (v[:, 3] << np.uint64(8))
    return lo, ext.astype(np.uint32)


def hash_key(lo, ext):
    """scone_hash_key: 64-bit arithmetic that wraps."""
    x = lo ^ (ext.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def partition(keys, lens, max_n, n_parts):
    """part = (uint32)(((hash >> 32) * n_parts) >> 32): the UPPER half of the hash scaled to [0, n_parts)."""
    h = hash_key(*pack_key(keys, lens, max_n))
    return (((h >> np.uint64(32)) * np.uint64(n_parts)) >> np.uint64(32)).astype(np.uint32)


# ------------------------------------------------------------------ helpers of the GPU tests
@functools.lru_cache(maxsize=None)
def chunks(chunk_tokens=CHUNK_TOKENS):
    from scone_amd import NGramExtractor
    return tuple(NGramExtractor._chunks(corpus(), chunk_tokens))


def sort_rows(keys, lens, *more):
    order = np.lexsort(tuple(keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)) + (lens,))
    return (keys[order], lens[order]) + tuple(m[order] for m in more)


def pow2_at_least(x, floor=1024):
    p = floor
    while p < x:
        p <<= 1
    return p
