"""CPU only.  (1) The Python model of the f-gram index (tests/index_model.py) against the product's own `__host__ __device__`
functions, through the stand-alone host program tests/index_model_check.cpp: every printed field -- ok, lo, ext, hash, home
bucket, step, bitmap bit -- of a few thousand keys in both key layouts.  (2) Every generator of hostile index states meets the
minimum its name promises, measured on the arrays it returns: a generator that silently stops producing crowded buckets, bitmap
false positives or a saturated tile fails here, before anything runs on a GPU (tests/test_gpu_index_stress.py)."""

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = [s[0] for s in M.states()]


# ------------------------------------------------------------------ 1. the model against the header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to compile tests/index_model_check.cpp for the host"
    exe = str(tmp_path_factory.mktemp("index_model") / "index_model_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "index_model_check.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    return exe


def _boundary_tokens():
    out = {0, 1, 2, 0xFFFE, 0xFFFF, 0x10000, 0x10001, 2**31 - 2, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1}
    for e in (18, 20, 24):
        out |= {2**e - 3, 2**e - 2, 2**e - 1, 2**e, 2**e + 1, 2**e + 3}
    return sorted(out)


def _cases():
    """[(max_n, tokens, capacity)]: the boundary tokens in every place of every length, the unpackable ones, random 32- and
    24-bit tokens, and every key of every generator state at the state's capacity."""
    rng = np.random.default_rng(5)
    edge = _boundary_tokens()
    caps = [4, 64, 1024, 1 << 20, 1 << 27, 1 << 31]
    out = []
    for max_n in (1, 2, 3, 4):
        for n in range(1, max_n + 1):
            for place in range(n):
                for t in edge:
                    g = [int(rng.integers(0, 50000)) for _ in range(n)]
                    g[place] = t
                    out.append((max_n, tuple(g), caps[len(out) % len(caps)]))
            for t in edge:                                # the same token in every place
                out.append((max_n, (t,) * n, caps[len(out) % len(caps)]))
            for _ in range(150):
                top = 2**32 if rng.random() < 0.5 else 2**24
                out.append((max_n, tuple(int(x) for x in rng.integers(0, top, size=n)), caps[len(out) % len(caps)]))
    for name in STATES:
        max_n, keys, lens, capacity, _, _ = M.state(name)
        for g in M.distinct_keys(keys, lens):
            out.append((max_n, g, capacity))
    return out


def test_bitmap_size_rule():
    """bits = clamp(8 * capacity, 1024, 2^30)"""
    assert [M.bloom_bits(c) for c in (4, 64, 128, 256, 1024, 1 << 20, 1 << 27, 1 << 28, 1 << 40)] == \
        [1024, 1024, 1024, 2048, 8192, 1 << 23, 1 << 30, 1 << 30, 1 << 30]


def test_model_agrees_with_the_header_on_every_field(checker, tmp_path):
    cases = _cases()
    assert len(cases) >= 3000
    assert {m for m, _, _ in cases} == {1, 2, 3, 4}
    assert sum(1 for m, g, _ in cases if m == 4 and max(g) >= M.TOKEN_LIMIT_N4) >= 100, "no unpackable keys were fed"
    assert sum(1 for m, g, _ in cases if m <= 3 and max(g) == 2**32 - 1) >= 10
    path = tmp_path / "keys.txt"
    with open(path, "w") as f:
        for max_n, g, cap in cases:
            t = list(g) + [0] * (4 - len(g))
            f.write(f"{max_n} {len(g)} {t[0]} {t[1]} {t[2]} {t[3]} {cap - 1} {M.bloom_bits(cap) - 1}\n")
    p = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    n_bad_keys = 0
    for (max_n, g, cap), line in zip(cases, lines):
        got = tuple(int(x) for x in line.split())
        ok, lo, ext = M.pack_key(g, max_n)
        h = M.hash_key(lo, ext)
        want = (int(ok), lo, ext, h, M.bucket_home(h, cap - 1), M.bucket_step(h), M.bloom_bit(h, M.bloom_bits(cap) - 1))
        assert got == want, (max_n, g, cap, dict(zip("ok lo ext hash home step bit".split(), zip(got, want))))
        n_bad_keys += not ok
        if ok:
            assert (lo, ext) != (0, 0) and want[5] & 1 and want[4] < cap // 4 and want[6] < M.bloom_bits(cap)
    assert n_bad_keys >= 100


def test_max_n_2_has_no_shared_lo_state():
    """Why shared_lo starts at max_n = 3: in the 32-bit layout ext is token 2 + 1, so keys of length <= 2 all have ext = 0 and
    two distinct ones never share lo."""
    rng = np.random.default_rng(6)
    seen = {}
    for _ in range(5000):
        g = tuple(int(x) for x in rng.integers(0, 40, size=int(rng.integers(1, 3))))
        ok, lo, ext = M.pack_key(g, 2)
        assert ok and ext == 0 and seen.setdefault(lo, g) == g
    with pytest.raises(ValueError):
        M.shared_lo(2)


# ------------------------------------------------------------------ 2. every state is what its name says
@pytest.mark.parametrize("name", STATES)
def test_state_is_a_legal_index_and_a_legal_batch(name):
    max_n, keys, lens, capacity, batch, facts = M.state(name)
    n = len(lens)
    assert keys.shape == (n, max_n) and keys.dtype == np.uint32 and lens.dtype == np.uint8
    assert lens.min() >= 1 and lens.max() <= max_n
    assert (keys[np.arange(max_n)[None, :] >= lens[:, None]] == 0).all()
    dist = M.distinct_keys(keys, lens)
    assert all(M.pack_key(g, max_n)[0] for g in dist), "a key that the build would refuse"
    assert capacity >= 4 and capacity & (capacity - 1) == 0 and len(dist) <= capacity
    assert facts["n_rows"] == n and facts["n_distinct"] == len(dist)
    b = facts["chunk_bounds"]
    assert b[0] == 0 and b[3] == n and b[0] < b[1] < b[2] < b[3]
    # the batch: -1 tokens, several sequences, ragged packed form with an empty sequence, about 6,000 tokens at the most
    B, T = batch.rect.shape
    assert batch.rect.dtype == np.int64 and batch.packed.dtype == np.int64
    assert batch.cu[0] == 0 and batch.cu[-1] == len(batch.packed) and (np.diff(batch.cu) >= 0).all()
    for form in ("rect", "packed"):
        assert 0 < facts[f"{form}_tokens"] <= M.MAX_BATCH_TOKENS
        assert facts[f"{form}_minus_one_tokens"] > 0 and facts[f"{form}_sequences"] >= 3
        assert facts[f"{form}_present_windows"] >= 64 and facts[f"{form}_absent_windows"] >= 64
        toks = batch.rect if form == "rect" else batch.packed
        assert toks.min() == -1 and toks.max() <= 2**31 - 1
    assert facts["rect_tokens"] == B * T and B * T > 254 and len(batch.packed) > 254          # more than one tile of the tiled match
    assert facts["keys_missing_from_batch"] == 0                      # wherever the build put a key, some window asks for it
    assert facts["packed_empty_sequences"] >= 1 and facts["packed_distinct_lengths"] >= 3


@pytest.mark.parametrize("max_n", [2, 3, 4])
def test_crowded(max_n):
    _, _, _, capacity, _, f = M.state(f"crowded-n{max_n}")
    assert f["crowded_buckets"] >= M.CROWDED_BUCKETS == 8
    assert f["crowded_min_keys"] >= M.CROWDED_KEYS == 12
    assert f["keys_beyond_their_home_at_least"] >= 8 * 8                     # a bucket holds 4 of its 12
    assert 0.70 <= f["load"] <= 0.80
    assert f["crowded_keys"] >= 8 * 12 and f["crowded_keys_missing_from_batch"] == 0


@pytest.mark.parametrize("capacity", M.FULL_CAPACITIES)
@pytest.mark.parametrize("max_n", [2, 3, 4])
def test_full(max_n, capacity):
    _, _, _, cap, _, f = M.state(f"full{capacity}-n{max_n}")
    assert cap == capacity == f["n_distinct"] == f["n_rows"] and f["buckets"] == capacity // 4
    assert f["lengths_present"] == list(range(1, max_n + 1))
    assert f["false_positive_absent_windows"] >= M.FULL_FALSE_POSITIVES == 32
    assert f["false_positive_absent_wide_unigrams"] >= 8
    assert len(f["present_windows_per_length"]) == max_n and min(f["present_windows_per_length"]) >= M.FULL_PRESENT_PER_LENGTH == 32


@pytest.mark.parametrize("max_n", [3, 4])
def test_shared_lo(max_n):
    _, _, _, _, _, f = M.state(f"shared_lo-n{max_n}")
    assert f["pairs"] >= M.SHARED_PAIRS == 64
    assert f["pairs_token2_moved_by_65536"] + f["pairs_last_token_differs"] == f["pairs"]
    if max_n == 3:
        assert f["pairs_last_token_differs"] >= 64
    else:
        assert f["pairs_token2_moved_by_65536"] >= 24 and f["pairs_last_token_differs"] >= 24
    assert f["shorter_key_present"] >= 24 and f["shorter_key_absent_bit_set"] >= 24


@pytest.mark.parametrize("max_n", [2, 3, 4])
def test_wide(max_n):
    _, _, _, _, _, f = M.state(f"wide-n{max_n}")
    assert f["saturated_run"] >= M.WIDE_RUN == 600
    assert f["saturated_run"] >= 2 * 254 + max_n                              # a whole 254-position tile, wherever the tiles start
    assert f["boundary_tokens_in_keys"] == sorted(M.wide_tokens(max_n)) and f["wide_tokens_as_unigram_keys"] == 5
    assert M.wide_tokens(max_n)[:4] == [2**18 - 1, 2**18, 2**18 + 1, 2**20 + 3]
    assert M.wide_tokens(max_n)[4] == (2**24 - 2 if max_n == 4 else 2**31 - 1)
    assert f["wide_unigram_windows_at_or_above_2_18"] >= 600 and f["absent_tokens_in_batch"] >= 4
    assert f["unpackable_tokens_in_batch"] == (2 if max_n == 4 else 0)
    assert M.unpackable_tokens(4) == [2**24 - 1, 2**31 - 1]


@pytest.mark.parametrize("max_n", [2, 3, 4])
def test_duplicates(max_n):
    _, _, _, _, _, f = M.state(f"duplicates-n{max_n}")
    assert f["n_dups"] == f["n_rows"] - f["n_distinct"] >= 64
    assert f["duplicated_keys_in_several_chunks"] >= 64
    assert f["duplicated_keys_smallest_id_not_in_chunk_0"] >= 16 and f["duplicated_keys_smallest_id_not_in_chunk_2"] >= 16
    assert f["duplicated_unigrams_below_2_18"] >= 8 and f["duplicated_unigrams_at_or_above_2_18"] >= 8
    assert f["duplicated_keys_missing_from_batch"] == 0


def test_generators_are_deterministic():
    for gen, args in ((M.crowded, (3,)), (M.full, (4, 64)), (M.shared_lo, (4,)), (M.wide, (2,)), (M.duplicates, (3,))):
        a, b = gen(*args), gen(*args)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[4] == b[4]
        assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
