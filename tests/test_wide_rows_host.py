"""What tests/test_gpu_wide_rows.py takes for granted about its inputs (tests/wide_rows_fixture.py), checked without a GPU."""

import os
import sys

import numpy as np
import pytest

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_geometry as G  # noqa: E402
import wide_rows_fixture as F  # noqa: E402


def test_scale_bytes_per_row_and_which_cases_exceed_one_pass():
    """One pass of a wave at 2 bytes per lane moves 128 scale bytes: INT4 8192 sits exactly there (the control), MXFP4 5120 /
    8192 and INT4 16384 beyond."""
    got = {F.case_id(c): F.scale_bytes(*c) for c in F.CASES}
    assert got == {"fp32-d4100": 0, "bf16-d4104": 0, "int8-d4112": 2, "fp16-d8192": 0, "int8-d8192": 2, "int4-d8192": 128,
                   "int4-d16384": 256, "mxfp4-d5120": 160, "mxfp4-d8192": 256, "fp32-d16384": 0}
    over = {F.case_id(c) for c in F.CASES if F.scale_bytes(*c) > F.COPY_LANE_BYTES}
    assert over == {"int4-d16384", "mxfp4-d5120", "mxfp4-d8192"}
    assert set(F.STAGED) <= set(F.CASES) and {c for c in F.CASES if F.scale_bytes(*c) and c[1] >= 5120} | {("fp16", 8192)} == set(F.STAGED)
    assert max(d for _, d in F.CASES) == F.WIDEST
    for fmt, d in F.CASES:
        assert d > 4096 and d % {"fp32": 4, "fp16": 8, "bf16": 8, "int8": 16, "int4": 128, "mxfp4": 128}[fmt] == 0
        # the quantised table really has that many scale bytes per row
        if (fmt, d) in (("int4", 8192), ("mxfp4", 5120), ("int8", 4112)):
            t = F.tables(fmt, d)
            assert t["scales"].shape[0] == F.n_rows() and t["scales"].nbytes == F.n_rows() * F.scale_bytes(fmt, d)
            assert len(np.unique(t["scales"])) > (1 if fmt == "int8" else 8)     # the scales differ along a row / between rows
    assert F.kernel_family("fp32", 4100) == "k_embed" and (4104 // 8, 4112 // 8, 5120 // 8) == (513, 514, 640)
    assert all(F.kernel_family(fmt, d) == "k_embed_wave_any" for fmt, d in F.CASES if d != 4100)


@pytest.mark.parametrize("name", sorted(F.RECTS))
def test_every_list_length_occurs_in_the_rectangles(name):
    """Every K the kernels' `switch (kown)` can meet at this T, in the rectangle and in its packed form per sequence length."""
    tok, pos = F.rect(name)
    B, T = F.RECTS[name]
    assert tok.shape == (B, T) and pos.shape == (B, T)
    keys, lens = F.vocabulary()
    kmax = G.max_list_length(T, F.MAX_N)
    assert kmax == F.MAX_N * (F.MAX_N + 1) // 2                        # T >= 2 max_n - 1: the full cover
    hist = np.bincount(F.list_lengths(keys, lens, tok), minlength=kmax + 1)
    assert len(hist) == kmax + 1 and (hist > 0).all(), hist.tolist()
    # longest_suffix: no f-gram, a bigram and a trigram end at some token
    f2id = R._key_dict(keys, lens)
    ids = np.asarray([R.paper_lookup(f2id, F.MAX_N, row.tolist()) for row in tok])
    assert (ids < 0).any() and {int(lens[i]) for i in ids[ids >= 0]} == {2, 3}
    flat, cu, seqs = F.packed(name)
    assert cu[0] == 0 and cu[-1] == B * T == flat.size and (np.diff(cu) == 0).any() and (np.diff(cu) == 1).any()
    assert len({len(s) for s in seqs}) == len(seqs) and np.array_equal(np.concatenate(seqs), tok.reshape(-1))


def test_walk_batch_makes_a_workgroup_walk_three_sequences():
    """At least 3 sequences per workgroup and a shorter last run, on 256 and on 240 compute units: every width here takes
    k_embed_wave_any, whose grid is a fixed 4096 workgroups whatever the chip (only k_embed_wave, d = 768 / 1024 / 1280, sizes
    its grid from the compute units), so the two answers are one."""
    for cus, (fmt, d) in ((cus, c) for cus in (256, 240) for c in F.CASES):
        B, T = F.walk_shape(d)
        assert B * T <= 16400 and (d < F.WIDEST or B * T * d * 2 < 300e6)
        if F.kernel_family(fmt, d) == "k_embed":
            continue                                                    # no walk: one lane group per token
        assert F.kernel_family(fmt, d) == "k_embed_wave_any" and d not in G.WAVE_DIMS
        g = G.wave_any(B, T)
        assert g.seqs_per_block >= 3 and 0 < g.last_run < g.seqs_per_block, g
        assert (g.chunks - 1) * g.seqs_per_block + g.last_run == B and g.pos_groups == 1
        assert not G.takes_one_launch(F.GEOM.get(fmt, fmt), d, B * T)
    assert G.wave_any(8192, 1).seqs_per_block == 2                      # one sequence fewer than 8193 and the walk is shorter
    for T in (1, 2):
        tok, pos = F.walk(T)
        keys, lens = F.vocabulary()
        hist = np.bincount(F.list_lengths(keys, lens, tok), minlength=G.max_list_length(T, F.MAX_N) + 1)
        assert (hist > 0).all() and len(hist) == G.max_list_length(T, F.MAX_N) + 1
        assert (pos[1:] != pos[:-1]).mean() > 0.9                       # positions differ between the sequences a workgroup walks


def test_staged_batch_references_cold_rows_in_three_chunks():
    tok, _ = F.rect("9x37")
    B, T = tok.shape
    keys, lens = F.vocabulary()
    chunks = F.stage_chunks(B, T, F.STAGE_TOKENS)
    assert [n for _, n in chunks] == [4, 4, 1]                          # at least 3 chunks, a ragged last one
    for b, n in chunks:
        cold = F.referenced(keys, lens, tok[b:b + n], F.MAX_N, F.HOT_ROWS)
        assert len(cold) > 0, (b, n)
    hits = R.match_hits(keys, lens, tok, F.MAX_N)
    assert ((hits >= 0) & (hits < F.HOT_ROWS)).any()                    # the head in HBM is used as well
    n_cold = F.n_rows() - F.HOT_ROWS
    # (STAGE_PROTECT + 1) chunks' worst case exceeds the cold rows: the whole cold table fits the cache, nothing is evicted
    assert F.STAGE_PROTECTED_CHUNKS * 4 * T * 6 >= n_cold
    assert 3 <= len(F.referenced(keys, lens, tok, F.MAX_N, F.HOT_ROWS)) <= n_cold


@pytest.mark.parametrize("fmt,d", F.EVICT_CASES)
def test_eviction_batch_references_more_cold_rows_than_the_cache_has_slots(fmt, d):
    keys, lens = F.evict_vocabulary()
    assert len(lens) == 600 and F.EVICT_SLOTS == 84
    x = F.evict_inputs(fmt, d)
    tok = x["tok"]
    assert tok.shape == (400, 2)
    cold = F.referenced(keys, lens, tok, F.EVICT_MAX_N, F.EVICT_TOKENS)
    assert F.EVICT_SLOTS < len(cold) <= 576
    assert len(F.stage_chunks(400, 2, F.EVICT_STAGE_TOKENS)) == 400     # one sequence per chunk
    # a pass ends with at most 84 rows cached and the next one references len(cold) > 84 distinct rows: it must copy some again
    assert (F.list_lengths(keys, lens, tok, F.EVICT_MAX_N) == 2).all()  # a unigram and the bigram of the pair
    assert F.scale_bytes(fmt, d) == {"int4": 16, "mxfp4": 160}[fmt] and x["scales"].shape[0] == 600
