#!/usr/bin/env python3
"""The streaming fit (scone_fit_state) beside the one-shot scone_fit at scale, run on the GPU box: the 30M-token Zipf corpus of
tools/fit_scale_check.py (6,000 texts of 5,000 tokens, max_n 3, min_freq 2), its numpy cross-check of distinct n-grams and
counts, and for every route three timed repeats (interleaved, after a warm-up of every route), the device memory it holds and
its growth events.  Routes: one-shot scone_fit; streaming in chunks of 2^20, 2^22, 2^24 tokens and as one chunk; and, to tell
atomic contention on hot unigram slots from probe traffic, the one-shot and the 2^22 stream on a uniform-token corpus.

The corpus is resident on the device before the clock starts; a time is wall time between two device synchronises and includes
the copy of the result to the host (both routes make it).  Writes one JSON record (--out, default
profiles/r13a/fit_stream.json)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scone_amd import synthetic as S
from scone_amd.hip_backend import FitState, fit_gpu, fit_occurrences

MAX_N, MIN_FREQ, MAX_F = 3, 2, 5_000_000


def numpy_check(tok, keys, lens, counts, n_distinct):
    """tools/fit_scale_check.py's check: distinct n-grams, per-key counts, and the descending count list."""
    n_texts, tlen = tok.shape
    V = np.uint64(1 << 21)
    ref_counts, distinct = [], 0
    for n in range(1, MAX_N + 1):
        packed = np.zeros((n_texts, tlen - n + 1), dtype=np.uint64)
        for k in range(n):
            packed = packed * V + tok[:, k:tlen - n + 1 + k].astype(np.uint64)
        u, c = np.unique(packed.reshape(-1), return_counts=True)
        distinct += len(u)
        ref_counts.append(c[c >= MIN_FREQ])
        sel = np.nonzero(lens == n)[0]
        pk = np.zeros(len(sel), dtype=np.uint64)
        for k in range(n):
            pk = pk * V + keys[sel, k].astype(np.uint64)
        pos = np.searchsorted(u, pk)
        assert np.array_equal(u[pos], pk), "a kept key does not occur in the corpus"
        assert np.array_equal(c[pos], counts[sel].astype(np.int64)), "count mismatch for length %d" % n
    ref = np.sort(np.concatenate(ref_counts))[::-1]
    assert distinct == n_distinct, (distinct, n_distinct)
    assert np.array_equal(ref[:len(lens)], counts.astype(np.int64)), "counts are not the top of the descending list"
    return distinct


def pow2_at_least(x, floor=1024):
    p = floor
    while p < x:
        p <<= 1
    return p


def run_one_shot(d_tok, d_off):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fit_gpu(d_tok, d_off, MAX_N, MIN_FREQ, MAX_F)
    torch.cuda.synchronize()
    return {"total_s": time.perf_counter() - t0}, res


def run_stream(d_tok, d_off, texts_per_chunk):
    """texts are equally long here, so a chunk of c tokens is c / tlen whole texts"""
    n_texts = d_off.numel() - 1
    tlen = d_tok.numel() // n_texts
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    with FitState(MAX_N) as st:
        for a in range(0, n_texts, texts_per_chunk):
            b = min(n_texts, a + texts_per_chunk)
            lo, hi = a * tlen, b * tlen
            st.update(d_tok[lo:hi], d_off[a:b + 1] - lo)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        free1 = torch.cuda.mem_get_info()[0]
        res = st.finalize(MIN_FREQ, MAX_F)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        stats = st.stats()
    return {"total_s": t2 - t0, "update_s": t1 - t0, "finalize_s": t2 - t1, "slots": stats["slots"],
            "state_bytes": 32 * stats["slots"], "mem_get_info_held_bytes": free0 - free1, "n_grows": stats["n_grows"],
            "n_distinct": stats["n_distinct"], "n_occurrences": stats["n_occurrences"]}, res


def summarise(samples):
    out = {}
    for k in samples[0]:
        v = [s[k] for s in samples]
        if k.endswith("_s"):
            out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
        else:
            out[k] = v[-1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13a",
                                                  "fit_stream.json"))
    ap.add_argument("--texts", type=int, default=6000)
    ap.add_argument("--tlen", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-uniform", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: no time is ever taken on a CPU"
    n_texts, tlen = args.texts, args.tlen
    n_tok = n_texts * tlen
    occ = fit_occurrences([tlen] * n_texts, MAX_N)
    off = torch.arange(n_texts + 1, dtype=torch.int64) * tlen
    d_off = off.cuda()
    corpora = {"zipf": S.stream_zipf(S.GPT2_VOCAB, n_texts, tlen, 21).astype(np.int64)}
    if not args.no_uniform:
        corpora["uniform"] = np.random.default_rng(22).integers(0, S.GPT2_VOCAB, size=(n_texts, tlen), dtype=np.int64)
    chunkings = {"stream_2^20": max(1, (1 << 20) // tlen), "stream_2^22": max(1, (1 << 22) // tlen),
                 "stream_2^24": max(1, (1 << 24) // tlen), "stream_one_chunk": n_texts}
    record = {"corpus": {"texts": n_texts, "tokens_per_text": tlen, "tokens": n_tok, "occurrences": occ, "vocab": S.GPT2_VOCAB},
              "fit": {"max_n": MAX_N, "min_freq": MIN_FREQ, "max_f_grams": MAX_F}, "device": torch.cuda.get_device_name(0),
              "timing": "wall time between device synchronises, corpus resident, result copied to the host; repeats interleaved",
              "one_shot_bytes_formula": 28 * pow2_at_least(2 * n_tok * MAX_N) + 16 * n_tok * MAX_N, "runs": {}}
    for cname, tok in corpora.items():
        d_tok = torch.from_numpy(tok.reshape(-1)).to(torch.int32).cuda()
        routes = {"one_shot": lambda: run_one_shot(d_tok, d_off)}
        for name, tpc in chunkings.items():
            if cname == "zipf" or name == "stream_2^22":
                routes[name] = (lambda tpc=tpc: run_stream(d_tok, d_off, tpc))
        small = d_off[:9]
        fit_gpu(d_tok[:8 * tlen], small, MAX_N, MIN_FREQ, MAX_F)                   # warm-up: code objects, rocPRIM, allocator
        with FitState(MAX_N) as st:
            st.update(d_tok[:8 * tlen], small)
            st.finalize(MIN_FREQ, MAX_F)
        samples = {name: [] for name in routes}
        ref = None
        for rep in range(args.repeats):
            for name, fn in routes.items():
                s, res = fn()
                samples[name].append(s)
                print("%-8s %-18s rep %d: %s" % (cname, name, rep, json.dumps(s)), flush=True)
                if name == "one_shot" and ref is None:
                    ref = res
                    if cname == "zipf":
                        t0 = time.time()
                        numpy_check(tok, ref[0], ref[1], ref[2], ref[3])
                        print("numpy cross-check of the one-shot result ok (%.0f s)" % (time.time() - t0), flush=True)
                else:                                                           # every route, every repeat: the same list
                    assert np.array_equal(res[0], ref[0]) and np.array_equal(res[1], ref[1]), name
                    assert np.array_equal(res[2].astype(np.uint64), ref[2].astype(np.uint64)) and res[3] == ref[3], name
                del res
        record["runs"][cname] = {name: summarise(v) for name, v in samples.items()}
        record["runs"][cname]["f_grams_kept"] = int(len(ref[1]))
        record["runs"][cname]["n_distinct"] = int(ref[3])
        del d_tok
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("ok: every route and repeat gave the one-shot's keys, ids and counts; wrote", args.out)


if __name__ == "__main__":
    main()
