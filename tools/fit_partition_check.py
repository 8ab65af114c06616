#!/usr/bin/env python3
"""The key-hash partitioned fit (scone_fit_update_part / scone_fit_finalize_seq) at scale, run on the GPU box: the 30M-token Zipf
corpus of tools/fit_scale_check.py (6,000 texts of 5,000 tokens, max_n 3, min_freq 2), resident on the device, streamed in
chunks of 2^20 tokens with P = 1, 2, 4, 8 partitions, three interleaved repeats after a warm-up of every route.  P = 1 is the plain
streaming route; P > 1 makes P passes (a fresh state per part, finalised with first numbers, selection taken to the host, state
closed), merges the P selections into a fresh state and finalises it.  Recorded per P: total time, time of every pass, merge +
finalise time, the largest `slots` any part reached and 32 B x slots beside what mem_get_info saw held, and that the result is
the one-shot scone_fit's keys, ids and counts.  A time is wall time between two device synchronises.

--gate-against DIR: also time the plain `stream, 2^20` route of THIS tree against a built checkout of the parent commit in DIR:
alternating fresh processes (each: corpus upload, a warm-up, --gate-runs timed runs), --gate-processes per side.  The new route
must be no slower than the parent's median plus the parent's own min-max spread in that run; both series go into the JSON.

Writes one JSON record (--out, default profiles/r15a/fit_partition.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N, MIN_FREQ, MAX_F = 3, 2, 5_000_000
CHUNK_TOKENS = 1 << 20
VOCAB, SEED = 50257, 21


def stream_pass(FitState, d_tok, d_off, tlen, texts_per_chunk, **part):
    """One pass over the resident corpus into a fresh state; the caller closes it."""
    n_texts = d_off.numel() - 1
    st = FitState(MAX_N)
    for a in range(0, n_texts, texts_per_chunk):
        b = min(n_texts, a + texts_per_chunk)
        lo, hi = a * tlen, b * tlen
        st.update(d_tok[lo:hi], d_off[a:b + 1] - lo, **part)
    return st


def worker(args):
    """The plain `stream, 2^20` route of the tree at --root, with nothing newer than FitState.update(tokens, offsets) and
    finalize(min_freq, max_f_grams): one JSON line with the timed runs."""
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    import scone_amd
    from scone_amd import _lib
    from scone_amd.hip_backend import FitState
    pkg = os.path.join(os.path.realpath(args.root), "scone_amd")
    assert os.path.realpath(os.path.dirname(scone_amd.__file__)) == pkg, scone_amd.__file__      # this tree's package ...
    assert os.path.realpath(_lib.LIB_PATH).startswith(pkg + os.sep), _lib.LIB_PATH               # ... and its own library
    tok = np.load(args.corpus)
    n_texts, tlen = tok.shape
    d_tok = torch.from_numpy(tok.reshape(-1)).cuda()
    d_off = (torch.arange(n_texts + 1, dtype=torch.int64) * tlen).cuda()
    tpc = max(1, CHUNK_TOKENS // tlen)
    runs, kept = [], None
    for rep in range(args.gate_runs + 1):                                # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = stream_pass(FitState, d_tok, d_off, tlen, tpc)
        res = st.finalize(MIN_FREQ, MAX_F)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st.close()
        kept = (int(len(res[1])), int(res[2].sum()), int(res[3]))
        if rep:
            runs.append(t1 - t0)
    print(json.dumps({"root": args.root, "total_s": runs, "f_grams_kept": kept[0], "sum_counts": kept[1], "n_distinct": kept[2]}))


def gate(args, corpus_path):
    sides = {"parent": os.path.abspath(args.gate_against), "new": HERE}
    series = {k: [] for k in sides}
    sig = {}
    for rep in range(args.gate_processes):
        for side, root in sides.items():                                 # alternating: parent, new, parent, new, ...
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--corpus", corpus_path,
                                   "--gate-runs", str(args.gate_runs)], capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                raise RuntimeError("gate worker of %s failed (%d):\n%s" % (side, done.returncode, done.stderr[-2000:]))
            rec = json.loads(done.stdout.strip().splitlines()[-1])
            series[side] += rec["total_s"]
            sig.setdefault(side, (rec["f_grams_kept"], rec["sum_counts"], rec["n_distinct"]))
            print("gate %-6s process %d: %s" % (side, rep, rec["total_s"]), flush=True)
    assert sig["parent"] == sig["new"], sig
    pm = statistics.median(series["parent"])
    spread = max(series["parent"]) - min(series["parent"])
    nm = statistics.median(series["new"])
    return {"route": "stream, 2^20 tokens per chunk, update + finalize, fresh process per sample group",
            "processes_per_side": args.gate_processes, "timed_runs_per_process": args.gate_runs,
            "parent_total_s": series["parent"], "new_total_s": series["new"], "parent_median_s": pm, "parent_spread_s": spread,
            "new_median_s": nm, "bound_s": pm + spread, "no_slower_than_parent": bool(nm <= pm + spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r15a", "fit_partition.json"))
    ap.add_argument("--texts", type=int, default=6000)
    ap.add_argument("--tlen", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--gate-against", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--gate-processes", type=int, default=3)
    ap.add_argument("--gate-runs", type=int, default=3)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--corpus", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from scone_amd import synthetic as S
    from scone_amd.hip_backend import FitState, fit_gpu, fit_occurrences
    assert torch.cuda.is_available(), "needs an MI355X: no time is ever taken on a CPU"
    n_texts, tlen = args.texts, args.tlen
    tok = S.stream_zipf(VOCAB, n_texts, tlen, SEED).astype(np.int32)
    d_tok = torch.from_numpy(tok.reshape(-1)).cuda()
    d_off = (torch.arange(n_texts + 1, dtype=torch.int64) * tlen).cuda()
    tpc = max(1, CHUNK_TOKENS // tlen)
    occ = fit_occurrences([tlen] * n_texts, MAX_N)

    def run(n_parts):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        if n_parts == 1:
            st = stream_pass(FitState, d_tok, d_off, tlen, tpc)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            held = free0 - torch.cuda.mem_get_info()[0]
            res = st.finalize(MIN_FREQ, MAX_F)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            stats = st.stats()
            st.close()
            assert stats["next_seq"] == occ
            return {"total_s": t2 - t0, "pass_s": [t2 - t0], "update_s": [t1 - t0], "merge_finalize_s": 0.0,
                    "max_slots": stats["slots"], "max_state_bytes": 32 * stats["slots"], "mem_get_info_held_bytes": held,
                    "part_n_distinct": [stats["n_distinct"]], "part_slots": [stats["slots"]], "selection_rows": len(res[1])}, res
        passes, updates, selections, slots, distinct, held = [], [], [], [], [], 0
        for p in range(n_parts):
            ta = time.perf_counter()
            st = stream_pass(FitState, d_tok, d_off, tlen, tpc, part=p, n_parts=n_parts)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            held = max(held, free0 - torch.cuda.mem_get_info()[0])
            k, l, c, _, f = st.finalize(MIN_FREQ, MAX_F, with_first=True)
            stats = st.stats()
            st.close()
            torch.cuda.synchronize()
            assert stats["next_seq"] == occ
            selections.append((k, l, c, f))
            slots.append(stats["slots"])
            distinct.append(stats["n_distinct"])
            updates.append(tb - ta)
            passes.append(time.perf_counter() - ta)
        tm = time.perf_counter()
        with FitState(MAX_N) as merged:
            for sel in selections:
                merged.merge(*sel)
            res = merged.finalize(MIN_FREQ, MAX_F)
            merged_slots = merged.stats()["slots"]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res = res[:3] + (sum(distinct),)
        return {"total_s": t2 - t0, "pass_s": passes, "update_s": updates, "merge_finalize_s": t2 - tm, "max_slots": max(slots),
                "max_state_bytes": 32 * max(slots), "mem_get_info_held_bytes": held, "part_n_distinct": distinct,
                "part_slots": slots, "merged_state_slots": merged_slots, "selection_rows": sum(len(s[1]) for s in selections)}, res

    record = {"corpus": {"texts": n_texts, "tokens_per_text": tlen, "tokens": n_texts * tlen, "occurrences": occ, "vocab": VOCAB,
                         "law": "iid Zipf(1.1), seed %d" % SEED},
              "fit": {"max_n": MAX_N, "min_freq": MIN_FREQ, "max_f_grams": MAX_F, "chunk_tokens": CHUNK_TOKENS},
              "device": torch.cuda.get_device_name(0), "mem_get_info_total_bytes": torch.cuda.mem_get_info()[1],
              "timing": "wall time between device synchronises, corpus resident, selections and result copied to the host; "
                        "repeats interleaved after one warm-up of every route", "partitions": {}}
    ref = fit_gpu(d_tok, d_off, MAX_N, MIN_FREQ, MAX_F)                  # the one-shot: the reference and a warm-up
    for n_parts in args.parts:
        run(n_parts)                                                     # warm-up: code objects, rocPRIM, allocator
    samples = {p: [] for p in args.parts}
    for rep in range(args.repeats):
        for n_parts in args.parts:
            s, res = run(n_parts)
            assert np.array_equal(res[0], ref[0]) and np.array_equal(res[1], ref[1]), n_parts           # keys, ids
            assert np.array_equal(res[2].astype(np.uint64), ref[2].astype(np.uint64)) and res[3] == ref[3], n_parts
            s["equals_one_shot_keys_ids_counts"] = True
            samples[n_parts].append(s)
            print("P = %d rep %d: %s" % (n_parts, rep, json.dumps(s)), flush=True)
            del res
    for n_parts, v in samples.items():
        tot = [s["total_s"] for s in v]
        per_pass = [t for s in v for t in s["pass_s"]]
        out = dict(v[-1])
        out["total_s"] = {"median": statistics.median(tot), "min": min(tot), "max": max(tot), "runs": tot}
        out["pass_s"] = {"median": statistics.median(per_pass), "min": min(per_pass), "max": max(per_pass),
                         "runs": [s["pass_s"] for s in v]}
        upd = [t for s in v for t in s["update_s"]]
        out["update_s"] = {"median": statistics.median(upd), "min": min(upd), "max": max(upd)}
        mf = [s["merge_finalize_s"] for s in v]
        out["merge_finalize_s"] = {"median": statistics.median(mf), "min": min(mf), "max": max(mf)}
        record["partitions"][str(n_parts)] = out
    record["f_grams_kept"] = int(len(ref[1]))
    record["n_distinct"] = int(ref[3])
    del d_tok, d_off
    torch.cuda.empty_cache()

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")

    write()
    print("ok: every P and repeat gave the one-shot's keys, ids and counts; wrote", args.out, flush=True)
    if args.gate_against:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "corpus.npy")
            np.save(path, tok)
            record["gate_plain_stream_vs_parent"] = gate(args, path)
        write()
    if args.gate_against and not record["gate_plain_stream_vs_parent"]["no_slower_than_parent"]:
        print("GATE MISSED: the plain stream route is slower than the parent's median + spread")
        sys.exit(1)


if __name__ == "__main__":
    main()
