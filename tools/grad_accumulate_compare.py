#!/usr/bin/env python3
"""Gradient accumulation over micro-batches on the device (`scone_grad_merge_map`, `scone_grad_merge_rows`,
`scone_backward_rows_acc`; include/scone_hip.h, "gradient accumulation") on the headline index: 1M-row INT8 served table, d = 768,
max_n = 3.  Two micro-batches of DIFFERENT tokens of the S_uniform stream, each of 4,096 (8 x 512), 65,536 (128 x 512) or
2048 x 512 tokens: the gradient of the first is there (`old`), the second's backward adds to it.  Three arms make the same
sparse gradient (asserted bit for bit before anything is timed), each from the second micro-batch's plan and fp16 `grad_out`:

  a_rows_add_coalesced   plan.rows(), then training._add_coalesced(old, new): the road of the parent commit
  b_rows_grad_merge      plan.rows(), then SconeTable.grad_merge(old, new)
  c_rows_accumulate      plan.rows(accumulate=old): the new rows are never stored

HIP events around each call, the blocks of the arms alternating round by round, the warm-up calls of every block discarded; per
block the median of its steps, per arm the median of the block medians and their minimum and maximum.  Per arm also the peak of
`torch.cuda.max_memory_allocated` over one call, above what was allocated before it (old and grad_out are there before; the
result is part of the peak).  For b and c: the bytes the arm must move -- grad_out once, the new rows written and read back (b
only), old read, the union written -- over its time, as a fraction of the device-copy rate of this process (a 1 GiB
device-to-device copy, read + written bytes over its time).

With --parent-lib: the PLAIN scone_backward_rows of this build against the parent commit's library, as alternating processes
(--procs per arm) on this box.  Bar: this build's median is above the parent's by no more than the parent's own spread of block
medians.

    python tools/grad_accumulate_compare.py [out.json] [rounds] [steps] [--parent-lib PATH] [--procs K]
    python tools/grad_accumulate_compare.py --plain-child [rounds] [steps]      (what --parent-lib starts; SCONE_HIP_LIB selects the library)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.grad_clip_compare import D, MAX_N, N_ROWS, T, WORKLOADS, copy_rate_tbs, summary, timed  # noqa: E402

NEW_SYMBOLS = ("scone_grad_merge_scratch", "scone_grad_merge_map", "scone_grad_merge_rows", "scone_backward_row_ids",
               "scone_backward_rows_acc")
SEEDS = (1234, 4321)          # the token streams of the two micro-batches


def setup():
    from scone_amd import EmbeddingCache, NGramExtractor
    from scone_amd import synthetic as S
    keys, lens = S.make_keys(N_ROWS, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="int8", seed=7, base_scale=0.02 / 127)
    return keys, lens, cache


def micro_batch(keys, lens, B, seed):
    import torch
    from scone_amd import synthetic as S
    tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, seed)).to("cuda", torch.int32)
    g = torch.randn((B * T, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B + seed)).half()
    return tok, g


def plain_child(rounds, steps):
    """plan.rows() of whatever library SCONE_HIP_LIB names (the parent's has none of the new symbols); one JSON line."""
    import ctypes
    from scone_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        if not hasattr(have, name):
            _lib.SIGNATURES.pop(name)
    import torch
    keys, lens, cache = setup()
    table = cache.table
    out = {"lib": _lib.LIB_PATH, "workloads": {}}
    for name, B in WORKLOADS:
        tok, g = micro_batch(keys, lens, B, SEEDS[1])
        with table.backward_plan(tok) as plan:
            bufs = (torch.empty(plan.n_rows, dtype=torch.int64, device="cuda"), torch.empty((plan.n_rows, D), device="cuda"))
            blocks = [timed(lambda: plan.rows(g, "mean", out=bufs), steps) for _ in range(rounds)]
            out["workloads"][name] = {"U": plan.n_rows, "backward_rows": blocks}
        del bufs, tok, g
        torch.cuda.empty_cache()
    assert table.status() == 0
    print("PLAIN " + json.dumps(out))


def plain_against_parent(parent_lib, procs, rounds, steps):
    import numpy as np
    arms = {"parent": os.path.abspath(parent_lib), "this_build": None}
    runs = {k: [] for k in arms}
    for _ in range(procs):
        for arm, path in arms.items():                                      # alternating processes
            env = dict(os.environ)
            env.pop("SCONE_HIP_LIB", None)
            if path:
                env["SCONE_HIP_LIB"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", str(rounds), str(steps)], env=env,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"the {arm} process failed ({r.returncode}): {r.stderr[-2000:]}")
            line = [x for x in r.stdout.splitlines() if x.startswith("PLAIN ")][-1]
            runs[arm].append(json.loads(line[6:]))
            print(f"plain backward_rows: a {arm} process done", file=sys.stderr, flush=True)
    report = {"what": "block medians in us of every process of an arm, pooled; bar: this build's median - the parent's median <= "
                      "the parent's spread (max - min of its block medians)",
              "parent_lib": "a build of the parent commit, given by --parent-lib", "processes_per_arm": procs, "rounds": rounds,
              "steps": steps, "workloads": {}}
    ok = True
    for name, _ in WORKLOADS:
        p = summary(np.concatenate([r["workloads"][name]["backward_rows"] for r in runs["parent"]]))
        t = summary(np.concatenate([r["workloads"][name]["backward_rows"] for r in runs["this_build"]]))
        within = bool(t["median_us"] - p["median_us"] <= p["spread_us"][1] - p["spread_us"][0])
        ok = ok and within
        report["workloads"][name] = {"U": runs["parent"][0]["workloads"][name]["U"], "parent": p, "this_build": t,
                                     "this_build/parent": t["median_us"] / p["median_us"], "within_parent_spread": within}
    report["backward_rows_within_the_parent_spread"] = ok
    return report


def peak_bytes(call):
    """max_memory_allocated over one call, above what was allocated before it."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    result = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del result
    return int(peak)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--plain-child":
        return plain_child(int(args[1]) if len(args) > 1 else 5, int(args[2]) if len(args) > 2 else 6)
    parent_lib, procs = None, 3
    for flag in ("--parent-lib", "--procs"):
        if flag in args:
            i = args.index(flag)
            value = args[i + 1]
            del args[i:i + 2]
            if flag == "--parent-lib":
                parent_lib = value
            else:
                procs = int(value)
    out_path = args[0] if len(args) > 0 else None
    rounds = int(args[1]) if len(args) > 1 else 5
    steps = int(args[2]) if len(args) > 2 else 6

    report = {"what": "call time in us, HIP events around each call; median_us is the median of the block medians, spread_us "
                      "their minimum and maximum; peak_bytes: torch.cuda.max_memory_allocated over one call above what was "
                      "allocated before it",
              "table": f"1M-row int8 served table, d={D}, max_n={MAX_N}; two micro-batches of different S_uniform tokens, fp16 grad_out",
              "rounds": rounds, "steps": steps, "workloads": {}}
    if parent_lib:                     # first: the alternating processes run while this one holds no device memory
        report["backward_rows_against_the_parent"] = plain_against_parent(parent_lib, procs, rounds, steps)
    else:
        report["backward_rows_against_the_parent"] = "not measured (no --parent-lib)"

    import numpy as np
    import torch
    from scone_amd.training import _add_coalesced
    keys, lens, cache = setup()
    table = cache.table
    copy_tbs = report["device_copy_TBps"] = copy_rate_tbs()
    for name, B in WORKLOADS:
        tok1, g1 = micro_batch(keys, lens, B, SEEDS[0])
        with table.backward_plan(tok1) as plan1:
            old_ids, old_rows = plan1.rows(g1, "mean")
        del tok1, g1
        old_sparse = torch.sparse_coo_tensor(old_ids[None], old_rows, (N_ROWS, D), is_coalesced=True)
        tok2, g2 = micro_batch(keys, lens, B, SEEDS[1])
        with table.backward_plan(tok2) as plan:

            def arm_a():
                return _add_coalesced(old_sparse, *plan.rows(g2, "mean"))

            def arm_b():
                return table.grad_merge(old_ids, old_rows, *plan.rows(g2, "mean"))

            def arm_c():
                return plan.rows(g2, "mean", accumulate=(old_ids, old_rows))

            calls = {"a_rows_add_coalesced": arm_a, "b_rows_grad_merge": arm_b, "c_rows_accumulate": arm_c}
            # agreement before anything is timed
            ra, rb, rc = arm_a(), arm_b(), arm_c()
            assert torch.equal(ra._indices()[0], rb[0]) and torch.equal(rb[0], rc[0])
            assert torch.equal(ra._values().view(torch.int32), rb[1].view(torch.int32)), "b differs from a"
            assert torch.equal(rb[1].view(torch.int32), rc[1].view(torch.int32)), "c differs from b"
            U_old, U_new, U_out = int(old_ids.numel()), plan.n_rows, int(rb[0].numel())
            del ra, rb, rc
            e = {"tokens_per_micro_batch": int(tok2.numel()), "U_old": U_old, "U_new": U_new, "U_out": U_out,
                 "row_bytes_U_out": 4 * D * U_out}
            blocks = {k: [] for k in calls}
            for _ in range(rounds):
                for k, call in calls.items():
                    blocks[k].append(timed(call, steps))
            grad_out_bytes = 2 * D * int(tok2.numel())
            must = {"b_rows_grad_merge": grad_out_bytes + 4 * D * (2 * U_new + U_old + U_out),
                    "c_rows_accumulate": grad_out_bytes + 4 * D * (U_old + U_out)}
            for k, call in calls.items():
                s = summary(blocks[k])
                s["peak_bytes"] = peak_bytes(call)
                if k in must:
                    tbs = must[k] / (s["median_us"] * 1e-6) / 1e12
                    s["bytes_it_must_move"], s["TBps"], s["fraction_of_copy_rate"] = must[k], tbs, tbs / copy_tbs
                e[k] = s
            a, b, c = (e[k] for k in calls)
            a_spread = a["spread_us"][1] - a["spread_us"][0]
            e["b/a"], e["c/a"], e["c/b"] = b["median_us"] / a["median_us"], c["median_us"] / a["median_us"], c["median_us"] / b["median_us"]
            e["b_below_a_beyond_a_spread"] = bool(a["median_us"] - b["median_us"] > a_spread)
            e["c_below_a_beyond_a_spread"] = bool(a["median_us"] - c["median_us"] > a_spread)
            e["peak_b_minus_c_in_U_new_arrays"] = (b["peak_bytes"] - c["peak_bytes"]) / float(4 * D * max(U_new, 1))
        report["workloads"][name] = e
        print(f"workload {name} done", file=sys.stderr, flush=True)
        del old_sparse, old_ids, old_rows, tok2, g2
        torch.cuda.empty_cache()
    assert table.status() == 0
    assert np.isfinite(copy_tbs)
    text = json.dumps(report, indent=1)
    print(text)
    if out_path and out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
