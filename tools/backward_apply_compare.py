#!/usr/bin/env python3
"""The backward applied in place (`scone_backward_apply_lean`) against the two calls it fuses (`scone_backward_rows`, then
`scone_opt_step_lean`), on the headline index: 1M rows, d = 768, max_n = 3, an in-place bf16 table, row-wise Adagrad with
stochastic rounding, fp16 `grad_out`.  The batches are those of DESIGN 4.4c: 4,096 (8 x 512), 65,536 (128 x 512) and 2048 x 512
tokens of the S_uniform stream.

One process, one table, ONE plan per batch shared by both arms, HIP events around each region, the blocks alternating round by
round, the warm-up calls of every block discarded; per block the median of its steps, per arm the median of the block medians
and their minimum and maximum.

  a  scone_backward_apply_lean                                   per touched element: row 2 + 2                  =  4 B
  b  scone_backward_rows + scone_opt_step_lean, ONE timed region  per touched element: grad_rows 4 + 4, row 2 + 2 = 12 B
  e  a 1 GiB device-to-device copy                                 read + written bytes over its time

Both arms also read `grad_out` once per reference (2 B per element) and move the row state (8 B per row); (b) writes and reads
the row ids (16 B per row) and writes into buffers allocated before the timing.  The partial slots of rows with several chunks
are written and read by both arms and are not counted.  Reported per arm: those bytes, that over the time, and the same as a
fraction of (e).  The bar: on the two larger batches (a) must not be slower than (b) by more than (b)'s own spread of block
medians in this run (`a_within_b_spread`).  The gain, a / b, is whatever is measured.

    python tools/backward_apply_compare.py [out.json] [rounds] [steps]

Without `out.json` the report goes to `backward_apply_compare.json` in the next free `profiles/rNNa/` directory.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from opt_step_compare import D, MAX_N, N_ROWS, T, WORKLOADS, copy_rate_tbs, summary, timed  # noqa: E402

LR = 1e-3
ARMS = ("a_backward_apply_lean", "b_backward_rows_then_opt_step_lean")


def next_profile_dir():
    taken = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)a", n) for n in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(taken, default=0) + 1:02d}a")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(next_profile_dir(), "backward_apply_compare.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6

    import torch
    from scone_amd import EmbeddingCache, NGramExtractor
    from scone_amd import synthetic as S
    keys, lens = S.make_keys(N_ROWS, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)
    table = EmbeddingCache.from_synthetic(ex, D, table_format="bf16", seed=7, base_scale=0.02 / 127).table
    copy_tbs = copy_rate_tbs()
    state = torch.zeros(N_ROWS, device="cuda")
    report = {"what": "region time in us, HIP events around each region; median_us is the median of the block medians, spread_us "
                      "their minimum and maximum; bytes_moved is what a region has to move, TBps that over median_us",
              "table": f"1M rows, d={D}, max_n={MAX_N}, bf16 in place, row-wise Adagrad, stochastic rounding; fp16 grad_out of "
                       "S_uniform token batches; one plan per batch shared by both arms",
              "rounds": rounds, "steps": steps, "device_copy_TBps": copy_tbs, "workloads": {}}

    for name, B in WORKLOADS:
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
        g = torch.randn((B * T, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
        with table.backward_plan(tok) as plan:
            U, refs = plan.n_rows, plan.n_refs
            ids_buf = torch.empty(U, dtype=torch.int64, device="cuda")
            rows_buf = torch.empty((U, D), dtype=torch.float32, device="cuda")
            step_no = [0]
            hp = dict(kind="rowwise_adagrad", lr=LR, row_state=state, rounding="stochastic", seed=1)

            def arm_a():
                step_no[0] += 1
                plan.apply_lean(g, "mean", step=step_no[0], **hp)

            def arm_b():
                step_no[0] += 1
                row_ids, grad_rows = plan.rows(g, "mean", out=(ids_buf, rows_buf))
                table.opt_step_lean(row_ids, grad_rows, step=step_no[0], **hp)

            calls = dict(zip(ARMS, (arm_a, arm_b)))
            shared = refs * D * 2 + U * 8
            moved = {ARMS[0]: shared + U * D * 4, ARMS[1]: shared + U * D * 12 + U * 16}
            blocks = {k: [] for k in calls}
            for _ in range(rounds):
                for k, call in calls.items():
                    blocks[k].append(timed(call, steps))
        e = {"tokens": tok.numel(), "U": U, "references": refs, "grad_rows_bytes_not_stored": U * D * 4}
        for k in ARMS:
            sm = summary(blocks[k])
            sm["bytes_moved"] = moved[k]
            sm["TBps"] = sm["bytes_moved"] / (sm["median_us"] * 1e-6) / 1e12
            sm["fraction_of_copy_rate"] = sm["TBps"] / copy_tbs
            e[k] = sm
        a, b = e[ARMS[0]], e[ARMS[1]]
        e["a/b"] = a["median_us"] / b["median_us"]
        e["b_spread_us"] = b["spread_us"][1] - b["spread_us"][0]
        e["a_within_b_spread"] = bool(a["median_us"] - b["median_us"] <= e["b_spread_us"])
        report["workloads"][name] = e
        del g, ids_buf, rows_buf
        torch.cuda.empty_cache()
    assert table.status() == 0
    report["bar_met_on_the_two_larger_row_sets"] = all(report["workloads"][n]["a_within_b_spread"] for n, _ in WORKLOADS[1:])
    text = json.dumps(report, indent=1)
    print(text)
    if out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
