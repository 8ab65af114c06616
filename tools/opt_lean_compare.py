#!/usr/bin/env python3
"""The lean optimizer step (`scone_opt_step_lean`) against the existing fused step (`scone_opt_step`), on the headline index:
1M rows, d = 768, max_n = 3.  The row sets are those of `backward_plan` over 4,096 (8 x 512), 65,536 (128 x 512) and
2048 x 512 tokens of the S_uniform stream; the gradient rows are what `BackwardPlan.rows` returns for a random
fp16 `grad_out`.

One process, HIP events around each call, the blocks alternating round by round, the warm-up calls of every block discarded;
per block the median of its steps, per arm the median of the block medians and their minimum and maximum.

  a  in place on a bf16 table, row-wise Adagrad, stochastic rounding      g 4 + row 2 + 2            =  8 B / element
  b  in place on a bf16 table, row-wise Adagrad, round to nearest         the same
  c  master mode, row-wise Adagrad, INT8 served table                     g 4 + master 4 + 4 + row 1 = 13 B / element
  d  scone_opt_step Adagrad on a bf16 table (the yardstick)               g 4 + master 4 + 4 + sum of squares 4 + 4 + row 2 = 22
  e  a 1 GiB device-to-device copy                                         read + written bytes over its time

Reported per arm: the bytes a step has to move (the row state and the INT8 scale included), that over the time, and the
same as a fraction of (e).  The bar: on the two larger row sets (a) must not be slower than (d) by more than (d)'s own spread
of block medians in this run (`a_within_d_spread`); the cost of the stochastic arm over the nearest one, a / b, is reported.

    python tools/opt_lean_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from opt_step_compare import D, MAX_N, N_ROWS, T, WORKLOADS, copy_rate_tbs, summary, timed  # noqa: E402

LR = 1e-3
ARMS = ("a_inplace_bf16_rowwise_stochastic", "b_inplace_bf16_rowwise_nearest", "c_master_int8_rowwise", "d_opt_step_adagrad_bf16")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19a", "opt_lean_compare.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6

    import torch
    from scone_amd import EmbeddingCache, NGramExtractor
    from scone_amd import synthetic as S
    keys, lens = S.make_keys(N_ROWS, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)

    def table_of(fmt):
        return EmbeddingCache.from_synthetic(ex, D, table_format=fmt, seed=7, base_scale=0.02 / 127)

    caches = {"ab": table_of("bf16"), "c": table_of("int8"), "d": table_of("bf16")}
    t_ab, t_c, t_d = (caches[k].table for k in ("ab", "c", "d"))
    copy_tbs = copy_rate_tbs()
    every = torch.arange(N_ROWS, device="cuda")
    master_c, master_d = t_c.gather_rows(every), t_d.gather_rows(every)        # the masters: the served rows, dequantised
    sumsq_d = torch.zeros_like(master_d)
    state_ab, state_c = torch.zeros(N_ROWS, device="cuda"), torch.zeros(N_ROWS, device="cuda")
    del every
    report = {"what": "call time in us, HIP events around each call; median_us is the median of the block medians, spread_us "
                      "their minimum and maximum; bytes_moved is what a step has to move, TBps that over median_us",
              "table": f"1M rows, d={D}, max_n={MAX_N}, row sets of S_uniform token batches; bf16 tables for a, b, d; int8 for c",
              "rounds": rounds, "steps": steps, "device_copy_TBps": copy_tbs, "workloads": {}}

    for name, B in WORKLOADS:
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
        g = torch.randn((B * T, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
        with t_c.backward_plan(tok) as plan:
            row_ids, grad_rows = plan.rows(g, "mean")
        torch.cuda.synchronize()
        del g
        U = int(row_ids.numel())
        step_no = [0]

        def arm_a():
            step_no[0] += 1
            t_ab.opt_step_lean(row_ids, grad_rows, kind="rowwise_adagrad", lr=LR, row_state=state_ab, rounding="stochastic", seed=1,
                               step=step_no[0])

        def arm_b():
            t_ab.opt_step_lean(row_ids, grad_rows, kind="rowwise_adagrad", lr=LR, row_state=state_ab)

        def arm_c():
            t_c.opt_step_lean(row_ids, grad_rows, kind="rowwise_adagrad", lr=LR, master=master_c, row_state=state_c)

        def arm_d():
            t_d.opt_step(row_ids, grad_rows, master_d, kind="adagrad", lr=LR, state2=sumsq_d)

        calls = dict(zip(ARMS, (arm_a, arm_b, arm_c, arm_d)))
        per_row = {ARMS[0]: D * 8 + 8, ARMS[1]: D * 8 + 8, ARMS[2]: D * 13 + 2 + 8, ARMS[3]: D * 22}
        blocks = {k: [] for k in calls}
        for _ in range(rounds):
            for k, call in calls.items():
                blocks[k].append(timed(call, steps))
        e = {"tokens": tok.numel(), "U": U}
        for k in ARMS:
            sm = summary(blocks[k])
            sm["bytes_moved"] = U * per_row[k]
            sm["TBps"] = sm["bytes_moved"] / (sm["median_us"] * 1e-6) / 1e12
            sm["fraction_of_copy_rate"] = sm["TBps"] / copy_tbs
            e[k] = sm
        a, b, d = e[ARMS[0]], e[ARMS[1]], e[ARMS[3]]
        e["a/d"] = a["median_us"] / d["median_us"]
        e["a/b"] = a["median_us"] / b["median_us"]
        e["d_spread_us"] = d["spread_us"][1] - d["spread_us"][0]
        e["a_within_d_spread"] = bool(a["median_us"] - d["median_us"] <= e["d_spread_us"])
        report["workloads"][name] = e
        del row_ids, grad_rows
        torch.cuda.empty_cache()
    for t in (t_ab, t_c, t_d):
        assert t.status() == 0
    report["bar_met_on_the_two_larger_row_sets"] = all(report["workloads"][n]["a_within_d_spread"] for n, _ in WORKLOADS[1:])
    text = json.dumps(report, indent=1)
    print(text)
    if out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
