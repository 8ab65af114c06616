#!/usr/bin/env python3
"""Clipping by the global gradient norm on the device (`scone_grad_sqnorm`, `scone_grad_ctl_set`, the `_ctl` optimizer steps;
include/scone_hip.h, "gradient norm, clipping and skipped steps") on the headline index: 1M-row INT8 served table, d = 768, fp32
master, max_n = 3.  The row sets are those of `backward_plan` over 4,096 (8 x 512), 65,536 (128 x 512) and 2048 x 512 tokens of
the S_uniform stream; the gradient rows are what `BackwardPlan.rows` returns for a random fp16 `grad_out`.

HIP events around each call, the blocks of the arms alternating round by round, the warm-up calls of every block discarded; per
block the median of its steps, per arm the median of the block medians and their minimum and maximum.  Three things are recorded.

  1. sqnorm        `SconeTable.grad_sqnorm` alone (three launches): its time, and the 4 * U * d bytes it reads over that time as a
                   fraction of the device-copy rate of this process (a 1 GiB device-to-device copy, read + written bytes over
                   its time).
  2. the clipped step by two roads, SGD and Adam.  Their bits differ by construction (the stock road rounds g * coef, then
     * grad_scale; the norm is summed in another order): only time is compared.
       new_<kind>    FGramOptimizer.step(max_norm=): grad_sqnorm, grad_ctl, the _ctl step; no synchronise
       stock_<kind>  torch.linalg.vector_norm(grad_rows), clamp(max_norm / (norm + 1e-6), max=1), grad_rows.mul_(coef), then the
                     plain FGramOptimizer.step(); no .item() either.  (The gradient is restored from a copy before every
                     block, outside the timed region.)
  3. with --parent-lib: the PLAIN scone_opt_step (SGD, Adam) and scone_opt_step_lean (row-wise Adagrad, master mode) of this build
     against the parent commit's library, as alternating processes (--procs per arm) on this box.  Bar: this build's median is
     above the parent's by no more than the parent's own spread of block medians.

    python tools/grad_clip_compare.py [out.json] [rounds] [steps] [--parent-lib PATH] [--procs K]
    python tools/grad_clip_compare.py --plain-child [rounds] [steps]      (what 3. starts; SCONE_HIP_LIB selects the library)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_N, D, N_ROWS, T = 3, 768, 1_000_000, 512
WORKLOADS = (("4096", 8), ("65536", 128), ("2048x512", 2048))
LR = 1e-3
NEW_SYMBOLS = ("scone_grad_sqnorm_scratch", "scone_grad_sqnorm", "scone_grad_ctl_set", "scone_opt_step_ctl", "scone_opt_step_lean_ctl")


def timed(call, steps, warm=2, before=None):
    import numpy as np
    import torch
    if before is not None:
        before()
    for _ in range(warm):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))


def summary(v):
    import numpy as np
    return {"median_us": float(np.median(v)), "spread_us": [float(np.min(v)), float(np.max(v))], "blocks": len(v)}


def copy_rate_tbs():
    import torch
    n = 1 << 30
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    us = [timed(lambda: dst.copy_(src), 4) for _ in range(5)]
    del src, dst
    torch.cuda.empty_cache()
    return 2 * n / (sorted(us)[2] * 1e-6) / 1e12


def setup():
    import torch
    from scone_amd import EmbeddingCache, NGramExtractor
    from scone_amd import synthetic as S
    keys, lens = S.make_keys(N_ROWS, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="int8", seed=7, base_scale=0.02 / 127)
    w0 = cache.table.gather_rows(torch.arange(N_ROWS, device="cuda"))          # the master: the served rows, dequantised
    return keys, lens, cache, w0


def row_set(table, keys, lens, B):
    import torch
    from scone_amd import synthetic as S
    tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
    g = torch.randn((B * T, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
    with table.backward_plan(tok) as plan:
        row_ids, grad_rows = plan.rows(g, "mean")
    torch.cuda.synchronize()
    return tok.numel(), row_ids, grad_rows


def plain_child(rounds, steps):
    """The plain steps of whatever library SCONE_HIP_LIB names (the parent's has none of the new symbols); one JSON line."""
    import ctypes
    from scone_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        if not hasattr(have, name):
            _lib.SIGNATURES.pop(name)
    import torch
    keys, lens, cache, w0 = setup()
    table = cache.table
    w, m, v, s = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0), torch.zeros(N_ROWS, device="cuda")
    out = {"lib": _lib.LIB_PATH, "workloads": {}}
    for name, B in WORKLOADS:
        _, row_ids, grad_rows = row_set(table, keys, lens, B)
        calls = {
            "opt_step_sgd": lambda: table.opt_step(row_ids, grad_rows, w, kind="sgd", lr=LR),
            "opt_step_adam": lambda: table.opt_step(row_ids, grad_rows, w, kind="adam", lr=LR, state1=m, state2=v, step=3),
            "opt_step_lean_rowwise": lambda: table.opt_step_lean(row_ids, grad_rows, kind="rowwise_adagrad", lr=LR, master=w, row_state=s),
        }
        blocks = {k: [] for k in calls}
        for _ in range(rounds):
            for k, call in calls.items():
                blocks[k].append(timed(call, steps))
        out["workloads"][name] = {"U": int(row_ids.numel()), **blocks}
        del row_ids, grad_rows
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
            print(f"plain steps: a {arm} process done", file=sys.stderr, flush=True)
    report = {"what": "block medians in us of every process of an arm, pooled; bar: this build's median - the parent's median <= "
                      "the parent's spread (max - min of its block medians)",
              "parent_lib": "a build of the parent commit, given by --parent-lib", "processes_per_arm": procs, "rounds": rounds, "steps": steps, "workloads": {}}
    ok = True
    for name, _ in WORKLOADS:
        e = {"U": runs["parent"][0]["workloads"][name]["U"]}
        for call in ("opt_step_sgd", "opt_step_adam", "opt_step_lean_rowwise"):
            p = summary(np.concatenate([r["workloads"][name][call] for r in runs["parent"]]))
            t = summary(np.concatenate([r["workloads"][name][call] for r in runs["this_build"]]))
            within = bool(t["median_us"] - p["median_us"] <= p["spread_us"][1] - p["spread_us"][0])
            ok = ok and within
            e[call] = {"parent": p, "this_build": t, "this_build/parent": t["median_us"] / p["median_us"], "within_parent_spread": within}
        report["workloads"][name] = e
    report["plain_calls_within_the_parent_spread"] = ok
    return report


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
                      "their minimum and maximum",
              "table": f"1M-row int8 served table, d={D}, fp32 master, max_n={MAX_N}, row sets of S_uniform token batches",
              "rounds": rounds, "steps": steps, "workloads": {}}
    # 3. first: the alternating processes run while this one holds no device memory
    if parent_lib:
        report["plain_steps_against_the_parent"] = plain_against_parent(parent_lib, procs, rounds, steps)
    else:
        report["plain_steps_against_the_parent"] = "not measured (no --parent-lib)"

    import torch
    from scone_amd import FGramOptimizer, TrainableFGramTable
    keys, lens, cache, w0 = setup()
    table = cache.table
    copy_tbs = report["device_copy_TBps"] = copy_rate_tbs()
    for name, B in WORKLOADS:
        tokens, row_ids, grad_rows = row_set(table, keys, lens, B)
        U = int(row_ids.numel())
        e = {"tokens": tokens, "U": U}
        # 1. the norm alone
        scratch = torch.empty(U + (U + 1023) // 1024, dtype=torch.float64, device="cuda")
        sq, _ = table.grad_sqnorm(grad_rows, scratch=scratch)
        ref = float(torch.linalg.vector_norm(grad_rows.double()) ** 2)
        assert abs(float(sq) - ref) <= 1e-10 * ref, (float(sq), ref)
        norm = float(sq) ** 0.5
        sq_blocks = []
        # 2. the two roads; max_norm is half the norm: every step is clipped
        work = grad_rows.clone()
        sparse = torch.sparse_coo_tensor(row_ids[None], work, (N_ROWS, D), is_coalesced=True)
        max_norm = 0.5 * norm
        blocks = {}
        for kind in ("sgd", "adam"):
            new = TrainableFGramTable(cache, w0.clone())
            stock = TrainableFGramTable(cache, w0.clone())
            nopt, sopt = FGramOptimizer(new, kind, lr=LR), FGramOptimizer(stock, kind, lr=LR)
            new.weight.grad = stock.weight.grad = sparse

            def new_step():
                nopt.step(max_norm=max_norm)

            def stock_step():
                total = torch.linalg.vector_norm(work)
                coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
                work.mul_(coef)
                sopt.step()

            def restore():
                work.copy_(grad_rows)

            # agreement before anything is timed: the same step but for roundings in another order
            restore()
            new_step()
            stock_step()
            restore()
            a, b = new.weight.detach()[row_ids], stock.weight.detach()[row_ids]
            diff, scale = float((a - b).abs().max()), float(b.abs().max())
            assert diff <= 1e-5 * max(scale, 1.0), (kind, diff, scale)
            coef = float(nopt.last_ctl.read()["coef"])
            assert abs(coef - 0.5) < 1e-3 and not nopt.found_nonfinite(), coef
            calls = {f"new_{kind}": new_step, f"stock_{kind}": stock_step}
            for k in calls:
                blocks[k] = []
            for _ in range(rounds):
                sq_blocks.append(timed(lambda: table.grad_sqnorm(grad_rows, scratch=scratch), steps))
                for k, call in calls.items():
                    blocks[k].append(timed(call, steps, before=restore))
            n_, s_ = summary(blocks[f"new_{kind}"]), summary(blocks[f"stock_{kind}"])
            e[f"new_{kind}"], e[f"stock_{kind}"] = n_, s_
            e[f"new_{kind}/stock_{kind}"] = n_["median_us"] / s_["median_us"]
            e[f"new_{kind}_beats_stock_beyond_its_spread"] = bool(s_["median_us"] - n_["median_us"] > s_["spread_us"][1] - s_["spread_us"][0])
            e[f"{kind}_max_abs_diff_vs_stock_after_one_step"] = diff
            del new, stock, nopt, sopt
            torch.cuda.empty_cache()
        q = summary(sq_blocks)
        tbs = 4 * U * D / (q["median_us"] * 1e-6) / 1e12
        e["sqnorm"] = q
        e["sqnorm_bytes_read"] = 4 * U * D
        e["sqnorm_TBps"] = tbs
        e["sqnorm_fraction_of_copy_rate"] = tbs / copy_tbs
        report["workloads"][name] = e
        print(f"workload {name} done", file=sys.stderr, flush=True)
        del sparse, work, row_ids, grad_rows, scratch
        torch.cuda.empty_cache()
    assert table.status() == 0
    text = json.dumps(report, indent=1)
    print(text)
    if out_path and out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
