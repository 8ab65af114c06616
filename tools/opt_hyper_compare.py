#!/usr/bin/env python3
"""Optimizer hyper-parameters on the device (include/scone_hip.h, "optimizer hyper-parameters on the device") against the by-value
steps, on the headline index: 1M rows, d = 768, max_n = 3, batches of 4,096 (8 x 512), 65,536 (128 x 512) and 2048 x 512 tokens
of the S_uniform stream, fp16 `grad_out`.  Two optimizers: Adam on the INT8 served table beside an fp32 master, and row-wise
Adagrad in place on bf16 rows with stochastic rounding -- the two that could not be captured before.

  (a) the region plan + rows + step, every step from an idle device: HIP-event time and HOST time until the last call returns,
      a_by_value   ctx.plan; ctx.rows; opt_step*(n=, lr=, step=...)                 today's static road, called eagerly
      b_dh_eager   ctx.plan; ctx.rows; opt_hyper_advance; opt_step*(n=, hyper=)      the capturable road, called eagerly
      c_dh_graph   road b captured once in a torch.cuda.graph and replayed (up to 2^20 possible references: 2048 x 512 is not
                   captured, see scone_backward_plan_dn in the header)
  (b) the step kernel alone on the same rows: opt_step*(n=, hyper=) against opt_step*(n=) by value, alternating blocks.  The only
      added device work is one uniform load of the block per wave: the _dh median is expected inside the _dn arm's own spread of
      block medians (recorded as `dh_inside_dn_spread`; nothing is asserted).
  (c) with --parent-lib: the UNTOUCHED scone_opt_step (SGD, Adam), scone_opt_step_dn (Adam) and scone_opt_step_lean (row-wise
      Adagrad, master mode) of this build against a library built from the parent commit, as alternating processes; reported
      against the parent's own spread of block medians.

Protocol (tools/backward_dn_compare.py's): blocks of the arms alternate round by round in one process, the warm-up steps of every
block are discarded; per block the median of its steps, per arm the median of the block medians and their minimum and maximum.

    python tools/opt_hyper_compare.py [out.json] [rounds] [steps] [--only=4096|65536|2048x512 ...] [--parent-lib PATH] [--procs K]
    python tools/opt_hyper_compare.py --plain-child [rounds] [steps]      (what (c) starts; SCONE_HIP_LIB selects the library)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.backward_dn_compare import CAPTURE_LIMIT_REFS, block  # noqa: E402
from tools.grad_clip_compare import D, LR, MAX_N, N_ROWS, T, WORKLOADS, row_set, setup, summary, timed  # noqa: E402

NEW_SYMBOLS = ("scone_opt_hyper_scalars_of", "scone_opt_hyper_init", "scone_opt_hyper_advance", "scone_opt_step_dh",
               "scone_opt_step_lean_dh", "scone_grad_ctl_set_dh")
PLAIN_CALLS = ("opt_step_sgd", "opt_step_adam", "opt_step_dn_adam", "opt_step_lean_rowwise")
OPTS = ("adam_int8_master", "rowwise_adagrad_bf16_inplace_stochastic")


def plain_child(rounds, steps):
    """The untouched steps of whatever library SCONE_HIP_LIB names (the parent's has none of the new symbols); one JSON line."""
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
        n = torch.tensor([row_ids.numel()], dtype=torch.int64, device="cuda")
        calls = {
            "opt_step_sgd": lambda: table.opt_step(row_ids, grad_rows, w, kind="sgd", lr=LR),
            "opt_step_adam": lambda: table.opt_step(row_ids, grad_rows, w, kind="adam", lr=LR, state1=m, state2=v, step=3),
            "opt_step_dn_adam": lambda: table.opt_step(row_ids, grad_rows, w, kind="adam", lr=LR, state1=m, state2=v, step=3, n=n),
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
    report = {"what": "block medians in us of every process of an arm, pooled; this build's median - the parent's median is held "
                      "against the parent's spread (max - min of its block medians)",
              "parent_lib": "a build of the parent commit, given by --parent-lib", "processes_per_arm": procs, "rounds": rounds,
              "steps": steps, "workloads": {}}
    for name, _ in WORKLOADS:
        e = {"U": runs["parent"][0]["workloads"][name]["U"]}
        for call in PLAIN_CALLS:
            p = summary(np.concatenate([r["workloads"][name][call] for r in runs["parent"]]))
            t = summary(np.concatenate([r["workloads"][name][call] for r in runs["this_build"]]))
            e[call] = {"parent": p, "this_build": t, "this_build/parent": t["median_us"] / p["median_us"],
                       "within_parent_spread": bool(t["median_us"] - p["median_us"] <= p["spread_us"][1] - p["spread_us"][0])}
        report["workloads"][name] = e
    return report


def main():
    args = sys.argv[1:]
    if args and args[0] == "--plain-child":
        return plain_child(int(args[1]) if len(args) > 1 else 5, int(args[2]) if len(args) > 2 else 6)
    parent_lib, procs = None, 2
    for flag in ("--parent-lib", "--procs"):
        if flag in args:
            i = args.index(flag)
            value = args[i + 1]
            del args[i:i + 2]
            if flag == "--parent-lib":
                parent_lib = value
            else:
                procs = int(value)
    only = [a.split("=", 1)[1] for a in args if a.startswith("--only=")]
    args = [a for a in args if not a.startswith("--")]
    out_path = args[0] if args else None
    rounds = int(args[1]) if len(args) > 1 else 5
    steps = int(args[2]) if len(args) > 2 else 8
    result = {"what": "times in us; median_us is the median of the block medians, spread_us their minimum and maximum",
              "n_rows": N_ROWS, "d": D, "max_n": MAX_N, "rounds": rounds, "steps": steps, "workloads": {}}
    # (c) first: the alternating processes run while this one holds no device memory
    result["untouched_steps_against_the_parent"] = (plain_against_parent(parent_lib, procs, rounds, steps) if parent_lib
                                                    else "not measured (no --parent-lib)")
    import torch
    from scone_amd import EmbeddingCache, NGramExtractor
    from scone_amd import synthetic as S
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    result["device"] = torch.cuda.get_device_name(0)
    keys, lens, cache, w = setup()
    bf16 = EmbeddingCache.from_synthetic(NGramExtractor.from_arrays(keys, lens, max_n=MAX_N), D, table_format="bf16", seed=7,
                                         base_scale=0.02)
    tables = {OPTS[0]: cache.table, OPTS[1]: bf16.table}
    m, v, s = torch.zeros_like(w), torch.zeros_like(w), torch.zeros(N_ROWS, device="cuda")
    hp = dict(lr=LR, weight_decay=0.01)
    for name, B in WORKLOADS:
        if only and name not in only:
            continue
        ntok = B * T
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
        g = torch.randn((ntok, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
        entry = {"tokens": ntok}
        for opt in OPTS:
            table = tables[opt]
            adam = opt == OPTS[0]
            with table.backward_plan(tok) as plan:
                U = plan.n_rows
            cap = U + 64
            ids = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
            rows = torch.full((cap, D), float("nan"), dtype=torch.float32, device="cuda")
            n = torch.zeros(1, dtype=torch.int64, device="cuda")
            ctx = table.backward_context(ntok)
            hy = table.opt_hyper(seed=5, eps=1e-8 if adam else 1e-10, **hp)
            t_host = [0]

            def step_value():
                t_host[0] += 1
                if adam:
                    table.opt_step(ids, rows, w, kind="adam", state1=m, state2=v, step=t_host[0], n=n, **hp)
                else:
                    table.opt_step_lean(ids, rows, kind="rowwise_adagrad", row_state=s, rounding="stochastic", seed=5, step=t_host[0],
                                        n=n, **hp)

            def step_hyper():
                if adam:
                    table.opt_step(ids, rows, w, kind="adam", state1=m, state2=v, n=n, hyper=hy)
                else:
                    table.opt_step_lean(ids, rows, kind="rowwise_adagrad", row_state=s, rounding="stochastic", n=n, hyper=hy)

            def road_a():
                ctx.plan(tok)
                ctx.rows(g, "mean", out=(ids, rows, n))
                step_value()

            def road_b():
                ctx.plan(tok)
                ctx.rows(g, "mean", out=(ids, rows, n))
                table.opt_hyper_advance(hy, "adam" if adam else "sgd")
                step_hyper()

            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                road_b()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            assert int(n.item()) == U and int(hy.step.item()) == 1
            calls = {"a_by_value": road_a, "b_dh_eager": road_b}
            graph = None
            if ntok * (MAX_N * (MAX_N + 1) // 2) <= CAPTURE_LIMIT_REFS:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    road_b()
                calls["c_dh_graph"] = graph.replay
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for _ in range(rounds):
                for k in calls:
                    d_us, h_us = block(calls[k], steps)
                    dev[k].append(d_us)
                    host[k].append(h_us)
            e = {"U": U, "event_us": {k: summary(dev[k]) for k in calls}, "host_us": {k: summary(host[k]) for k in calls}}
            if graph is None:
                e["c_dh_graph"] = "not captured: above 2^20 possible references scone_backward_plan_dn refuses a capturing stream"
            # (b) the step kernel alone, the same rows
            table.opt_hyper_advance(hy, "adam" if adam else "sgd")
            kernels = {"dn_by_value": step_value, "dh": step_hyper}
            kb = {k: [] for k in kernels}
            for _ in range(rounds):
                for k in kernels:
                    kb[k].append(timed(kernels[k], steps))
            dn, dh = summary(kb["dn_by_value"]), summary(kb["dh"])
            e["step_kernel_us"] = {"dn_by_value": dn, "dh": dh, "dh/dn": dh["median_us"] / dn["median_us"],
                                   "dh_inside_dn_spread": bool(dn["spread_us"][0] <= dh["median_us"] <= dn["spread_us"][1])}
            torch.cuda.synchronize()
            assert hy.read()["bad"] == 0 and table.status() == 0
            entry[opt] = e
            print(name, opt, json.dumps(e), flush=True)
            ctx.close()
            del graph, ids, rows
            torch.cuda.empty_cache()
        result["workloads"][name] = entry
        del tok, g
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
