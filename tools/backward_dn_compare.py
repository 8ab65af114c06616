#!/usr/bin/env python3
"""Backward + optimizer step with the counts on the device (include/scone_hip.h, "backward and optimizer step without a host
synchronisation") against today's road, on the headline index: 1M-row INT8 served table, d = 768, max_n = 3, fp32 master, SGD.
Batches of 4,096 (8 x 512), 65,536 (128 x 512) and 2048 x 512 tokens of the S_uniform stream, fp16 `grad_out`.  The region is
backward + step: plan, rows, optimizer step.  Three roads leave the same master and table (the rows and the count are asserted
bit for bit against road a before anything is timed):

  a_by_value   table.backward_plan(tok); plan.rows(g, out=); table.opt_step(ids, rows, w); plan.close()      today's road
  b_dn_eager   ctx.plan(tok); ctx.rows(g, out=(ids, rows, n)); table.opt_step(ids, rows, w, n=n)             called eagerly
  c_dn_graph   road b captured once in a torch.cuda.graph and replayed (batches of up to 2^20 possible references: the library
               refuses to capture a larger plan, see scone_backward_plan_dn in the header)

Every step starts on an idle device (a synchronise before it, outside the timed window) and records two numbers: the time
between HIP events around the region, and the HOST time from the first call until the last call has returned -- what the
sync-free form is for: on road a the host waits for the plan's readback inside the region, on b and c it only enqueues.  The
blocks of the three roads alternate round by round in one process, the warm-up steps of every block are discarded; per block the
median of its steps, per road the median of the block medians and their minimum and maximum.  Nothing here is a bar: the `_dn`
road sorts and scans the worst-case reference count of the batch, exactly as today's road does, and walks its device counts over
grids sized from bounds.

Memory: `ctx.nbytes` (the library's own figure) beside what a live plan of today's road holds (free device memory with the plan
alive against the plan closed) and the transient peak of its build computed from the same buffer sizes (rocPRIM's scratch left
out: the library does not report it).

    python tools/backward_dn_compare.py [out.json] [rounds] [steps] [--only=4096|65536|2048x512 ...]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.grad_clip_compare import D, LR, MAX_N, N_ROWS, T, WORKLOADS, setup  # noqa: E402

ROADS = ("a_by_value", "b_dn_eager", "c_dn_graph")
CAPTURE_LIMIT_REFS = 1 << 20     # above it scone_backward_plan_dn refuses a capturing stream (include/scone_hip.h)


def block(call, steps, warm=2):
    """(median event time, median host time) of one block, in microseconds."""
    import numpy as np
    import torch
    dev, host = [], []
    for i in range(warm + steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if i >= warm:
            dev.append(e0.elapsed_time(e1) * 1e3)
            host.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.median(host))


def summary(v):
    import numpy as np
    return {"median_us": float(np.median(v)), "spread_us": [float(np.min(v)), float(np.max(v))], "blocks": len(v)}


def plan_build_bytes(ntok, n_rows, d, U, n_slots, chunk):
    """The device memory scone_backward_plan holds while it builds (its hipMallocs, rocPRIM's scratch left out) and afterwards."""
    cand = MAX_N * (MAX_N + 1) // 2
    R = ntok * cand
    seg = min(R, n_rows)
    kept = 4 * ntok * 2 + 4 * R + 4 * (seg + 1) + 16 * (R // chunk + seg + 1) + 16 * (R // chunk + 1) + 32
    tmp = 4 * (ntok + 1) * 2 + 4 * R * 5 + 4 * (seg + 2) + 4 * (seg + 1) * 2 + 8 * (seg + 1) * 2 + 4 * ntok * (8 if MAX_N <= 3 else 16)
    return kept + tmp, kept + 4 * n_slots * d


def main():
    import numpy as np
    import torch
    from scone_amd import synthetic as S
    from scone_amd.hip_backend import backward_chunk
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    rounds = int(args[1]) if len(args) > 1 else 5
    steps = int(args[2]) if len(args) > 2 else 10
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    keys, lens, cache, w = setup()
    table = cache.table
    chunk = backward_chunk()
    result = {"device": torch.cuda.get_device_name(0), "n_rows": N_ROWS, "d": D, "max_n": MAX_N, "chunk": chunk, "rounds": rounds,
              "steps": steps, "workloads": {}}
    for name, B in WORKLOADS:
        if only and name not in only:
            continue
        ntok = B * T
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
        g = torch.randn((ntok, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
        # ---- the reference of the bit check, and the memory of today's road
        torch.cuda.synchronize()
        free_closed = torch.cuda.mem_get_info()[0]
        plan = table.backward_plan(tok)
        torch.cuda.synchronize()
        plan_live = free_closed - torch.cuda.mem_get_info()[0]
        U, refs = plan.n_rows, plan.n_refs
        ref_ids, ref_rows = plan.rows(g, "mean")
        plan.close()
        ids_a = torch.empty(U, dtype=torch.int64, device="cuda")
        rows_a = torch.empty((U, D), dtype=torch.float32, device="cuda")
        cap = U + 64
        ids_b = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
        rows_b = torch.full((cap, D), float("nan"), dtype=torch.float32, device="cuda")
        n_b = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx = table.backward_context(ntok)
        ctx.plan(tok)
        ctx.rows(g, "mean", out=(ids_b, rows_b, n_b))
        torch.cuda.synchronize()
        assert int(n_b.item()) == U and ctx.counts() == (U, refs)
        assert torch.equal(ids_b[:U], ref_ids) and torch.equal(rows_b[:U].view(torch.int32), ref_rows.view(torch.int32)), "rows differ"
        assert bool((ids_b[U:] == -7).all())
        del ref_ids, ref_rows

        def road_a():
            with table.backward_plan(tok) as p:
                i_, r_ = p.rows(g, "mean", out=(ids_a, rows_a))
                table.opt_step(i_, r_, w, kind="sgd", lr=LR)

        def road_b():
            ctx.plan(tok)
            ctx.rows(g, "mean", out=(ids_b, rows_b, n_b))
            table.opt_step(ids_b, rows_b, w, kind="sgd", lr=LR, n=n_b)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            road_b()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        calls = {"a_by_value": road_a, "b_dn_eager": road_b}
        graph = None
        if ntok * (MAX_N * (MAX_N + 1) // 2) <= CAPTURE_LIMIT_REFS:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                road_b()
            calls["c_dn_graph"] = graph.replay
        roads = tuple(calls)
        dev = {k: [] for k in roads}
        host = {k: [] for k in roads}
        for _ in range(rounds):
            for k in roads:
                d_us, h_us = block(calls[k], steps)
                dev[k].append(d_us)
                host[k].append(h_us)
        build, _ = plan_build_bytes(ntok, N_ROWS, D, U, 0, chunk)
        entry = {"tokens": ntok, "U": U, "refs": refs,
                 "event_us": {k: summary(dev[k]) for k in roads}, "host_us": {k: summary(host[k]) for k in roads},
                 "memory_bytes": {"ctx_nbytes": ctx.nbytes, "plan_live_measured": int(plan_live), "plan_build_computed_without_rocprim": int(build)}}
        a = entry["event_us"]["a_by_value"]
        entry["margin_us"] = a["spread_us"][1] - a["spread_us"][0]
        if graph is None:
            entry["c_dn_graph"] = "not captured: above 2^20 possible references scone_backward_plan_dn refuses a capturing stream"
        for k in roads[1:]:
            entry[f"{k}_minus_a_event_us"] = entry["event_us"][k]["median_us"] - a["median_us"]
            entry[f"{k}_minus_a_host_us"] = entry["host_us"][k]["median_us"] - entry["host_us"]["a_by_value"]["median_us"]
        result["workloads"][name] = entry
        print(name, json.dumps(entry), flush=True)
        ctx.close()
        del graph, ids_a, rows_a, ids_b, rows_b, tok, g
        torch.cuda.empty_cache()
    assert table.status() == 0
    result["old_road"] = ("no existing kernel changed: the gfx950 disassembly of every kernel of scone_backward.hip, scone_opt.hip, "
                          "scone_opt_lean.hip and scone_grad_norm.hip equals the parent commit's instruction for instruction "
                          "(llvm-objdump -d of the unbundled code objects, compared per kernel)")
    text = json.dumps(result, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
