#!/usr/bin/env python3
"""The lookup's backward (`scone_backward_*`) against the stock-ops road, on the headline index and token stream: 1M-row table,
d = 768, max_n = 3, S_uniform tokens, fp16 `grad_out`, at 4,096 (8 x 512), 65,536 (128 x 512) and 2048 x 512 tokens.

One process, HIP events around each block, the blocks alternating round by round, the warm-up calls of every block discarded;
per block the median of its steps, per workload the median of the block medians and their minimum and maximum.  Before anything
is timed the library's rows are compared with the stock road's (same row ids; values within fp32 summation error -- the stock
road adds with float atomics in no fixed order, so its bits are not comparable) and two calls of the library bit for bit.

  plan        SconeTable.backward_plan + close (match, expand, stable radix sort by row, segment scans; one synchronise)
  rows        BackwardPlan.rows(grad_out, "mean") into buffers made once: the chunk pass and the second pass
  counts      BackwardPlan.counts()
  embed       the forward lookup of the same tokens (fp16 out), for scale
  stock_plan  match_csr (with its host synchronise), the expanded position index, torch.unique(ids, return_inverse=True)
  stock_rows  index_add_ of (g.float() * w)[pos] into a zeroed [U, d]: the stock road's reduce step

Also recorded: n_refs, U, the bytes the reduction moves (n_refs * d * sizeof(g) + U * d * 4) and that over the rows time as a
fraction of the measured device-copy rate (README: 5.4-5.8 TB/s).  The rows block is repeated, each in a child process of its
own, for every chunk length C whose library tools/build_backward_chunks.sh has built (build/bwd_chunks/libbwd_c<C>.so).

    python tools/backward_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_N, D, N_ROWS, T = 3, 768, 1_000_000, 512
WORKLOADS = (("4096", 8), ("65536", 128), ("2048x512", 2048))
COPY_RATE_TBS = (5.4, 5.8)


def timed(call, steps, warm=2):
    import numpy as np
    import torch
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


def setup():
    import torch
    from scone_amd import EmbeddingCache, NGramExtractor
    from scone_amd import synthetic as S
    keys, lens = S.make_keys(N_ROWS, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="int8", seed=7, base_scale=0.02 / 127)
    table = cache.table
    work = {}
    for name, B in WORKLOADS:
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
        g = torch.randn((B * T, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
        work[name] = (tok, g)
    table.reserve(max(t.numel() for t, _ in work.values()))
    return cache, table, work


def rows_only(rounds, steps):
    """Child process: the rows block alone, with whatever library SCONE_HIP_LIB names."""
    import torch
    from scone_amd.hip_backend import backward_chunk
    cache, table, work = setup()
    out = {"C": backward_chunk(), "workloads": {}}
    for name, (tok, g) in work.items():
        with table.backward_plan(tok) as plan:
            bufs = (torch.empty(plan.n_rows, dtype=torch.int64, device="cuda"), torch.empty((plan.n_rows, D), device="cuda"))
            blocks = [timed(lambda: plan.rows(g, "mean", out=bufs), steps) for _ in range(rounds)]
            torch.cuda.synchronize()
        out["workloads"][name] = summary(blocks)
    assert table.status() == 0
    print("ROWS_ONLY " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if a != "--rows-only"]
    out_path = args[0] if len(args) > 0 else None
    rounds = int(args[1]) if len(args) > 1 else 5
    steps = int(args[2]) if len(args) > 2 else 6
    if "--rows-only" in sys.argv:
        return rows_only(rounds, steps)

    # the other chunk lengths first, each in a fresh child process (a process loads one library), before this one opens the GPU
    variants = {}
    for c in (64, 128, 256, 512):
        lib = os.path.join(ROOT, "build", "bwd_chunks", f"libbwd_c{c}.so")
        if not os.path.exists(lib):
            continue
        env = dict(os.environ, SCONE_HIP_LIB=lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-only", "-", str(rounds), str(steps)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"the C = {c} child failed ({r.returncode}); nothing more is started\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS_ONLY ")][-1]
        rec = json.loads(line[len("ROWS_ONLY "):])
        assert rec["C"] == c
        variants[str(c)] = rec["workloads"]

    import numpy as np
    import torch
    from scone_amd.hip_backend import backward_chunk
    cache, table, work = setup()
    report = {"what": "call time in us, HIP events around each block; median_us is the median of the block medians, spread_us "
                      "their minimum and maximum",
              "table": f"1M-row int8, d={D}, max_n={MAX_N}, S_uniform tokens, fp16 grad_out, reduce=mean",
              "rounds": rounds, "steps": steps, "C": backward_chunk(), "rows_us_by_C": variants, "workloads": {}}

    def stock_plan(tok):
        off, ids = table.match_csr(tok)
        K = off[1:] - off[:-1]
        pos = torch.repeat_interleave(torch.arange(K.numel(), device="cuda"), K.long())
        uniq, inverse = torch.unique(ids, return_inverse=True)
        return K, pos, uniq, inverse

    def stock_rows(g, K, pos, uniq, inverse, out):
        w = 1.0 / K.clamp(min=1).float()
        out.zero_()
        out.index_add_(0, inverse, (g.float() * w[:, None])[pos])
        return out

    for name, (tok, g) in work.items():
        plan = table.backward_plan(tok)
        U, n_refs = plan.n_rows, plan.n_refs
        bufs = (torch.empty(U, dtype=torch.int64, device="cuda"), torch.empty((U, D), device="cuda"))
        K, pos, uniq, inverse = stock_plan(tok)
        stock_out = torch.empty((U, D), device="cuda")
        emb_out = torch.empty((*tok.shape, D), dtype=torch.float16, device="cuda")
        # agreement before anything is timed
        ids, rows = plan.rows(g, "mean", out=bufs)
        again = plan.rows(g, "mean")
        assert torch.equal(ids, again[0]) and torch.equal(rows.view(torch.int32), again[1].view(torch.int32)), "not reproducible"
        assert torch.equal(ids, uniq.long()) and pos.numel() == n_refs
        ref = stock_rows(g, K, pos, uniq, inverse, stock_out)
        scale = float(ref.abs().max())
        err = float((rows - ref).abs().max()) / scale
        assert err < 1e-3, err
        assert torch.equal(plan.counts(), K.int())
        calls = {
            "plan": lambda: table.backward_plan(tok).close(),
            "rows": lambda: plan.rows(g, "mean", out=bufs),
            "counts": lambda: plan.counts(),
            "embed": lambda: table.embed(tok, out_dtype=torch.float16, out=emb_out),
            "stock_plan": lambda: stock_plan(tok),
            "stock_rows": lambda: stock_rows(g, K, pos, uniq, inverse, stock_out),
        }
        blocks = {k: [] for k in calls}
        for _ in range(rounds):
            for k, call in calls.items():
                blocks[k].append(timed(call, steps))
        e = {"tokens": tok.numel(), "n_refs": n_refs, "U": U, "max_rel_diff_vs_stock": err}
        for k, v in blocks.items():
            e[k] = summary(v)
        moved = n_refs * D * g.element_size() + U * D * 4
        e["bytes_moved"] = moved
        tbs = moved / (e["rows"]["median_us"] * 1e-6) / 1e12
        e["rows_TBps"] = tbs
        e["rows_fraction_of_copy_rate"] = [tbs / COPY_RATE_TBS[1], tbs / COPY_RATE_TBS[0]]
        e["rows/stock_rows"] = e["rows"]["median_us"] / e["stock_rows"]["median_us"]
        e["rows_beats_stock_rows_beyond_its_spread"] = bool(
            e["stock_rows"]["median_us"] - e["rows"]["median_us"] > e["stock_rows"]["spread_us"][1] - e["stock_rows"]["spread_us"][0])
        report["workloads"][name] = e
        plan.close()
        del bufs, K, pos, uniq, inverse, stock_out, emb_out, ref, rows, ids, again
        torch.cuda.empty_cache()
    assert table.status() == 0
    text = json.dumps(report, indent=1)
    print(text)
    if out_path and out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
