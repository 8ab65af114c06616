#!/usr/bin/env python3
"""The fused sparse optimizer step (`FGramOptimizer.step`, one `scone_opt_step` launch) against the stock road (a `torch.optim`
sparse step, then `TrainableFGramTable.commit()`), on the headline index: 1M-row INT8 served table, d = 768, fp32 master,
max_n = 3.  The row sets are those of `backward_plan` over 4,096 (8 x 512), 65,536 (128 x 512) and 2048 x 512 tokens of the
S_uniform stream; the gradient rows are what `BackwardPlan.rows` returns for a random fp16 `grad_out`.

One process, HIP events around each call, the blocks alternating round by round, the warm-up calls of every block discarded;
per block the median of its steps, per arm the median of the block medians and their minimum and maximum.  Both arms start
from `weight.grad` already set (setting it is host work common to both).  Before anything is timed one step of each arm from
equal weights is compared (fp32 evaluations in different orders: a relative difference below 1e-5), and the served rows the
fused step wrote are compared with a gather of `store_f32` of its weights.

  fused_<kind>   FGramOptimizer.step(): master, state and served table in one launch, no synchronise
  stock_<kind>   torch.optim.SGD / SparseAdam .step() + commit() (unique over the touched ids, weight[ids], store_f32_ids,
                 the stream synchronise of SconeTable.store_f32)

Also recorded: U, the bytes a step has to move (U * d * 4 * (reads + writes) + U * (d + 2) for the INT8 row and its scale;
SGD reads g, w and writes w, Adam reads g, w, m, v and writes w, m, v), that over the fused time, and the same as a fraction of
the device-copy rate measured in this process (a 1 GiB device-to-device copy, read + written bytes over its time).

    python tools/opt_step_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_N, D, N_ROWS, T = 3, 768, 1_000_000, 512
WORKLOADS = (("4096", 8), ("65536", 128), ("2048x512", 2048))
STREAMS = {"sgd": (2, 1), "adam": (4, 3)}          # fp32 row streams read, written
LR = 1e-3


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


def copy_rate_tbs():
    import torch
    n = 1 << 30
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    us = [timed(lambda: dst.copy_(src), 4) for _ in range(5)]
    del src, dst
    torch.cuda.empty_cache()
    return 2 * n / (sorted(us)[2] * 1e-6) / 1e12


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6

    import torch
    from scone_amd import EmbeddingCache, FGramOptimizer, NGramExtractor, TrainableFGramTable
    from scone_amd import synthetic as S
    keys, lens = S.make_keys(N_ROWS, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="int8", seed=7, base_scale=0.02 / 127)
    table = cache.table
    copy_tbs = copy_rate_tbs()
    w0 = table.gather_rows(torch.arange(N_ROWS, device="cuda"))                # the master: the served rows, dequantised
    report = {"what": "call time in us, HIP events around each call; median_us is the median of the block medians, spread_us "
                      "their minimum and maximum",
              "table": f"1M-row int8 served table, d={D}, fp32 master, max_n={MAX_N}, row sets of S_uniform token batches",
              "rounds": rounds, "steps": steps, "device_copy_TBps": copy_tbs, "workloads": {}}

    for name, B in WORKLOADS:
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
        g = torch.randn((B * T, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)).half()
        with table.backward_plan(tok) as plan:
            row_ids, grad_rows = plan.rows(g, "mean")
        torch.cuda.synchronize()
        del g
        U = int(row_ids.numel())
        sparse = torch.sparse_coo_tensor(row_ids[None], grad_rows, (N_ROWS, D), is_coalesced=True)
        e = {"tokens": tok.numel(), "U": U}
        for kind in ("sgd", "adam"):
            fused = TrainableFGramTable(cache, w0.clone())
            stock = TrainableFGramTable(cache, w0.clone())
            opt = FGramOptimizer(fused, kind, lr=LR)
            topt = (torch.optim.SGD([stock.weight], lr=LR) if kind == "sgd" else torch.optim.SparseAdam([stock.weight], lr=LR))

            def fused_step():
                fused.weight.grad = sparse
                opt.step()

            def stock_step():
                stock.weight.grad = sparse
                stock._touched.append(row_ids)
                topt.step()
                stock.commit()

            # agreement before anything is timed
            stock_step()
            fused_step()
            diff = float((fused.weight.detach()[row_ids] - stock.weight.detach()[row_ids]).abs().max())
            scale = float(stock.weight.detach()[row_ids].abs().max())
            assert diff <= 1e-5 * max(scale, 1.0), (kind, diff, scale)
            served = table.gather_rows(row_ids)
            table.store_f32(fused.weight.detach()[row_ids], ids=row_ids)
            assert torch.equal(served.view(torch.int32), table.gather_rows(row_ids).view(torch.int32)), "the served rows differ"
            assert fused.commit() == 0

            calls = {f"fused_{kind}": fused_step, f"stock_{kind}": stock_step}
            blocks = {k: [] for k in calls}
            for _ in range(rounds):
                for k, call in calls.items():
                    blocks[k].append(timed(call, steps))
            f, s = summary(blocks[f"fused_{kind}"]), summary(blocks[f"stock_{kind}"])
            reads, writes = STREAMS[kind]
            moved = U * D * 4 * (reads + writes) + U * (D + 2)
            tbs = moved / (f["median_us"] * 1e-6) / 1e12
            e[f"fused_{kind}"], e[f"stock_{kind}"] = f, s
            e[f"{kind}_bytes_moved"] = moved
            e[f"fused_{kind}_TBps"] = tbs
            e[f"fused_{kind}_fraction_of_copy_rate"] = tbs / copy_tbs
            e[f"fused_{kind}/stock_{kind}"] = f["median_us"] / s["median_us"]
            e[f"fused_{kind}_beats_stock_beyond_its_spread"] = bool(s["median_us"] - f["median_us"] > s["spread_us"][1] - s["spread_us"][0])
            e[f"{kind}_max_abs_diff_vs_stock_after_one_step"] = diff
            del fused, stock, opt, topt
            torch.cuda.empty_cache()
        report["workloads"][name] = e
        del sparse, row_ids, grad_rows
        torch.cuda.empty_cache()
    assert table.status() == 0
    text = json.dumps(report, indent=1)
    print(text)
    if out_path and out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
