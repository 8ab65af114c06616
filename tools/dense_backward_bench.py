#!/usr/bin/env python3
"""The backward of the dense side (`wte` / `wpe` gradients by index plan, `scone_backward_wpe`) against the stock road, headline
index (1M rows, d = 768, max_n = 3, bf16 table), fp16 `grad_out`, vocab 50,257, n_pos 512, iid Zipf(1.1) tokens, at 4096
(8 x 512), 65536 (128 x 512) and 2048 x 512 tokens.  One process, HIP events around the whole call sequence of an arm, the arms
alternating in blocks round by round, the warm-up calls of every block discarded; a block's figure is the median of its timed
calls, an arm's the median of its block medians, its spread (max - min) / median of the block medians.  A 1 GiB device copy is
timed in the same process, the same way.

  a_plan     SconeTable.backward_plan_index(tok, vocab) (allocates, sorts, synchronises once) + close
  a_rows     plan.rows(grad_out) on a plan made beforehand: grad_wte as (ids, rows)
  b_wpe      SconeTable.backward_wpe(grad_out [B, T, d], n_pos): no plan
  b_index    default_positions + backward_plan_index(pos, n_pos) + rows: the same bits through a plan
  c_wte      the stock road: aten.embedding_dense_backward (what F.embedding's backward runs)
  c_wpe      grad_out.view(B, T, d).sum(0)
  d_new      the embedding stage's step on an InPlaceFGramTable: y = m(tok, wte=P, wpe=Q); y.backward(g) -- one fused forward,
             the table gradient and both dense gradients without float atomics
  d_stock    y = m(tok, base=F.embedding(tok, P)) + F.embedding(pos, Q); y.backward(g): the table gradient the same way, the
             dense gradients by torch

Before anything is timed, b_wpe and b_index are compared bit for bit, and a / d_new against the stock gradients within the fp32
bound of the sums.  Each ratio is new / stock, beside the stock arm's own spread.

    python tools/dense_backward_bench.py [out.json] [rounds] [steps]

`rows-ab` mode times `scone_backward_plan` and `scone_backward_rows` of the TABLE's backward on the same three batches and
prints one JSON line: run it in alternating processes with SCONE_HIP_LIB naming a build of the parent commit and this one, to
see that the plan-size refactor under them costs nothing (`python tools/dense_backward_bench.py rows-ab [rounds] [steps]`).
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from scone_amd import _lib

_other = os.environ.get("SCONE_HIP_LIB")
if _other:                                          # a build of an earlier commit lacks the entry points this change adds
    _have = ctypes.CDLL(_other)
    for _name in [n for n in _lib.SIGNATURES if not hasattr(_have, n)]:
        del _lib.SIGNATURES[_name]

from scone_amd import EmbeddingCache, InPlaceFGramTable, NGramExtractor  # noqa: E402
from scone_amd import synthetic as S  # noqa: E402

D, T, N_POS = 768, 512, 512
SIZES = (("4096", 8), ("65536", 128), ("2048x512", 2048))


def timed(call, steps):
    for _ in range(2):                              # warm-up of THIS arm at THIS size, discarded
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))


def summary(v):
    m = float(np.median(v))
    return {"median_us": m, "spread": (max(v) - min(v)) / m, "block_medians_us": v}


def world(tokens="zipf"):
    keys, lens = S.make_keys(1_000_000, S.GPT2_VOCAB, 3, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=3)
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="bf16", seed=7, base_scale=0.02)
    bmax = max(b for _, b in SIZES)
    if tokens == "zipf":
        tok = torch.from_numpy(S.stream_zipf(S.GPT2_VOCAB, bmax, T, 1234)).to("cuda", torch.int32)
    else:                                           # f-grams laid end to end: every position has table references
        tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, bmax, T, 1234)).to("cuda", torch.int32)
    cache.table.reserve(bmax * T)
    return cache, tok


def rows_ab(rounds, steps):
    cache, tok_all = world("f-grams")
    table = cache.table
    g = torch.randn(tok_all.numel(), D, device="cuda").half()
    res = {}
    for _ in range(rounds):
        for name, b in SIZES:
            tok = tok_all[:b].contiguous()
            with table.backward_plan(tok) as plan:
                ids = torch.empty(plan.n_rows, dtype=torch.int64, device="cuda")
                rows = torch.empty((plan.n_rows, D), dtype=torch.float32, device="cuda")
                res.setdefault(name + "/rows", []).append(timed(lambda: plan.rows(g[:b * T], "mean", out=(ids, rows)), steps))
            res.setdefault(name + "/plan", []).append(timed(lambda: table.backward_plan(tok).close(), steps))
    assert table.status() == 0
    print(json.dumps({"lib": _other or "this tree", "cells": {k: summary(v) for k, v in res.items()}}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rows-ab":
        return rows_ab(int(sys.argv[2]) if len(sys.argv) > 2 else 5, int(sys.argv[3]) if len(sys.argv) > 3 else 6)
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    assert rounds * steps >= 20
    cache, tok_all = world()
    table = cache.table
    gen = torch.Generator(device="cuda").manual_seed(5)
    P = (torch.randn(S.GPT2_VOCAB, D, generator=gen, device="cuda") * 0.02).half().requires_grad_()
    Q = (torch.randn(N_POS, D, generator=gen, device="cuda") * 0.01).half().requires_grad_()
    g_all = torch.randn(tok_all.numel(), D, generator=gen, device="cuda").half()
    module = InPlaceFGramTable(cache)
    gib_src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    gib_dst = torch.empty_like(gib_src)

    def arms(b):
        tok = tok_all[:b].contiguous()
        tok64 = tok.reshape(-1).long()
        g = g_all[:b * T]
        g3 = g.view(b, T, D)
        pos = torch.arange(T, device="cuda").repeat(b)
        plan = table.backward_plan_index(tok, S.GPT2_VOCAB)
        ids = torch.empty(plan.n_rows, dtype=torch.int64, device="cuda")
        rows = torch.empty((plan.n_rows, D), dtype=torch.float32, device="cuda")

        def b_index():
            with table.backward_plan_index(table.default_positions(b, T), N_POS) as p:
                return p.rows(g, "sum")[1]

        def clear():
            P.grad = Q.grad = None
            module.grad = None

        def d_new():
            clear()
            module(tok, wte=P, wpe=Q).backward(g3)

        def d_stock():
            clear()
            (module(tok, base=F.embedding(tok64.view(b, T), P)) + F.embedding(pos.view(b, T), Q)).backward(g3)

        return plan, {
            "a_plan": lambda: table.backward_plan_index(tok, S.GPT2_VOCAB).close(),
            "a_rows": lambda: plan.rows(g, "sum", out=(ids, rows)),
            "b_wpe": lambda: table.backward_wpe(g3, N_POS),
            "b_index": b_index,
            "c_wte": lambda: torch.ops.aten.embedding_dense_backward(g, tok64, S.GPT2_VOCAB, -1, False),
            "c_wpe": lambda: g3.sum(0),
            "d_new": d_new,
            "d_stock": d_stock,
        }

    for name, b in SIZES:                                                   # the arms compute the same thing
        plan, r = arms(b)
        assert torch.equal(r["b_wpe"]().view(torch.int32), r["b_index"]().view(torch.int32)), name
        ids, rows = r["a_rows"]()
        stock = r["c_wte"]().float()
        tol = 5e-2 * stock.abs().max().item()           # a sanity check: the stock sums are fp16, added in no fixed order
        assert (stock[ids] - rows).abs().max().item() <= tol, name
        r["d_new"]()
        new_wte, new_wpe, new_tab = P.grad.float().clone(), Q.grad.float().clone(), module.grad[1].clone()
        r["d_stock"]()
        assert (P.grad.float() - new_wte).abs().max().item() <= tol and torch.equal(module.grad[1], new_tab), name
        assert (Q.grad.float() - new_wpe).abs().max().item() <= 5e-2 * new_wpe.abs().max().item(), name
        plan.close()
    assert table.status() == 0

    res = {name: {} for name, _ in SIZES}
    copy = []
    for _ in range(rounds):
        copy.append(timed(lambda: gib_dst.copy_(gib_src), steps))
        for name, b in SIZES:
            plan, r = arms(b)
            for k, call in r.items():
                res[name].setdefault(k, []).append(timed(call, steps))
            plan.close()
    assert table.status() == 0

    c = summary(copy)
    c["GB_per_s_read_plus_write"] = 2 * (1 << 30) / (c["median_us"] * 1e-6) / 1e9
    report = {"setup": "1M-row index, d=768, max_n=3, bf16 table, fp16 grad_out / wte / wpe, vocab 50257, n_pos 512, iid Zipf(1.1) "
                       "tokens; us per call, HIP events around the whole call sequence, median of block medians, spread = "
                       "(max - min) / median of the block medians; ratios are new / stock",
              "rounds": rounds, "steps": steps, "copy_1GiB": c, "sizes": {}}
    for name, b in SIZES:
        e = {"tokens": b * T}
        e.update({k: summary(v) for k, v in res[name].items()})
        m = {k: e[k]["median_us"] for k in res[name]}
        e["wte: (a_plan + a_rows) / c_wte"] = (m["a_plan"] + m["a_rows"]) / m["c_wte"]
        e["wte: a_rows / c_wte"] = m["a_rows"] / m["c_wte"]
        e["wpe: b_wpe / c_wpe"] = m["b_wpe"] / m["c_wpe"]
        e["wpe: b_wpe / b_index"] = m["b_wpe"] / m["b_index"]
        e["step: d_new / d_stock"] = m["d_new"] / m["d_stock"]
        report["sizes"][name] = e
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
