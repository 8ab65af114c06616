#!/usr/bin/env python3
"""The fused lookup over a batch's live rows (`scone_embed_rows`) against its floor and against the stock road, headline index
(1M rows, d = 768, max_n = 3), bf16 live rows, fp16 output, at 4096 (8 x 512), 65536 (128 x 512) and 2048 x 512 tokens.  One
process, HIP events around the whole call sequence of an arm, the arms alternating in blocks round by round, the warm-up calls of
every block discarded; a block's figure is the median of its timed calls, an arm's the median of its block medians:

  a  SconeTable.embed_rows(tok, row_ids, rows, wte=, wpe=, out=)     the rows of the batch, taken from a bf16 table
  b  SconeTable.embed(tok, wte=, wpe=, out=) on that bf16 table, SCONE_FUSED_MAX_TOKENS=0: two launches like a -- the floor, the
     same gather without the id -> slot search (at d = 768 through the specialised kernel, where a walks the row in units)
  c  the stock road: match_csr + torch.searchsorted(row_ids, ids) + F.embedding_bag(mean) + wte[tok] + wpe, fp16

Before anything is timed the outputs of a and b are compared bit for bit at every size.  Recorded: a / b, a / c, the spread of b's
block medians, the search's share (a - b) and U, the distinct rows of the batch.

    python tools/embed_rows_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import sys

os.environ["SCONE_FUSED_MAX_TOKENS"] = "0"        # read when the handle is created: arm b takes match + gather at every size

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from scone_amd import EmbeddingCache, NGramExtractor
from scone_amd import synthetic as S

D, T = 768, 512
SIZES = (("4096", 8), ("65536", 128), ("2048x512", 2048))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    assert rounds * steps >= 20
    keys, lens = S.make_keys(1_000_000, S.GPT2_VOCAB, 3, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=3)
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="bf16", seed=7, base_scale=0.02)
    table = cache.table
    bmax = max(b for _, b in SIZES)
    rect = torch.from_numpy(S.stream_uniform_ids(keys, lens, bmax, T, 1234)).to("cuda", torch.int32)
    g = torch.Generator(device="cuda").manual_seed(5)
    wte = (torch.randn(S.GPT2_VOCAB, D, generator=g, device="cuda") * 0.02).half()
    wpe = (torch.randn(1024, D, generator=g, device="cuda") * 0.01).half()
    out = torch.empty(bmax * T, D, dtype=torch.float16, device="cuda")
    table.reserve(bmax * T)

    live = {}
    for name, b in SIZES:                                                   # the batch's rows, taken from the bf16 table
        tok = rect[:b].contiguous()
        with table.backward_plan(tok) as plan:
            ids = plan.row_ids().clone()
        live[name] = (tok, ids, table.gather_rows(ids).to(torch.bfloat16))

    def arms(name, b):
        tok, ids, rows = live[name]
        n = b * T
        pos = torch.arange(T, device="cuda").repeat(b)

        def stock():
            off, hit = table.match_csr(tok)
            slots = torch.searchsorted(ids, hit.to(torch.int64))
            fg = F.embedding_bag(slots, rows, off[:-1].to(torch.int64), mode="mean")
            return (wte[tok.reshape(-1).long()] + fg.half()) + wpe[pos]

        return {
            "a": lambda: table.embed_rows(tok, ids, rows, wte=wte, wpe=wpe, out=out[:n]),
            "b": lambda: table.embed(tok, wte=wte, wpe=wpe, out=out[:n]),
            "c": stock,
        }

    for name, b in SIZES:                                                   # same bits on a and b
        r = arms(name, b)
        want = r["b"]().clone()
        out.fill_(float("nan"))
        r["a"]()
        assert torch.equal(out[:b * T].view(torch.int16), want.view(-1, D).view(torch.int16)), name
        del want
    assert table.status() == 0

    res = {name: {k: [] for k in "abc"} for name, _ in SIZES}
    for _ in range(rounds):
        for name, b in SIZES:
            for k, call in arms(name, b).items():
                for _ in range(2):                                          # warm-up of THIS arm at THIS size, discarded
                    call()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                for e0, e1 in ev:
                    e0.record()
                    call()
                    e1.record()
                torch.cuda.synchronize()
                res[name][k].append(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])))
    assert table.status() == 0

    report = {"setup": "1M-row index, d=768, max_n=3, bf16 live rows / bf16 table, fp16 out, SCONE_FUSED_MAX_TOKENS=0; a = embed_rows, "
                       "b = embed on the bf16 table (two launches), c = match_csr + searchsorted + embedding_bag + adds; "
                       "us per call, HIP events around the whole call sequence, median of block medians",
              "rounds": rounds, "steps": steps, "sizes": {}}
    for name, b in SIZES:
        entry = {"tokens": b * T, "U": int(live[name][1].numel())}
        for k, v in res[name].items():
            entry[k] = {"median_us": float(np.median(v)), "block_medians_us": v}
        a, bb, c = (entry[k]["median_us"] for k in "abc")
        entry["a/b"], entry["a/c"] = a / bb, a / c
        entry["b_spread"] = (max(res[name]["b"]) - min(res[name]["b"])) / bb
        entry["search_share_us"] = a - bb
        report["sizes"][name] = entry
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
