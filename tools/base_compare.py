#!/usr/bin/env python3
"""The fused lookup onto a dense base (`scone_embed_base`) against the road `embed_tokens(base=...)` took before it, headline
table (1M-row INT8, d = 768, fp16 out), at 4096 (8 x 512), 65536 (128 x 512) and 2048 x 512 tokens.  One process, HIP events
around the WHOLE call sequence of a road (its launches, allocations and, for road a, its host synchronise), the three roads
alternating in blocks round by round, the warm-up calls of every block discarded:

  a  SconeTable.match_csr + SconeTable.gather_reduce(base=)    the earlier road: five launches and a host synchronise
  b  SconeTable.embed_base(tok, base, out=out)                 the new call: one launch up to 32768 tokens, two above
  c  SconeTable.embed(tok, wte=, wpe=, out=out)                context: the same tokens on the wte road

b reads B*T*d*2 compulsory bytes of base rows that c gets from L2-resident wte rows, so b slower than c is expected; the claim
to check is b against a.  Before anything is timed, the outputs of a and b are compared bit for bit at every size.

    python tools/base_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

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
    cache = EmbeddingCache.from_synthetic(ex, D, table_format="int8", seed=7, base_scale=0.02 / 127)
    table = cache.table
    bmax = max(b for _, b in SIZES)
    rect = torch.from_numpy(S.stream_uniform_ids(keys, lens, bmax, T, 1234)).to("cuda", torch.int32)
    g = torch.Generator(device="cuda").manual_seed(5)
    wte = (torch.randn(S.GPT2_VOCAB, D, generator=g, device="cuda") * 0.02).half()
    wpe = (torch.randn(1024, D, generator=g, device="cuda") * 0.01).half()
    base = (torch.randn(bmax * T, D, generator=g, device="cuda") * 0.02).half()
    out = torch.empty(bmax * T, D, dtype=torch.float16, device="cuda")
    table.reserve(bmax * T)

    def roads(b):
        tok, n = rect[:b].contiguous(), b * T
        return {
            "a": lambda: table.gather_reduce(*table.match_csr(tok), "mean", base=base[:n], out_dtype=torch.float16),
            "b": lambda: table.embed_base(tok, base[:n], out=out[:n]),
            "c": lambda: table.embed(tok, wte=wte, wpe=wpe, out=out[:n]),
        }

    for name, b in SIZES:                                                   # same bits on both base roads
        r = roads(b)
        want = r["a"]()
        out.fill_(float("nan"))
        r["b"]()
        assert torch.equal(out[:b * T].view(torch.int16), want.view(torch.int16)), name
        del want
    assert table.status() == 0

    res = {name: {k: [] for k in "abc"} for name, _ in SIZES}
    for _ in range(rounds):
        for name, b in SIZES:
            for k, call in roads(b).items():
                for _ in range(2):                                          # warm-up of THIS road at THIS size, discarded
                    call()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                for e0, e1 in ev:
                    e0.record()
                    call()
                    e1.record()
                torch.cuda.synchronize()
                res[name][k] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    assert table.status() == 0

    report = {"table": "1M-row INT8, d=768, max_n=3, fp16 out; a = match_csr + gather_reduce(base), b = embed_base, "
                       "c = embed(wte, wpe); call time in us, HIP events around the whole call sequence",
              "rounds": rounds, "steps": steps, "sizes": {}}
    for name, b in SIZES:
        entry = {"tokens": b * T}
        for k, v in res[name].items():
            entry[k] = {"min_us": float(np.min(v)), "median_us": float(np.median(v)), "max_us": float(np.max(v)), "timed_calls": len(v)}
        entry["b/a"] = entry["b"]["median_us"] / entry["a"]["median_us"]
        entry["b/c"] = entry["b"]["median_us"] / entry["c"]["median_us"]
        report["sizes"][name] = entry
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
