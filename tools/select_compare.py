#!/usr/bin/env python3
"""The fused lookup at chosen positions (`scone_embed_select`) against the two roads a serving loop had before it.  Two tables:
the headline one (1M-row INT8, d = 768, fp16 out) and a 1M-row fp16 table at d = 4096 (the any-d body: no one-launch road
existed there).  One process, HIP events around the WHOLE call sequence of a road, the roads alternating in blocks round by
round, the warm-up calls of every block discarded; before anything is timed the outputs of the three roads are compared bit for
bit.

  a  the full lookup over every token (embed_varlen / embed), then index_select of the wanted rows
  b  the windows that decide the wanted rows repacked by torch indexing into a rectangle, embed with explicit positions, slice
  c  embed_select

Packed workloads: 256 sequences of 8..512 tokens; a step wants the last token of each ("last1"), the last 4 of each ("last4"),
or one 512-token chunk plus the last token of the 255 others ("chunk": road b is two embed calls and a cat).  What a serving
loop knows on the host before the step -- cu_seqlens, the wanted positions, the window indices and their positions -- is on the
device before the clock starts, for every road alike.

Rectangular workloads: B = 1 / 8 / 64 at T = 512, the step of `Engine.generate_ids` on a covering lookup: the last max_n
positions of every row.  Here the roads start from what the engine holds, `ids` int64 [B, T] on the device, and the torch glue
of each is inside the clock: b is the engine's own code (slice the last 2 max_n - 1 tokens, build their positions, embed, slice),
c converts `ids`, builds `sel` on the device and calls embed_select.

    python tools/select_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scone_amd import EmbeddingCache, NGramExtractor
from scone_amd import synthetic as S

MAX_N, T_RECT, N_SEQS = 3, 512, 256
TABLES = (("int8_d768", "int8", 768, 0.02 / 127), ("fp16_d4096", "fp16", 4096, 0.02))


def packed_workloads(table, keys, lens, wte, wpe, dev):
    rng = np.random.default_rng(99)
    seq_lens = rng.integers(8, 513, size=N_SEQS)
    seq_lens[17] = 512                                                       # the sequence whose 512 tokens are the prefill chunk
    cu_np = np.zeros(N_SEQS + 1, dtype=np.int64)
    np.cumsum(seq_lens, out=cu_np[1:])
    total = int(cu_np[-1])
    # one long token stream cut into the sequences (stream_uniform_ids draws whole rows; only the f-gram density matters here)
    rows = (total + T_RECT - 1) // T_RECT
    tok = torch.from_numpy(S.stream_uniform_ids(keys, lens, rows, T_RECT, 4321).reshape(-1)[:total].copy()).to(dev, torch.int32)
    cu = torch.from_numpy(cu_np.astype(np.int32)).to(dev)
    d = table.dim

    def window(last, k):
        """[n, MAX_N - 1 + k] flattened indices ending at `last`, and their places inside their sequences."""
        w = MAX_N - 1 + k
        idx = last[:, None] + np.arange(-w + 1, 1)[None, :]
        seq = np.searchsorted(cu_np, last, side="right") - 1
        assert (idx >= cu_np[seq][:, None]).all()                          # every window lies inside its sequence
        return torch.from_numpy(idx).to(dev), torch.from_numpy(idx - cu_np[seq][:, None]).to(dev, torch.int32)

    out = {}
    for name, k in (("last1", 1), ("last4", 4)):
        sel_np = EmbeddingCache.last_positions(cu_np, k).numpy().astype(np.int64)
        sel = torch.from_numpy(sel_np).to(dev, torch.int32)
        sel64 = sel.long()
        idx, pos = window(cu_np[1:] - 1, k)
        out[name] = dict(n_sel=len(sel_np), tokens=total, roads={
            "a": lambda sel64=sel64: table.embed_varlen(tok, cu, wte=wte, wpe=wpe).index_select(0, sel64),
            "b": lambda idx=idx, pos=pos, k=k: table.embed(tok[idx], wte=wte, wpe=wpe, position_ids=pos)[:, -k:].reshape(-1, d),
            "c": lambda sel=sel: table.embed_select(tok, sel, cu_seqlens=cu, wte=wte, wpe=wpe)})
    # one sequence of exactly 512 tokens is wanted whole (a prefill chunk), the last token of every other one
    big, chunk_len = 17, 512
    chunk = np.arange(cu_np[big + 1] - chunk_len, cu_np[big + 1])
    others = np.delete(cu_np[1:] - 1, big)
    sel_np = np.concatenate([chunk, others])
    sel = torch.from_numpy(sel_np).to(dev, torch.int32)
    sel64 = sel.long()
    lo = max(int(cu_np[big]), int(chunk[0]) - (MAX_N - 1))                  # the chunk with the context in front of it
    cidx = torch.arange(lo, int(cu_np[big + 1]), device=dev)
    cpos = (cidx - int(cu_np[big])).to(torch.int32)[None, :]
    idx, pos = window(others, 1)
    out["chunk"] = dict(n_sel=len(sel_np), tokens=total, roads={
        "a": lambda: table.embed_varlen(tok, cu, wte=wte, wpe=wpe).index_select(0, sel64),
        "b": lambda: torch.cat([table.embed(tok[cidx][None, :], wte=wte, wpe=wpe, position_ids=cpos)[0, -chunk_len:],
                                table.embed(tok[idx], wte=wte, wpe=wpe, position_ids=pos)[:, -1]]),
        "c": lambda: table.embed_select(tok, sel, cu_seqlens=cu, wte=wte, wpe=wpe)})
    return out


def rect_workloads(table, keys, lens, wte, wpe, dev):
    out = {}
    d = table.dim
    rect = torch.from_numpy(S.stream_uniform_ids(keys, lens, 64, T_RECT, 1234)).to(dev, torch.int64)
    for B in (1, 8, 64):
        ids = rect[:B].contiguous()
        T = T_RECT
        redo, win = min(MAX_N, T), min(T, 2 * MAX_N - 1)

        def road_a(ids=ids, B=B):
            sel = (torch.arange(B, device=dev)[:, None] * T + torch.arange(T - redo, T, device=dev)[None, :]).reshape(-1)
            return table.embed(ids, wte=wte, wpe=wpe).reshape(-1, d).index_select(0, sel)

        def road_b(ids=ids, B=B):                                           # engine.py, the covering branch of generate_ids
            pos = torch.arange(T - win, T, device=dev).unsqueeze(0).expand(B, -1)
            return table.embed(ids[:, -win:], wte=wte, wpe=wpe, position_ids=pos)[:, -redo:, :].reshape(-1, d)

        def road_c(ids=ids, B=B):
            sel = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] * T
                   + torch.arange(T - redo, T, device=dev, dtype=torch.int32)[None, :]).reshape(-1)
            return table.embed_select(ids, sel, wte=wte, wpe=wpe)

        out[f"B{B}xT{T}"] = dict(n_sel=B * redo, tokens=B * T, roads={"a": road_a, "b": road_b, "c": road_c})
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    assert rounds * steps >= 20
    dev = torch.device("cuda")
    keys, lens = S.make_keys(1_000_000, S.GPT2_VOCAB, MAX_N, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=MAX_N)
    report = {"what": "call time in us, HIP events around the whole call sequence of a road; a = full lookup + index_select, "
                      "b = windows repacked by torch indexing + embed + slice, c = embed_select; median_us is the median of "
                      "the block medians, spread_us their minimum and maximum",
              "rounds": rounds, "steps": steps, "tables": {}}
    for tname, fmt, d, scale in TABLES:
        cache = EmbeddingCache.from_synthetic(ex, d, table_format=fmt, seed=7, base_scale=scale)
        table = cache.table
        g = torch.Generator(device="cuda").manual_seed(5)
        wte = (torch.randn(S.GPT2_VOCAB, d, generator=g, device="cuda") * 0.02).half()
        wpe = (torch.randn(1024, d, generator=g, device="cuda") * 0.01).half()
        work = {}
        work.update(packed_workloads(table, keys, lens, wte, wpe, dev))
        work.update(rect_workloads(table, keys, lens, wte, wpe, dev))
        table.reserve(max(w["tokens"] for w in work.values()))

        for name, w in work.items():                                        # same bits on all three roads
            got = {k: call().contiguous() for k, call in w["roads"].items()}
            assert tuple(got["c"].shape) == (w["n_sel"], d), (tname, name, got["c"].shape)
            for k in "ab":
                assert torch.equal(got[k].view(torch.int16), got["c"].view(torch.int16)), (tname, name, k)
            del got
        assert table.status() == 0

        blocks = {name: {k: [] for k in "abc"} for name in work}
        for _ in range(rounds):
            for name, w in work.items():
                for k, call in w["roads"].items():
                    for _ in range(2):                                      # warm-up of THIS road at THIS workload, discarded
                        call()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                    for e0, e1 in ev:
                        e0.record()
                        call()
                        e1.record()
                    torch.cuda.synchronize()
                    blocks[name][k].append(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])))
        assert table.status() == 0

        entry = {"table": f"1M-row {fmt}, d={d}, max_n={MAX_N}, fp16 out", "workloads": {}}
        for name, w in work.items():
            e = {"tokens": w["tokens"], "n_sel": w["n_sel"]}
            for k, v in blocks[name].items():
                e[k] = {"median_us": float(np.median(v)), "spread_us": [float(np.min(v)), float(np.max(v))], "blocks": len(v)}
            e["c/a"] = e["c"]["median_us"] / e["a"]["median_us"]
            e["c/b"] = e["c"]["median_us"] / e["b"]["median_us"]
            entry["workloads"][name] = e
        report["tables"][tname] = entry
        del cache, table, wte, wpe, work
        torch.cuda.empty_cache()
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
