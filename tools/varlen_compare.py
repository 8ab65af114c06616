#!/usr/bin/env python3
"""The packed variable-length lookup (`scone_embed_varlen`) against the rectangular one, headline table (1M-row INT8,
d = 768, fp16 out, wte and wpe), 2048 sequences, one process, HIP events, the variants alternating round by round, warm-up
steps discarded, medians over rounds x steps >= 20 timed steps per variant:

  a  scone_embed on the rectangle [2048, 512], default positions          (yardstick: code this feature does not touch)
  b  the same rectangle with explicit position_ids                        (yardstick)
  c  the packed call on the same tokens, 2048 equal lengths of 512
  d  the packed call on lengths uniform in 1..512 (about half the tokens)
  e  scone_embed on those ragged sequences PADDED to [2048, 512]          (yardstick: what a caller does today)
  c_T<n>, d_T<n>  c / d on handles whose gather traversal uses rows of n tokens (SCONE_VARLEN_T; default: the stream is one row)
  f1 / f2  a ragged 4,096-token batch (128 sequences of 1..63 tokens) in the one-launch form / in the two-kernel form

Every variant reports `step_us` (stream time of one call) and `match_us` (stream time minus the gather kernels' own time as
`scone_profile_*` brackets them: the match kernel plus the launch gap; 0 for the one-launch form).  Ratios: c/b = the cost of
the boundary search and of the traversal, c/a = that plus the loss of the register-held position row, d/e = the point of the
feature.  The outputs of c (every traversal) are checked bit for bit against a's.

    python tools/varlen_compare.py [out.json] [rounds] [steps]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scone_amd import EmbeddingCache, NGramExtractor
from scone_amd import synthetic as S

B, T, D = 2048, 512, 768
PAD = S.GPT2_VOCAB - 1            # GPT-2's <|endoftext|>, the usual pad id


def handle(ex, **env):
    """A handle of the headline table created under `env` (the library reads its switches in scone_create)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        c = EmbeddingCache.from_synthetic(ex, D, table_format="int8", seed=7, base_scale=0.02 / 127)
        c.table                       # created now, while the environment holds
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return c


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    assert rounds * steps >= 20
    keys, lens = S.make_keys(1_000_000, S.GPT2_VOCAB, 3, seed=11)
    ex = NGramExtractor.from_arrays(keys, lens, max_n=3)
    rect = torch.from_numpy(S.stream_uniform_ids(keys, lens, B, T, 1234)).to("cuda", torch.int32)
    g = torch.Generator(device="cuda").manual_seed(5)
    wte = (torch.randn(S.GPT2_VOCAB, D, generator=g, device="cuda") * 0.02).half()
    wpe = (torch.randn(1024, D, generator=g, device="cuda") * 0.01).half()
    out = torch.empty(B * T, D, dtype=torch.float16, device="cuda")

    pos_rect = torch.arange(T, dtype=torch.int32, device="cuda").expand(B, T).contiguous()
    cu_equal = (torch.arange(B + 1, dtype=torch.int32) * T).cuda()
    rng = np.random.default_rng(99)
    rag = rng.integers(1, T + 1, size=B)
    keep = torch.from_numpy(np.arange(T)[None, :] < rag[:, None]).cuda()
    packed = rect[keep].contiguous()                                     # row-major: sequence after sequence
    cu_rag = torch.from_numpy(np.concatenate([[0], np.cumsum(rag)]).astype(np.int32)).cuda()
    padded = torch.where(keep, rect, torch.full_like(rect, PAD)).contiguous()
    small = rng.integers(1, 64, size=128)
    cu_small = torch.from_numpy(np.concatenate([[0], np.cumsum(small)]).astype(np.int32)).cuda()
    tok_small = rect.reshape(-1)[:int(small.sum())].contiguous()

    main_h = handle(ex)
    two_h = handle(ex, SCONE_FUSED_MAX_TOKENS=0)
    trav = {n: handle(ex, SCONE_VARLEN_T=n) for n in (128, 512, 2048)}       # the default: the whole stream as ONE row

    def rect_call(c, tok, pos=None):
        return lambda: c.embed_tokens(tok, wte=wte, wpe=wpe, position_ids=pos, out=out[:tok.numel()])

    def packed_call(c, tok, cu):
        return lambda: c.embed_tokens(tok, cu_seqlens=cu, wte=wte, wpe=wpe, out=out[:tok.numel()])

    variants = {
        "a": (main_h, rect_call(main_h, rect), B * T),
        "b": (main_h, rect_call(main_h, rect, pos_rect), B * T),
        "c": (main_h, packed_call(main_h, rect.reshape(-1), cu_equal), B * T),
        "d": (main_h, packed_call(main_h, packed, cu_rag), packed.numel()),
        "e": (main_h, rect_call(main_h, padded), B * T),
        "f1": (main_h, packed_call(main_h, tok_small, cu_small), tok_small.numel()),
        "f2": (two_h, packed_call(two_h, tok_small, cu_small), tok_small.numel()),
    }
    for n, c in trav.items():
        tag = str(n)
        variants[f"c_T{tag}"] = (c, packed_call(c, rect.reshape(-1), cu_equal), B * T)
        variants[f"d_T{tag}"] = (c, packed_call(c, packed, cu_rag), packed.numel())

    # same bits whatever the entry point and the traversal
    variants["a"][1]()
    want = out.clone()
    for name in ("c", "c_T128", "c_T512", "c_T2048"):
        out.fill_(float("nan"))
        variants[name][1]()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), name
    del want

    res = {k: {"step_us": [], "match_us": []} for k in variants}
    for _ in range(rounds):
        for name, (c, call, ntok) in variants.items():
            table = c.table
            for _ in range(2):                                            # warm-up of THIS variant's shapes, discarded
                call()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for e0, e1 in ev:
                e0.record()
                call()
                e1.record()
            torch.cuda.synchronize()
            res[name]["step_us"] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
            table.profile_enable(True)
            table.profile_read(reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                call()
            e1.record()
            torch.cuda.synchronize()
            _, kernel_ms = table.profile_read(reset=True)
            table.profile_enable(False)
            res[name]["match_us"].append((e0.elapsed_time(e1) - kernel_ms) / steps * 1e3)
            assert table.status() == 0, name

    med = {k: {"tokens": variants[k][2], "step_us": float(np.median(v["step_us"])), "step_us_min": float(np.min(v["step_us"])),
               "step_us_max": float(np.max(v["step_us"])), "timed_steps": len(v["step_us"]),
               "match_us": float(np.median(v["match_us"]))} for k, v in res.items()}
    s = lambda k: med[k]["step_us"]
    report = {
        "table": "1M-row INT8, d=768, max_n=3, fp16 out, wte + wpe; 2048 sequences",
        "ragged_tokens": int(packed.numel()), "rectangle_tokens": B * T,
        "variants": med,
        "ratios": {"c/b": s("c") / s("b"), "c/a": s("c") / s("a"), "d/e": s("d") / s("e"), "b/a": s("b") / s("a"),
                   "d/c": s("d") / s("c"), "match c/b": med["c"]["match_us"] / med["b"]["match_us"],
                   "f1/f2 (one launch / two kernels, 4096 ragged tokens)": s("f1") / s("f2")},
        "traversal_c_step_us": {k: s(k) for k in med if k == "c" or k.startswith("c_T")},
        "traversal_d_step_us": {k: s(k) for k in med if k == "d" or k.startswith("d_T")},
    }
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
