#!/usr/bin/env python3
"""The bf16 table format against fp16, gather kernel only, on C2's shape: 1M rows, d = 768, 2048 x 512 tokens, a different batch
every step, fp16 out, wte + wpe.  One process; an fp16 and a bf16 table filled from the same synthetic rows (the same fp32
value rounded to either format), one output buffer shared by both (the kernel's time follows the buffer's placement:
profiles/r06m); the two tables alternate fp16 / bf16 / fp16 / bf16 / ... in blocks of `steps` lookups, each block after two
untimed ones; the gather kernel is timed by the library's own events (scone_profile_enable / scone_profile_samples).

Both formats move the same bytes, so the bar is fp16's own spread in this run: the median over the bf16 blocks' medians may
exceed fp16's by at most (max - min of fp16's block medians) / fp16's median.  The report holds every block's median, the two
figures and `within_bar`.

    python tools/format_compare.py [out.json] [blocks per format >= 4] [steps per block]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from benchkit.workloads import make_batches, make_vocabulary
from scone_amd import EmbeddingCache
from scone_amd import synthetic as S

N, B, T, D = 1_000_000, 2048, 512, 768


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    assert blocks >= 4 and steps >= 1
    warm = 2
    ex, keys, lens = make_vocabulary(N, "zipf")
    _, batches = make_batches(ex, keys, lens, "uniform", B, T, 1234, steps + warm)
    g = torch.Generator(device="cuda").manual_seed(5)
    wte = (torch.randn(S.GPT2_VOCAB, D, generator=g, device="cuda") * 0.02).half()
    wpe = (torch.randn(1024, D, generator=g, device="cuda") * 0.01).half()
    out = torch.empty(B, T, D, dtype=torch.float16, device="cuda")
    caches = {f: EmbeddingCache.from_synthetic(ex, D, table_format=f, seed=7, base_scale=0.02 / 127) for f in ("fp16", "bf16")}
    for c in caches.values():
        c.table.reserve(B * T)
    # the two tables hold the same rows up to their format's rounding
    ids = torch.arange(0, N, 9973)
    a, b = (caches[f].table.gather_rows(ids) for f in ("fp16", "bf16"))
    assert torch.allclose(a, b, rtol=2.0 ** -8, atol=2.0 ** -24), "the fp16 and the bf16 table hold different rows"

    medians = {"fp16": [], "bf16": []}
    for _ in range(blocks):
        for f in ("fp16", "bf16"):
            c, table = caches[f], caches[f].table
            for k in range(warm):
                c.embed_tokens(batches[k], wte=wte, wpe=wpe, out=out)
            table.profile_enable(True)
            table.profile_read(reset=True)
            for k in range(steps):
                c.embed_tokens(batches[warm + k], wte=wte, wpe=wpe, out=out)
            torch.cuda.synchronize()
            samples = table.profile_samples()
            table.profile_read(reset=True)
            table.profile_enable(False)
            assert len(samples) == steps and table.status() == 0, (f, len(samples))
            medians[f].append(float(np.median(samples)))
    m16, mbf = float(np.median(medians["fp16"])), float(np.median(medians["bf16"]))
    spread = (max(medians["fp16"]) - min(medians["fp16"])) / m16
    report = {
        "workload": f"{N}-row table d={D} max_n=3 in HBM, S_uniform, {B}x{T} tokens/step, a different batch every step, fp16 out, "
                    f"wte + wpe; gather kernel (k_embed_wave) by the library's profile events",
        "blocks_per_format": blocks, "steps_per_block": steps, "order": "fp16, bf16, fp16, bf16, ...",
        "block_median_kernel_ms": medians,
        "fp16_median_ms": m16, "bf16_median_ms": mbf, "bf16_over_fp16": mbf / m16,
        "fp16_spread": spread, "bar": "bf16_over_fp16 - 1 <= fp16_spread", "within_bar": bool(mbf / m16 - 1.0 <= spread),
    }
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
