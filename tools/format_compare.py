#!/usr/bin/env python3
"""A new table format against its twin, gather kernel only.  Two pairs:

  bf16 / fp16   (default) the text below
  mxfp4 / int4  `python tools/format_compare.py out.json 4 30 mxfp4`: 1M rows, d = 1024, synthetic fill in either format (the same
                payload words; INT4 with its fp16 group scales, MXFP4 with its E8M0 block scales -- different VALUES, the same
                access pattern), otherwise the same procedure.  The MXFP4 row is 3 % larger (544 against 528 B), so the bar is
                mxfp4 / int4 <= 1.03 + INT4's own spread of block medians in this run; a ratio below 1 means the cheaper
                decode (two elements per convert) is visible.

The bf16 table format against fp16, gather kernel only, on C2's shape: 1M rows, d = 768, 2048 x 512 tokens, a different batch
every step, fp16 out, wte + wpe.  One process; an fp16 and a bf16 table filled from the same synthetic rows (the same fp32
value rounded to either format), one output buffer shared by both (the kernel's time follows the buffer's placement:
profiles/r06m); the two tables alternate fp16 / bf16 / fp16 / bf16 / ... in blocks of `steps` lookups, each block after two
untimed ones; the gather kernel is timed by the library's own events (scone_profile_enable / scone_profile_samples).

Both formats move the same bytes, so the bar is fp16's own spread in this run: the median over the bf16 blocks' medians may
exceed fp16's by at most (max - min of fp16's block medians) / fp16's median.  The report holds every block's median, the two
figures and `within_bar`.

    python tools/format_compare.py [out.json] [blocks per format >= 4] [steps per block] [bf16 | mxfp4]
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

N, B, T = 1_000_000, 2048, 512
PAIRS = {"bf16": ("fp16", "bf16", 768, 0.0), "mxfp4": ("int4", "mxfp4", 1024, 0.03)}   # new format: twin, itself, d, allowance for row bytes


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    assert blocks >= 4 and steps >= 1
    old, new, D, allowance = PAIRS[sys.argv[4] if len(sys.argv) > 4 else "bf16"]
    warm = 2
    ex, keys, lens = make_vocabulary(N, "zipf")
    _, batches = make_batches(ex, keys, lens, "uniform", B, T, 1234, steps + warm)
    g = torch.Generator(device="cuda").manual_seed(5)
    wte = (torch.randn(S.GPT2_VOCAB, D, generator=g, device="cuda") * 0.02).half()
    wpe = (torch.randn(1024, D, generator=g, device="cuda") * 0.01).half()
    out = torch.empty(B, T, D, dtype=torch.float16, device="cuda")
    caches = {f: EmbeddingCache.from_synthetic(ex, D, table_format=f, seed=7, base_scale=0.02 / 127) for f in (old, new)}
    for c in caches.values():
        c.table.reserve(B * T)
    # the two tables hold the same rows up to their format's rounding
    ids = torch.arange(0, N, 9973)
    a, b = (caches[f].table.gather_rows(ids) for f in (old, new))
    if new == "bf16":
        assert torch.allclose(a, b, rtol=2.0 ** -8, atol=2.0 ** -24), "the fp16 and the bf16 table hold different rows"
    else:
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and a.abs().max() < 1 and b.abs().max() < 1

    medians = {old: [], new: []}
    for _ in range(blocks):
        for f in (old, new):
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
    m16, mbf = float(np.median(medians[old])), float(np.median(medians[new]))
    spread = (max(medians[old]) - min(medians[old])) / m16
    report = {
        "workload": f"{N}-row table d={D} max_n=3 in HBM, S_uniform, {B}x{T} tokens/step, a different batch every step, fp16 out, "
                    f"wte + wpe; gather kernel (k_embed_wave) by the library's profile events",
        "blocks_per_format": blocks, "steps_per_block": steps, "order": f"{old}, {new}, {old}, {new}, ...",
        "block_median_kernel_ms": medians,
        f"{old}_median_ms": m16, f"{new}_median_ms": mbf, f"{new}_over_{old}": mbf / m16,
        f"{old}_spread": spread, "bar": f"{new}_over_{old} - 1 <= {allowance:g} + {old}_spread",
        "within_bar": bool(mbf / m16 - 1.0 <= allowance + spread),
    }
    if new == "mxfp4":
        report["row_bytes"] = {old: caches[old].table.payload_bytes() + caches[old].table.scale_bytes(),
                               new: caches[new].table.payload_bytes() + caches[new].table.scale_bytes()}
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
