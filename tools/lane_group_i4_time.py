"""Time of the lane-group kernel k_embed<INT4> behind scone_gather_reduce, one build per process.

    SCONE_HIP_LIB=<libscone_hip.so> python tools/lane_group_i4_time.py

launch_table_fmt (scone_embed_wave.h) sends caller-supplied lists to k_embed_csr_wave at d = 768 / 1024 / 1280 and to the
lane-group kernel k_embed<FMT, OutT, 0, 16, 6, SRC_CSR, MODE_FULL> at every other width: an INT4 table of d = 2048 is the
shape that launches the kernel whose nibble decode is row_codec<INT4>::add_word.  16384 lists of 6 ids into a 100,000-row
synthetic table, fp16 output; prints one JSON line: microseconds per call over 200 calls (one pair of events), after 20.
Run the two builds alternately, each in a fresh process, and compare the medians inside one session.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scone_amd import _lib  # noqa: E402
from scone_amd.hip_backend import SconeTable  # noqa: E402

N, D, NTOK, K, CALLS, WARMUP = 100_000, 2048, 16384, 6, 200, 20

keys = np.zeros((N, 3), dtype=np.uint32)
keys[:, 0] = np.arange(N)
t = SconeTable(3, N, D, "int4")
t.index_build(keys, np.ones(N, dtype=np.uint8))
t.fill_synthetic(5, 0.02)
rng = np.random.default_rng(21)
off = torch.arange(0, (NTOK + 1) * K, K, dtype=torch.int32, device="cuda")
ids = torch.from_numpy(rng.integers(0, N, size=NTOK * K).astype(np.int32)).cuda()
for _ in range(WARMUP):
    out = t.gather_reduce(off, ids, "mean", out_dtype=torch.float16)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(CALLS):
    out = t.gather_reduce(off, ids, "mean", out_dtype=torch.float16)
b.record()
torch.cuda.synchronize()
assert t.status() == 0
print(json.dumps({"lib": _lib.LIB_PATH, "us_per_call": round(a.elapsed_time(b) * 1e3 / CALLS, 2), "d": D, "lists": NTOK, "ids_per_list": K,
                  "checksum": float(out.float().abs().sum())}))
