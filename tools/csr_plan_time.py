"""Wall time of `SconeTable.backward_plan_csr` (the call with its synchronisations) on device-resident lists.

    [SCONE_HIP_LIB=other/libscone_hip.so] python tools/csr_plan_time.py [label]

One line per size: ntok positions with K = 3 uniform ids each over a 1M-row table (d = 8, fp16: the plan does not read a row),
median [min, max] of 15 calls after 3 warm-up calls.  To compare two builds of the library, run it once per build, each in a
process of its own, alternating (`profiles/r17a/csr_plan_time.txt`)."""

import sys
import time

import numpy as np
import torch

from scone_amd.hip_backend import SconeTable


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "library"
    n_rows, K = 1_000_000, 3
    table = SconeTable(3, n_rows, dim=8, table_format="fp16")
    rng = np.random.default_rng(0)
    for ntok in (4096, 65536, 1 << 20, 4 << 20):
        off = torch.arange(ntok + 1, dtype=torch.int32, device="cuda") * K
        ids = torch.from_numpy(rng.integers(0, n_rows, size=ntok * K).astype(np.int32)).cuda()
        times = []
        for it in range(18):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan = table.backward_plan_csr(off, ids)
            t1 = time.perf_counter()
            refs = plan.n_refs
            plan.close()
            if it >= 3:
                times.append((t1 - t0) * 1e3)
        assert refs == ntok * K and table.status() == 0
        print(f"{label:10s} ntok {ntok:8d} refs {refs:9d} plan {np.median(times):8.3f} ms [{min(times):.3f}, {max(times):.3f}]", flush=True)


if __name__ == "__main__":
    main()
