#!/bin/bash
# Lists every k_embed_wave / k_embed_fused / k_embed_select / k_embed_rows / k_match_ell / k_bwd_chunks / k_bwd_combine (and their _dn forms) /
# k_bwd_head_dn / k_opt_step / k_opt_lean (by value, _dn and _dh forms) / k_opt_hyper_* /
# k_bwd_partials / k_bwd_apply / k_grad_* instantiation that uses
# scratch memory (register spills):
# a spill inside the per-token loop turns into HBM traffic (WRITE_SIZE +2 % and -5 % speed on the INT4 kernel before
# the occupancy estimate of scone_embed_wave.h accounted for its scale registers).  CPU only (hipcc -S).
cd "$(dirname "$0")/../scone_amd/csrc" || exit 1
rc=0
for src in scone_gather_i8 scone_gather_i4 scone_gather_f16 scone_gather_f32 scone_gather_bf16 scone_gather_mxfp4 scone_index \
           scone_select_f32 scone_select_f16 scone_select_i8 scone_select_i4 scone_select_bf16 scone_select_mxfp4 scone_rows_f32 scone_rows_f16 scone_rows_bf16 scone_backward scone_backward_dn scone_backward_apply scone_opt scone_opt_lean scone_opt_hyper scone_grad_norm; do
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S $src.hip -o /tmp/$src.s 2>/dev/null || { echo "compile failed: $src"; exit 1; }
  python3 - /tmp/$src.s $src <<'PY' || rc=1
import re, sys
name, vg, bad = None, None, 0
for line in open(sys.argv[1]):
    m = re.match(r"^(_Z\S+):", line)
    if m:
        name = m.group(1)
    elif "; NumVgprs:" in line:
        vg = int(line.split()[-1])
    elif "; ScratchSize:" in line:
        sc = int(line.split()[-1])
        if sc and name and any(k in name for k in ("k_embed_wave", "k_embed_fused", "k_embed_select", "k_embed_rows", "k_embed_csr_wave", "k_match_ell", "k_bwd_chunks", "k_bwd_combine", "k_bwd_head", "k_opt_step", "k_opt_lean", "k_opt_hyper", "k_bwd_partials", "k_bwd_apply", "k_grad_")):
            print(f"{sys.argv[2]}: scratch {sc} B/lane, {vg} VGPRs: {name[:110]}")
            bad += 1
sys.exit(1 if bad else 0)
PY
done
[ $rc = 0 ] && echo "no wave kernel uses scratch"
exit $rc
