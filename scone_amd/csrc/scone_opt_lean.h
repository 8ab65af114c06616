// What the lean optimizer step's kernels share -- k_opt_lean (scone_opt_lean.hip) and the fused backward + lean step
// (scone_backward_apply.hip): the per-element arithmetic of include/scone_hip.h, "lean optimizer step", one IEEE fp32 rounding per
// operation (the units are built with -ffp-contract=off and nothing here calls fmaf), and the host-side check of a scone_lean_cfg.
#pragma once

#include "scone_common.h"
#include "scone_opt_rows.h"
#include "scone_quant.h"

#include <cmath>

struct lean_rand {
  uint64_t seed;
  int64_t step;
};

__device__ __forceinline__ float lean_scale(const scone_opt_scalars &k, float g) { return k.gscale == 1.0f ? g : g * k.gscale; }

__device__ __forceinline__ void lean_scale4(const scone_opt_scalars &k, float4 &g) {
  g.x = lean_scale(k, g.x), g.y = lean_scale(k, g.y), g.z = lean_scale(k, g.z), g.w = lean_scale(k, g.w);
}

// a lane's part of q: its elements in ascending j, the product rounded first, then the sum.  A piece the lane does not have is
// all +0.0f: q + (+0.0f * +0.0f) keeps every bit of q (q is never -0.0f: it starts at +0.0f and only squares are added)
__device__ __forceinline__ float lean_sum_sq(float q, const float4 &g1) {
  const float a = g1.x * g1.x, b = g1.y * g1.y, c = g1.z * g1.z, e = g1.w * g1.w;
  q = q + a;
  q = q + b;
  q = q + c;
  q = q + e;
  return q;
}

// one element from g1 (already scaled): the contract's statement, one rounding per operation
template <int KIND>
__device__ __forceinline__ float lean_elem(const scone_opt_scalars &k, float g1, float w, float den) {
  float w1 = w;
  if (k.decay != 0.0f) {
    const float dw = k.decay * w;
    w1 = w - dw;
  }
  const float num = k.alpha * g1;
  if (KIND == SCONE_LEAN_SGD) return w1 - num;
  return w1 - num / den;
}

// SCONE_ROUND_STOCHASTIC of one element: (u + r) >> 16, r = 16 random bits; an inf / NaN is rounded as nearest does
__device__ __forceinline__ uint32_t lean_bf16_stochastic(float x, uint32_t row_key, uint32_t col) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7F800000u) == 0x7F800000u) return scone_f32_to_bf16_bits(x);
  return (u + scone_lean_rand16_of(row_key, col)) >> 16;
}

// ---- host side
static inline const char *lean_check(const scone_lean_cfg *cfg) {
  if (!cfg) return "null cfg";
  if (cfg->struct_size != sizeof(scone_lean_cfg)) return "cfg.struct_size does not match this library";
  if (cfg->kind != SCONE_LEAN_SGD && cfg->kind != SCONE_LEAN_ROWWISE_ADAGRAD) return "bad kind";
  if (cfg->rounding != SCONE_ROUND_NEAREST && cfg->rounding != SCONE_ROUND_STOCHASTIC) return "bad rounding";
  if (cfg->reserved != 0) return "cfg.reserved must be 0";
  if (!std::isfinite(cfg->lr) || !std::isfinite(cfg->eps) || !std::isfinite(cfg->weight_decay) || !std::isfinite(cfg->grad_scale))
    return "lr, eps, weight_decay and grad_scale must be finite";
  return nullptr;
}

// The mode refusals of a lean step, for the handle's table format: in place (no master) the rows must be fp32 or bf16, and only
// in-place bf16 rows have anything to round.  master_wording: scone_opt_step_lean names its d_master argument in the first text;
// scone_backward_apply_lean, which is always in place, has none
static inline int lean_inplace_check(scone_handle *h, const char *who, bool stoch, bool has_master, bool master_wording) {
  const int fmt = h->cfg.table_fmt;
  if (!has_master && fmt != SCONE_FMT_F32 && fmt != SCONE_FMT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who,
                        (std::string(master_wording ? "in place (d_master == NULL)" : "in place") +
                         " needs an fp32 or bf16 table, this one is " + scone_fmt_name(fmt))
                            .c_str());
  if (stoch && has_master)
    return scone_refuse(h, SCONE_EINVAL, who, "stochastic rounding with a master: there is nothing to round");
  if (stoch && fmt != SCONE_FMT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who, "stochastic rounding on an fp32 table: there is nothing to round");
  return SCONE_OK;
}

static inline void lean_scalars(const scone_lean_cfg *cfg, scone_opt_scalars *out) {
  *out = scone_opt_scalars{};
  out->alpha = (float)cfg->lr;
  out->eps = (float)cfg->eps;
  out->decay = (float)(cfg->lr * cfg->weight_decay);
  out->gscale = (float)cfg->grad_scale;
}
