// What the two optimizer kernels share -- k_opt_step (scone_opt.hip) and k_opt_lean (scone_opt_lean.hip): how one wave turns the
// fp32 pieces of an updated row into the served table's bytes, and the random bits of the stochastic bf16 rounding.
//
// Lane l of the wave owns the 16-byte pieces l, l + 64, .. of a row (piece p = elements 4p .. 4p + 3); a row is walked in blocks
// of OPT_NT * 64 pieces.  fp32 / fp16 / bf16 pieces are stored on their own; an INT4 group (32 lanes of one piece pass) and an
// MXFP4 block (8 lanes) have their maximum inside one pass; INT8 needs the maximum of the whole row first: a row of up to one
// block stays in registers (opt_i8_store_block), a wider one is read back from the fp32 master row, every lane reading only the
// pieces it stored itself (opt_i8_store_wide).  The maxima are exact, so the lane mapping cannot show in the bits.  The element
// arithmetic is scone_quant.h's.
#pragma once

#include "scone_common.h"
#include "scone_quant.h"

#include <cmath>

constexpr int OPT_NT = 4;  // pieces per lane and block: 4 x 64 x 4 = 1024 elements

// ---- the host side both entry points open with
// the handle, then the cfg (bad_cfg: what the entry point's cfg check found, or null), then the table
static inline int opt_need_table(scone_handle *h, const char *who, const char *bad_cfg) {
  if (!h) return SCONE_EINVAL;
  if (bad_cfg) return scone_refuse(h, SCONE_EINVAL, who, bad_cfg);
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (!h->rows) return scone_refuse(h, SCONE_ESTATE, who, "handle has no table");
  return SCONE_OK;
}
// what scone_opt_step says of a cfg (null: nothing).  adam_needs_step false: scone_opt_hyper_init, whose step is the count of
// steps already applied and is checked there
static inline const char *opt_cfg_check(const scone_opt_cfg *cfg, bool adam_needs_step = true) {
  if (!cfg) return "null cfg";
  if (cfg->struct_size != sizeof(scone_opt_cfg)) return "cfg.struct_size does not match this library";
  if (cfg->kind != SCONE_OPT_SGD && cfg->kind != SCONE_OPT_ADAGRAD && cfg->kind != SCONE_OPT_ADAM) return "bad kind";
  if (!std::isfinite(cfg->lr) || !std::isfinite(cfg->beta1) || !std::isfinite(cfg->beta2) || !std::isfinite(cfg->eps) ||
      !std::isfinite(cfg->weight_decay) || !std::isfinite(cfg->grad_scale))
    return "lr, beta1, beta2, eps, weight_decay and grad_scale must be finite";
  if (adam_needs_step && cfg->kind == SCONE_OPT_ADAM && cfg->step < 1) return "Adam needs step >= 1";
  return nullptr;
}
// Which form of a step this is: what the by-value, _ctl, _dn and _dh entry points of both steps differ in.  The extern "C"
// wrappers fill it by designated fields; what a form does not have stays null / false.
struct opt_call {
  const char *who;                          // the entry point's name, for its refusals
  const scone_grad_ctl *d_ctl = nullptr;    // the control block; the kernel reads it when it is not null
  bool need_ctl = false;                    // _ctl: a null d_ctl is refused (beside a device count the block is optional)
  const uint64_t *d_n = nullptr;            // _dn, _dh: the count on the device, the call's n its cap
  bool with_n = false;
  const scone_opt_hyper *d_hyper = nullptr;  // _dh: the scalars on the device; the cfg is null and ...
  bool with_hyper = false;
  int32_t kind = 0, rounding = 0;           // ... these come by value in its place (rounding: the lean step's)
};
// the refusals every form of both steps opens with, in this order (bad_cfg: the unit's verdict on its cfg, or on the kind and
// rounding of a _dh call); the unit's own checks, the n == 0 early success and the data pointers follow
static inline int opt_open(scone_handle *h, const opt_call &c, const char *bad_cfg) {
  SCONE_TRY(opt_need_table(h, c.who, bad_cfg));
  if (c.need_ctl && !c.d_ctl) return scone_refuse(h, SCONE_EINVAL, c.who, "null d_ctl");
  if (c.with_n && !c.d_n) return scone_refuse(h, SCONE_EINVAL, c.who, "null d_n");
  if (c.with_hyper && !c.d_hyper) return scone_refuse(h, SCONE_EINVAL, c.who, "null d_hyper");
  return SCONE_OK;
}
// the table is about to change: as scone_table_store_f32_ids, the staged cache of cold rows is dropped.  Returns the grid for n
// listed rows, a wave each (SCONE_OPT_MAX_BLOCKS caps it)
static inline unsigned opt_begin(scone_handle *h, unsigned long long n) {
  if (h->stage) scone_stage_destroy(h);
  const unsigned blocks = scone_capped_blocks((n + 3) / 4);
  return h->opt_max_blocks > 0 && blocks > (unsigned long long)h->opt_max_blocks ? (unsigned)h->opt_max_blocks : blocks;
}

// Where a row-parallel kernel takes its row count from.  opt_n_value: the launch, as ever (one 8-byte kernel argument).
// opt_n_device (the _dn entry points): n = min(*d_n, n_cap), a count an earlier kernel of the stream left on the device; the
// address is a kernel argument, so the load is a scalar one that every wave makes before anything else.
struct opt_n_value {
  unsigned long long n;
  __device__ __forceinline__ unsigned long long get() const { return n; }
};
struct opt_n_device {
  const unsigned long long *d_n;
  unsigned long long n_cap;
  __device__ __forceinline__ unsigned long long get() const {
    const unsigned long long n = *d_n;
    return n < n_cap ? n : n_cap;
  }
};

// Where an optimizer kernel takes its scalars from.  opt_s_value: the launch, as ever (32 bytes of kernel arguments; the lean
// step's seed and step are the lean_rand argument beside it).  opt_s_device (the _dh entry points): the scone_opt_hyper block an
// earlier kernel of the stream (scone_opt_hyper_advance) left on the device.  Its address is a kernel argument and its fields
// are wave-uniform: every wave loads them once, before the row loop and before its first store, as *d_n is read.  load() is
// false when the block says the step was not applied: the wave then ends before it touches anything.  (The compiler keeps the
// eight scalars' load behind that branch, whatever order the source states: a wave of the _dh kernels waits for one more
// scalar-load round trip than a wave of the _dn kernels before its first row -- 0.4 us of a 22 us launch, nothing at size.)
struct opt_s_value {
  scone_opt_scalars sc;
  __device__ __forceinline__ bool load(scone_opt_scalars &out) const {
    out = sc;
    return true;
  }
  template <typename RND>
  __device__ __forceinline__ void rand(RND &) const {}
};
struct opt_s_device {
  const scone_opt_hyper *__restrict__ hy;
  __device__ __forceinline__ bool load(scone_opt_scalars &out) const {
    if (hy->applied == 0u) return false;
    out = hy->sc;
    return true;
  }
  template <typename RND>
  __device__ __forceinline__ void rand(RND &r) const {
    r.seed = hy->seed;
    r.step = hy->step;
  }
};

// The sources of a call (host side): launch(nsrc, ssrc) is called once, with the pair the form has -- count and scalars by value,
// the count on the device, or both on the device.  These three are every combination the kernels are instantiated for: there is
// no form with a by-value count beside scalars on the device.
template <typename F>
static inline void opt_with_sources(const opt_call &c, unsigned long long n, const scone_opt_scalars &sc, F &&launch) {
  const unsigned long long *d_n = reinterpret_cast<const unsigned long long *>(c.d_n);
  if (c.with_hyper)
    launch(opt_n_device{d_n, n}, opt_s_device{c.d_hyper});
  else if (c.with_n)
    launch(opt_n_device{d_n, n}, opt_s_value{sc});
  else
    launch(opt_n_value{n}, opt_s_value{sc});
}

// a wave-uniform float computed by the vector unit, put back where a kernel argument lives (a scalar register): the kernels read
// gscale in every element's statement, and the _ctl entry points replace it by a product
__device__ __forceinline__ float opt_uniform(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }

__device__ __forceinline__ uint32_t opt_i8_word(const float4 &x, float sf) {
  const float xs[4] = {x.x, x.y, x.z, x.w};
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) word |= (uint32_t)(uint8_t)(int8_t)(int)scone_q_elem(xs[k], sf, 127.f) << (8 * k);
  return word;
}

// The served-table bytes of piece p (elements 4p .. 4p + 3) of local row lr for the formats whose scale, if any, is known
// inside one piece pass.  Every lane of the wave calls this (the group maxima are shuffles); `on` guards the stores.
template <int FMT>
__device__ __forceinline__ void opt_store_piece(const scone_row_store &st, __half *__restrict__ scales, unsigned long long lr, int d,
                                                int p, bool on, const float4 &x, int lane) {
  uint8_t *row = st.row(lr);
  if (FMT == SCONE_FMT_F32) {
    if (on) reinterpret_cast<float4 *>(row)[p] = x;
  } else if (FMT == SCONE_FMT_F16) {
    const uint32_t a = __half_as_ushort(__float2half_rn(x.x)), b = __half_as_ushort(__float2half_rn(x.y));
    const uint32_t c = __half_as_ushort(__float2half_rn(x.z)), e = __half_as_ushort(__float2half_rn(x.w));
    if (on) reinterpret_cast<uint2 *>(row)[p] = make_uint2(a | (b << 16), c | (e << 16));
  } else if (FMT == SCONE_FMT_BF16) {
    if (on)
      reinterpret_cast<uint2 *>(row)[p] =
          make_uint2((uint32_t)scone_f32_to_bf16_bits(x.x) | ((uint32_t)scone_f32_to_bf16_bits(x.y) << 16),
                     (uint32_t)scone_f32_to_bf16_bits(x.z) | ((uint32_t)scone_f32_to_bf16_bits(x.w) << 16));
  } else if (FMT == SCONE_FMT_I4) {  // a group of 128 elements is 32 lanes of this pass
    float m = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
    for (int s = 16; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    const __half sh = scone_q_scale(m, 7.0f);
    const float sf = __half2float(sh);
    const int q[4] = {(int)scone_q_elem(x.x, sf, 7.f), (int)scone_q_elem(x.y, sf, 7.f), (int)scone_q_elem(x.z, sf, 7.f),
                      (int)scone_q_elem(x.w, sf, 7.f)};
    const uint32_t b0 = (uint32_t)((q[0] + 8) | ((q[1] + 8) << 4)) & 0xFFu, b1 = (uint32_t)((q[2] + 8) | ((q[3] + 8) << 4)) & 0xFFu;
    if (on) {
      reinterpret_cast<unsigned short *>(row)[p] = (unsigned short)(b0 | (b1 << 8));
      if ((lane & 31) == 0) scales[lr * (unsigned long long)(d / SCONE_I4_GROUP) + scone_i4_scale_slot(p >> 5, d)] = sh;
    }
  } else if (FMT == SCONE_FMT_MXFP4) {  // a block of 32 elements is 8 lanes of this pass
    const uint32_t uu[4] = {__float_as_uint(x.x), __float_as_uint(x.y), __float_as_uint(x.z), __float_as_uint(x.w)};
    uint32_t m = max(max(uu[0] & 0x7FFFFFFFu, uu[1] & 0x7FFFFFFFu), max(uu[2] & 0x7FFFFFFFu, uu[3] & 0x7FFFFFFFu));
    for (int s = 4; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    const uint32_t X = scone_mx_block_scale(m);
    const uint32_t nib[4] = {scone_mx_nibble(uu[0], X), scone_mx_nibble(uu[1], X), scone_mx_nibble(uu[2], X), scone_mx_nibble(uu[3], X)};
    if (on) {
      reinterpret_cast<unsigned short *>(row)[p] = (unsigned short)(nib[0] | (nib[1] << 4) | (nib[2] << 8) | (nib[3] << 12));
      if ((lane & 7) == 0)
        reinterpret_cast<uint8_t *>(scales)[lr * (unsigned long long)(d / SCONE_MX_BLOCK) + scone_mx_scale_slot(p >> 3, d)] = (uint8_t)X;
    }
  }
}

// INT8: one piece into the lane's running maximum
__device__ __forceinline__ float opt_i8_amax(float rowmax, const float4 &w) {
  return fmaxf(rowmax, fmaxf(fmaxf(fabsf(w.x), fabsf(w.y)), fmaxf(fabsf(w.z), fabsf(w.w))));
}

// INT8, the whole row is the block in registers (pieces <= OPT_NT * 64): scale and payload.  Every lane calls this.
__device__ __forceinline__ void opt_i8_store_block(const scone_row_store &st, __half *__restrict__ scales, unsigned long long lr, int p0,
                                                   int lane, const bool (&on)[OPT_NT], const float4 (&w)[OPT_NT], float rowmax) {
  const __half sh = scone_q_scale(scone_wave_max(rowmax), 127.0f);
  const float sf = __half2float(sh);
  uint32_t *o = reinterpret_cast<uint32_t *>(st.row(lr));
#pragma unroll
  for (int t = 0; t < OPT_NT; ++t)
    if (on[t]) o[p0 + t * 64 + lane] = opt_i8_word(w[t], sf);
  if (lane == 0) scales[lr] = sh;
}

// INT8, a wide row: read back from the master row W what THIS lane stored there.  Every lane calls this.
__device__ __forceinline__ void opt_i8_store_wide(const scone_row_store &st, __half *__restrict__ scales, unsigned long long lr,
                                                  const float4 *W, int pieces, int lane, float rowmax) {
  const __half sh = scone_q_scale(scone_wave_max(rowmax), 127.0f);
  const float sf = __half2float(sh);
  uint32_t *o = reinterpret_cast<uint32_t *>(st.row(lr));
  for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
    float4 x[OPT_NT];
#pragma unroll
    for (int t = 0; t < OPT_NT; ++t) {
      const int p = p0 + t * 64 + lane;
      if (p < pieces) x[t] = W[p];
    }
#pragma unroll
    for (int t = 0; t < OPT_NT; ++t) {
      const int p = p0 + t * 64 + lane;
      if (p < pieces) o[p] = opt_i8_word(x[t], sf);
    }
  }
  if (lane == 0) scales[lr] = sh;
}

// ---- the random bits of SCONE_ROUND_STOCHASTIC (include/scone_hip.h, "lean optimizer step"): 16 bits keyed by (seed, step,
// GLOBAL row id, column) and by nothing else -- never by list position, wave, grid or shard.  scone_lean_row_key is wave-uniform
// (six rounds per row); scone_lean_rand16_of adds the column: one round per element.
__host__ __device__ inline uint32_t scone_lean_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t scone_lean_row_key(uint64_t seed, int64_t step, uint64_t row_id) {
  const uint64_t t = (uint64_t)step;
  uint32_t h = 0x9E3779B9u;
  h = scone_lean_mix(h ^ (uint32_t)seed);
  h = scone_lean_mix(h ^ (uint32_t)(seed >> 32));
  h = scone_lean_mix(h ^ (uint32_t)t);
  h = scone_lean_mix(h ^ (uint32_t)(t >> 32));
  h = scone_lean_mix(h ^ (uint32_t)row_id);
  h = scone_lean_mix(h ^ (uint32_t)(row_id >> 32));
  return h;
}
__host__ __device__ inline uint32_t scone_lean_rand16_of(uint32_t row_key, uint32_t col) { return scone_lean_mix(row_key ^ col) >> 16; }
