// The fused sparse optimizer step (include/scone_hip.h, "optimizer step"): for every listed row, one wave reads the gradient
// row, the fp32 master row and the optimizer state, writes the updated master row and state in place and stores the row into
// the served table in the table's format -- exactly the bytes scone_table_store_f32_ids of the updated row would store.
//
// Shape.  One wave owns a row; lane l owns the 16-byte pieces l, l + 64, .. of every stream.  A row is walked in blocks of
// OPT_NT * 64 pieces (1024 elements): the loads of all streams of a block are issued before its arithmetic.  fp32 / fp16 / bf16
// rows are stored element by element.  INT4 groups (128 elements = 32 lanes of one piece pass) and MXFP4 blocks (32 elements =
// 8 lanes) have their maximum inside one pass: __shfl_xor over that many lanes, then the payload.  INT8 needs the maximum of the
// whole row before its first payload byte: rows of up to 1024 elements stay in registers (one block); wider rows are stored to
// the master first and read back, every lane reading only the pieces it stored itself -- no lane ever depends on another
// lane's global store.  The maxima are exact (no rounding), so the bits cannot depend on which lanes hold which elements.
//
// Arithmetic.  Every operation is one IEEE fp32 rounding: the library is built with -ffp-contract=off and nothing here calls
// fmaf; sqrtf and / are hipcc's correctly rounded defaults and subnormals are kept (tests/test_gpu_opt_step.py pins all of it).
// The element arithmetic of every row format is scone_quant.h's, shared with k_store_f32 (scone_table.hip); the GPU tests hold the
// two kernels together on every format.  Plain vector stores only; the one atomic is the integer atomicOr on the status word.
#include "scone_common.h"
#include "scone_opt_rows.h"  // the row stores shared with k_opt_lean
#include "scone_quant.h"

#include <cmath>

namespace {

// one element: the contract's statement, one rounding per operation
template <int KIND>
__device__ __forceinline__ void opt_elem(const scone_opt_scalars &k, float g, float &w, float &m, float &v) {
  const float g1 = k.gscale == 1.0f ? g : g * k.gscale;
  float w1 = w;
  if (k.decay != 0.0f) {
    const float dw = k.decay * w;
    w1 = w - dw;
  }
  if (KIND == SCONE_OPT_SGD) {
    const float s = k.alpha * g1;
    w = w1 - s;
  } else if (KIND == SCONE_OPT_ADAGRAD) {
    const float gg = g1 * g1;
    v = v + gg;
    const float num = k.alpha * g1;
    const float den = sqrtf(v) + k.eps;
    w = w1 - num / den;
  } else {
    const float a = k.b1 * m, b = k.c1 * g1;
    m = a + b;
    const float gg = g1 * g1;
    const float c = k.b2 * v, e = k.c2 * gg;
    v = c + e;
    const float num = k.alpha * m;
    const float den = sqrtf(v) + k.eps;
    w = w1 - num / den;
  }
}

// One wave per listed row; the grid-stride loop over rows is k_store_f32's.  NSRC (scone_opt_rows.h): n by value, or the count
// scone_opt_step_dn reads from the device.  SSRC (scone_opt_rows.h): the scalars by value, or the scone_opt_hyper block
// scone_opt_step_dh reads them from -- a block whose last advance did not apply ends the wave before it touches anything.
template <int FMT, int KIND, typename NSRC, typename SSRC>
__global__ __launch_bounds__(256) void k_opt_step(const int64_t *__restrict__ ids, const float *__restrict__ grad,
                                                  NSRC nsrc, unsigned long long row_begin, unsigned long long row_end,
                                                  int d, SSRC ssrc, float *__restrict__ master, float *__restrict__ state1,
                                                  float *__restrict__ state2, scone_row_store st, __half *__restrict__ scales,
                                                  uint32_t *__restrict__ status, const scone_grad_ctl *__restrict__ ctl) {
  scone_opt_scalars sc;
  if (!ssrc.load(sc)) return;
  // scone_opt_step_ctl (ctl != null; wave-uniform): a set skip flag ends the wave before it touches anything; else the block's
  // coef joins gscale by one fp32 product and the rest is the plain call with that gscale
  if (ctl) {
    if (ctl->skip != 0u) return;
    sc.gscale = opt_uniform(sc.gscale * ctl->coef);
  }
  const unsigned long long n = nsrc.get();
  constexpr bool HAS_M = KIND == SCONE_OPT_ADAM;
  constexpr bool HAS_V = KIND != SCONE_OPT_SGD;
  const int lane = threadIdx.x & 63;
  const int pieces = d >> 2;
  const unsigned long long nwaves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  for (unsigned long long r = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n; r += nwaves) {
    const long long id = ids[r];
    // wave-uniform: outside the owned range, or not above its predecessor in the list -> skipped, never an address
    if ((unsigned long long)id < row_begin || (unsigned long long)id >= row_end || (r > 0 && id <= ids[r - 1])) {
      if (lane == 0) atomicOr(status, SCONE_ST_BAD_ID);
      continue;
    }
    const unsigned long long lr = (unsigned long long)id - row_begin;
    const float4 *G = reinterpret_cast<const float4 *>(grad + r * (unsigned long long)d);
    float4 *W = reinterpret_cast<float4 *>(master + lr * (unsigned long long)d);
    float4 *M = HAS_M ? reinterpret_cast<float4 *>(state1 + lr * (unsigned long long)d) : nullptr;
    float4 *V = HAS_V ? reinterpret_cast<float4 *>(state2 + lr * (unsigned long long)d) : nullptr;
    float rowmax = 0.f;  // INT8 only
    for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
      float4 g[OPT_NT], w[OPT_NT], m[OPT_NT], v[OPT_NT];
      bool on[OPT_NT];
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        on[t] = p < pieces;
        g[t] = w[t] = m[t] = v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on[t]) {
          g[t] = G[p];
          w[t] = W[p];
          if (HAS_M) m[t] = M[p];
          if (HAS_V) v[t] = V[p];
        }
      }
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        opt_elem<KIND>(sc, g[t].x, w[t].x, m[t].x, v[t].x);
        opt_elem<KIND>(sc, g[t].y, w[t].y, m[t].y, v[t].y);
        opt_elem<KIND>(sc, g[t].z, w[t].z, m[t].z, v[t].z);
        opt_elem<KIND>(sc, g[t].w, w[t].w, m[t].w, v[t].w);
      }
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        if (on[t]) {
          W[p] = w[t];
          if (HAS_M) M[p] = m[t];
          if (HAS_V) V[p] = v[t];
        }
        if (FMT == SCONE_FMT_I8) {
          if (on[t]) rowmax = opt_i8_amax(rowmax, w[t]);
        } else if (p0 + t * 64 < pieces) {  // wave-uniform: a pass with no piece at all has no shuffles either
          opt_store_piece<FMT>(st, scales, lr, d, p, on[t], w[t], lane);
        }
      }
      if (FMT == SCONE_FMT_I8 && pieces <= OPT_NT * 64) opt_i8_store_block(st, scales, lr, p0, lane, on, w, rowmax);  // the row is in registers
    }
    if (FMT == SCONE_FMT_I8 && pieces > OPT_NT * 64) opt_i8_store_wide(st, scales, lr, W, pieces, lane, rowmax);
  }
}

void opt_scalars(const scone_opt_cfg *cfg, scone_opt_scalars *out) {
  double alpha = cfg->lr;
  if (cfg->kind == SCONE_OPT_ADAM) {
    const double t = (double)cfg->step;
    alpha = cfg->lr * std::sqrt(1.0 - std::pow(cfg->beta2, t)) / (1.0 - std::pow(cfg->beta1, t));
  }
  out->alpha = (float)alpha;
  out->b1 = (float)cfg->beta1;
  out->b2 = (float)cfg->beta2;
  out->c1 = (float)(1.0 - cfg->beta1);
  out->c2 = (float)(1.0 - cfg->beta2);
  out->eps = (float)cfg->eps;
  out->decay = (float)(cfg->lr * cfg->weight_decay);
  out->gscale = (float)cfg->grad_scale;
}

struct opt_args {
  const int64_t *ids;
  const float *grad;
  unsigned long long n;  // the row count; the cap of the count on the device in the _dn and _dh forms
  scone_opt_scalars sc;  // by value; not read in the _dh form
  float *master, *s1, *s2;
};

// the one launch site: the kind, then the sources of the call's form (scone_opt_rows.h), select the instantiation
template <int FMT>
void opt_launch(scone_handle *h, int kind, const opt_call &c, const opt_args &a, unsigned blocks, hipStream_t s) {
  auto launch = [&](auto K) {
    opt_with_sources(c, a.n, a.sc, [&](auto nsrc, auto ssrc) {
      hipLaunchKernelGGL((k_opt_step<FMT, decltype(K)::value, decltype(nsrc), decltype(ssrc)>), dim3(blocks), dim3(256), 0, s, a.ids,
                         a.grad, nsrc, (unsigned long long)h->cfg.row_begin, (unsigned long long)h->cfg.row_end, h->cfg.dim, ssrc,
                         a.master, a.s1, a.s2, scone_store_of(h), (__half *)h->scales, h->d_status, c.d_ctl);
    });
  };
  if (kind == SCONE_OPT_SGD)
    launch(std::integral_constant<int, SCONE_OPT_SGD>());
  else if (kind == SCONE_OPT_ADAGRAD)
    launch(std::integral_constant<int, SCONE_OPT_ADAGRAD>());
  else
    launch(std::integral_constant<int, SCONE_OPT_ADAM>());
}

}  // namespace

extern "C" int scone_opt_scalars_of(const scone_opt_cfg *cfg, scone_opt_scalars *out) {
  if (!out || opt_cfg_check(cfg)) return SCONE_EINVAL;
  opt_scalars(cfg, out);
  return SCONE_OK;
}

namespace {

// every form of scone_opt_step: c says which (scone_opt_rows.h); cfg is null in the _dh form, n the cap in the _dn and _dh forms
int opt_step(scone_handle *h, const opt_call &c, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows, uint64_t n,
             float *d_master, float *d_state1, float *d_state2, scone_stream_t stream) {
  const int kind = c.with_hyper ? c.kind : cfg ? cfg->kind : 0;
  const char *bad_cfg = !c.with_hyper ? opt_cfg_check(cfg)
                        : kind != SCONE_OPT_SGD && kind != SCONE_OPT_ADAGRAD && kind != SCONE_OPT_ADAM ? "bad kind" : nullptr;
  SCONE_TRY(opt_open(h, c, bad_cfg));
  if (n == 0) return SCONE_OK;
  if (!d_row_ids || !d_grad_rows || !d_master) return scone_refuse(h, SCONE_EINVAL, c.who, "null pointer");
  if (kind == SCONE_OPT_ADAM && !d_state1) return scone_refuse(h, SCONE_EINVAL, c.who, "Adam needs d_state1 (m)");
  if (kind != SCONE_OPT_SGD && !d_state2) return scone_refuse(h, SCONE_EINVAL, c.who, "Adam / Adagrad need d_state2 (v / the sum of squares)");
  SCONE_ON_DEVICE(h);
  opt_args a;
  a.ids = d_row_ids, a.grad = d_grad_rows, a.n = n, a.master = d_master, a.s1 = d_state1, a.s2 = d_state2;
  a.sc = scone_opt_scalars{};
  if (!c.with_hyper) opt_scalars(cfg, &a.sc);
  const unsigned blocks = opt_begin(h, n);
  const int bad = scone_dispatch_fmt(h->cfg.table_fmt, [&](auto F) { opt_launch<decltype(F)::value>(h, kind, c, a, blocks, (hipStream_t)stream); });
  if (bad) return scone_refuse(h, SCONE_EINVAL, c.who, "bad format");
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

}  // namespace

extern "C" int scone_opt_step(scone_handle *h, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows, uint64_t n,
                              float *d_master, float *d_state1, float *d_state2, scone_stream_t stream) {
  return opt_step(h, {.who = "scone_opt_step"}, cfg, d_row_ids, d_grad_rows, n, d_master, d_state1, d_state2, stream);
}

extern "C" int scone_opt_step_ctl(scone_handle *h, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                                  uint64_t n, float *d_master, float *d_state1, float *d_state2, const scone_grad_ctl *d_ctl,
                                  scone_stream_t stream) {
  return opt_step(h, {.who = "scone_opt_step_ctl", .d_ctl = d_ctl, .need_ctl = true}, cfg, d_row_ids, d_grad_rows, n, d_master, d_state1,
                  d_state2, stream);
}

extern "C" int scone_opt_step_dn(scone_handle *h, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                                 const uint64_t *d_n, uint64_t n_cap, float *d_master, float *d_state1, float *d_state2,
                                 const scone_grad_ctl *d_ctl, scone_stream_t stream) {
  return opt_step(h, {.who = "scone_opt_step_dn", .d_ctl = d_ctl, .d_n = d_n, .with_n = true}, cfg, d_row_ids, d_grad_rows, n_cap, d_master,
                  d_state1, d_state2, stream);
}

extern "C" int scone_opt_step_dh(scone_handle *h, int32_t kind, const int64_t *d_row_ids, const float *d_grad_rows, const uint64_t *d_n,
                                 uint64_t n_cap, float *d_master, float *d_state1, float *d_state2, const scone_opt_hyper *d_hyper,
                                 const scone_grad_ctl *d_ctl, void *stream) {
  return opt_step(h, {.who = "scone_opt_step_dh", .d_ctl = d_ctl, .d_n = d_n, .with_n = true, .d_hyper = d_hyper, .with_hyper = true,
                      .kind = kind},
                  nullptr, d_row_ids, d_grad_rows, n_cap, d_master, d_state1, d_state2, stream);
}
