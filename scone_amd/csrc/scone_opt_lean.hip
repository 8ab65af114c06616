// The lean optimizer step (include/scone_hip.h, "lean optimizer step"): plain SGD or row-wise Adagrad -- ONE fp32 accumulator per
// row -- on an fp32 master row (master mode: the served row is re-stored in the table's format, as k_opt_step does) or on the
// served fp32 / bf16 row itself (in-place mode: no master copy; bf16 rows rounded to nearest or stochastically).
//
// Shape.  k_opt_step's: one wave per listed row, a grid-stride loop over the list, lane l owns the 16-byte pieces l, l + 64, ..
// of g (and the 8-byte pieces of a bf16 row: the same elements), blocks of OPT_NT * 64 pieces with the loads of a block issued
// before its arithmetic.  Row-wise Adagrad needs q, the row's sum of g1 * g1, before the first update: a row of up to 1024
// elements is one block whose g stays in registers; a wider row walks g twice (the second walk re-reads what this wave has just
// read).  Either way a lane adds its elements in ascending j, so block boundaries cannot change a bit; the lanes are combined by
// the butterfly the contract states.  The row's accumulator is read and written by lane 0; s' reaches the other lanes by a shuffle.
//
// Arithmetic.  Every operation is one IEEE fp32 rounding: built with -ffp-contract=off, nothing here calls fmaf, sqrtf and / are
// hipcc's correctly rounded defaults and subnormals are kept (tests/test_gpu_opt_lean.py pins all of it).  The stores of every
// row format are scone_opt_rows.h's, shared with k_opt_step.  Plain vector stores only; the one atomic is the integer atomicOr
// on the status word.
#include "scone_opt_lean.h"

namespace {

// NSRC (scone_opt_rows.h): n by value, or the count scone_opt_step_lean_dn reads from the device.  SSRC (scone_opt_rows.h): the
// scalars and the random bits' seed and step by value, or read from the scone_opt_hyper block of scone_opt_step_lean_dh -- a
// block whose last advance did not apply ends the wave before it touches anything.
template <int FMT, int KIND, bool INPLACE, bool STOCH, typename NSRC, typename SSRC>
__global__ __launch_bounds__(256) void k_opt_lean(const int64_t *__restrict__ ids, const float *__restrict__ grad,
                                                  NSRC nsrc, unsigned long long row_begin, unsigned long long row_end,
                                                  int d, SSRC ssrc, lean_rand rnd, float *__restrict__ master,
                                                  float *__restrict__ row_state, scone_row_store st, __half *__restrict__ scales,
                                                  uint32_t *__restrict__ status, const scone_grad_ctl *__restrict__ ctl) {
  scone_opt_scalars sc;
  if (!ssrc.load(sc)) return;
  if (STOCH) ssrc.rand(rnd);
  // scone_opt_step_lean_ctl (ctl != null; wave-uniform): as in k_opt_step -- a set skip flag ends the wave before it touches
  // anything; else the block's coef joins gscale by one fp32 product
  if (ctl) {
    if (ctl->skip != 0u) return;
    sc.gscale = opt_uniform(sc.gscale * ctl->coef);
  }
  const unsigned long long n = nsrc.get();
  static_assert(!INPLACE || FMT == SCONE_FMT_F32 || FMT == SCONE_FMT_BF16, "only fp32 and bf16 rows are weights in place");
  static_assert(!STOCH || (INPLACE && FMT == SCONE_FMT_BF16), "only an in-place bf16 row is rounded");
  constexpr bool ROWWISE = KIND == SCONE_LEAN_ROWWISE_ADAGRAD;
  const int lane = threadIdx.x & 63;
  const int pieces = d >> 2;
  const bool one_block = pieces <= OPT_NT * 64;
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
    // the weights: the master row, or the served row itself
    float4 *W = INPLACE ? reinterpret_cast<float4 *>(st.row(lr)) : reinterpret_cast<float4 *>(master + lr * (unsigned long long)d);
    uint2 *W16 = reinterpret_cast<uint2 *>(st.row(lr));  // an in-place bf16 row: piece p is 8 bytes
    const uint32_t row_key = STOCH ? scone_lean_row_key(rnd.seed, rnd.step, (uint64_t)id) : 0u;

    float4 g[OPT_NT], w[OPT_NT];
    bool on[OPT_NT];
    auto load_block = [&](int p0) {  // both streams of a block in flight before any arithmetic
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        on[t] = p < pieces;
        g[t] = w[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on[t]) {
          g[t] = G[p];
          if (INPLACE && FMT == SCONE_FMT_BF16) {
            const uint2 b = W16[p];
            w[t] = make_float4(__uint_as_float(b.x << 16), __uint_as_float(b.x & 0xFFFF0000u), __uint_as_float(b.y << 16),
                               __uint_as_float(b.y & 0xFFFF0000u));
          } else {
            w[t] = W[p];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) lean_scale4(sc, g[t]);
    };

    float den = 0.f;
    if (ROWWISE) {
      float q = 0.f;
      if (one_block) {
        load_block(0);
#pragma unroll
        for (int t = 0; t < OPT_NT; ++t) q = lean_sum_sq(q, g[t]);
      } else {
        for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
          float4 x[OPT_NT];
#pragma unroll
          for (int t = 0; t < OPT_NT; ++t) {
            const int p = p0 + t * 64 + lane;
            x[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < pieces) x[t] = G[p];
          }
#pragma unroll
          for (int t = 0; t < OPT_NT; ++t) {
            lean_scale4(sc, x[t]);
            q = lean_sum_sq(q, x[t]);
          }
        }
      }
      for (int s = 32; s >= 1; s >>= 1) q = q + __shfl_xor(q, s, 64);  // the contract's butterfly: every lane ends with the same bits
      float s_new = 0.f;
      if (lane == 0) {
        const float g2 = q / (float)d;
        s_new = row_state[lr] + g2;
        row_state[lr] = s_new;
      }
      s_new = __shfl(s_new, 0, 64);
      den = sqrtf(s_new) + sc.eps;
    }

    float rowmax = 0.f;  // INT8 only
    for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
      if (!(ROWWISE && one_block)) load_block(p0);
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        w[t].x = lean_elem<KIND>(sc, g[t].x, w[t].x, den);
        w[t].y = lean_elem<KIND>(sc, g[t].y, w[t].y, den);
        w[t].z = lean_elem<KIND>(sc, g[t].z, w[t].z, den);
        w[t].w = lean_elem<KIND>(sc, g[t].w, w[t].w, den);
      }
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        if (!INPLACE && on[t]) W[p] = w[t];
        if (STOCH) {
          const uint32_t j = (uint32_t)p << 2;
          if (on[t])
            W16[p] = make_uint2(lean_bf16_stochastic(w[t].x, row_key, j) | (lean_bf16_stochastic(w[t].y, row_key, j + 1) << 16),
                                lean_bf16_stochastic(w[t].z, row_key, j + 2) | (lean_bf16_stochastic(w[t].w, row_key, j + 3) << 16));
        } else if (FMT == SCONE_FMT_I8) {
          if (on[t]) rowmax = opt_i8_amax(rowmax, w[t]);
        } else if (p0 + t * 64 < pieces) {  // wave-uniform: a pass with no piece at all has no shuffles either
          opt_store_piece<FMT>(st, scales, lr, d, p, on[t], w[t], lane);
        }
      }
      if (FMT == SCONE_FMT_I8 && one_block) opt_i8_store_block(st, scales, lr, p0, lane, on, w, rowmax);
    }
    if (FMT == SCONE_FMT_I8 && !one_block) opt_i8_store_wide(st, scales, lr, W, pieces, lane, rowmax);
  }
}

struct lean_args {
  const int64_t *ids;
  const float *grad;
  unsigned long long n;  // the row count; the cap of the count on the device in the _dn and _dh forms
  scone_opt_scalars sc;  // by value, with rnd's seed and step; not read in the _dh form
  lean_rand rnd;
  float *master, *row_state;
};

// the one launch site: the kind, then the sources of the call's form (scone_opt_rows.h), select the instantiation
template <int FMT, bool INPLACE, bool STOCH>
void lean_launch(scone_handle *h, int kind, const opt_call &c, const lean_args &a, unsigned blocks, hipStream_t s) {
  auto launch = [&](auto K) {
    opt_with_sources(c, a.n, a.sc, [&](auto nsrc, auto ssrc) {
      hipLaunchKernelGGL((k_opt_lean<FMT, decltype(K)::value, INPLACE, STOCH, decltype(nsrc), decltype(ssrc)>), dim3(blocks), dim3(256),
                         0, s, a.ids, a.grad, nsrc, (unsigned long long)h->cfg.row_begin, (unsigned long long)h->cfg.row_end,
                         h->cfg.dim, ssrc, a.rnd, a.master, a.row_state, scone_store_of(h), (__half *)h->scales, h->d_status, c.d_ctl);
    });
  };
  if (kind == SCONE_LEAN_SGD)
    launch(std::integral_constant<int, SCONE_LEAN_SGD>());
  else
    launch(std::integral_constant<int, SCONE_LEAN_ROWWISE_ADAGRAD>());
}

}  // namespace

extern "C" int scone_lean_scalars_of(const scone_lean_cfg *cfg, scone_opt_scalars *out) {
  if (!out || lean_check(cfg)) return SCONE_EINVAL;
  lean_scalars(cfg, out);
  return SCONE_OK;
}

extern "C" uint32_t scone_lean_rand16(uint64_t seed, int64_t step, uint64_t row_id, uint32_t col) {
  return scone_lean_rand16_of(scone_lean_row_key(seed, step, row_id), col);
}

namespace {

// every form of scone_opt_step_lean: c says which (scone_opt_rows.h); cfg is null in the _dh form, n the cap in the _dn and _dh forms
int opt_step_lean(scone_handle *h, const opt_call &c, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                  uint64_t n, float *d_master, float *d_row_state, scone_stream_t stream) {
  const int kind = c.with_hyper ? c.kind : cfg ? cfg->kind : 0;
  const int rounding = c.with_hyper ? c.rounding : cfg ? cfg->rounding : 0;
  const char *bad_cfg = !c.with_hyper ? lean_check(cfg)
                        : kind != SCONE_LEAN_SGD && kind != SCONE_LEAN_ROWWISE_ADAGRAD              ? "bad kind"
                        : rounding != SCONE_ROUND_NEAREST && rounding != SCONE_ROUND_STOCHASTIC ? "bad rounding"
                                                                                                : nullptr;
  SCONE_TRY(opt_open(h, c, bad_cfg));
  const int fmt = h->cfg.table_fmt;
  const bool inplace = d_master == nullptr, stoch = rounding == SCONE_ROUND_STOCHASTIC;
  SCONE_TRY(lean_inplace_check(h, c.who, stoch, !inplace, true));
  if (n == 0) return SCONE_OK;
  if (!d_row_ids || !d_grad_rows) return scone_refuse(h, SCONE_EINVAL, c.who, "null pointer");
  if (kind == SCONE_LEAN_ROWWISE_ADAGRAD && !d_row_state)
    return scone_refuse(h, SCONE_EINVAL, c.who, "row-wise Adagrad needs d_row_state (one fp32 per owned row)");
  SCONE_ON_DEVICE(h);
  lean_args a;
  a.ids = d_row_ids, a.grad = d_grad_rows, a.n = n, a.master = d_master, a.row_state = d_row_state;
  a.rnd = lean_rand{0, 0}, a.sc = scone_opt_scalars{};
  if (!c.with_hyper) {
    a.rnd.seed = cfg->seed, a.rnd.step = cfg->step;
    lean_scalars(cfg, &a.sc);
  }
  const unsigned blocks = opt_begin(h, n);
  hipStream_t s = (hipStream_t)stream;
  if (inplace) {
    if (fmt == SCONE_FMT_F32)
      lean_launch<SCONE_FMT_F32, true, false>(h, kind, c, a, blocks, s);
    else if (stoch)
      lean_launch<SCONE_FMT_BF16, true, true>(h, kind, c, a, blocks, s);
    else
      lean_launch<SCONE_FMT_BF16, true, false>(h, kind, c, a, blocks, s);
  } else if (scone_dispatch_fmt(fmt, [&](auto F) { lean_launch<decltype(F)::value, false, false>(h, kind, c, a, blocks, s); })) {
    return scone_refuse(h, SCONE_EINVAL, c.who, "bad format");
  }
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

}  // namespace

extern "C" int scone_opt_step_lean(scone_handle *h, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                                   uint64_t n, float *d_master, float *d_row_state, scone_stream_t stream) {
  return opt_step_lean(h, {.who = "scone_opt_step_lean"}, cfg, d_row_ids, d_grad_rows, n, d_master, d_row_state, stream);
}

extern "C" int scone_opt_step_lean_ctl(scone_handle *h, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                                       uint64_t n, float *d_master, float *d_row_state, const scone_grad_ctl *d_ctl,
                                       scone_stream_t stream) {
  return opt_step_lean(h, {.who = "scone_opt_step_lean_ctl", .d_ctl = d_ctl, .need_ctl = true}, cfg, d_row_ids, d_grad_rows, n, d_master,
                       d_row_state, stream);
}

extern "C" int scone_opt_step_lean_dn(scone_handle *h, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                                      const uint64_t *d_n, uint64_t n_cap, float *d_master, float *d_row_state,
                                      const scone_grad_ctl *d_ctl, scone_stream_t stream) {
  return opt_step_lean(h, {.who = "scone_opt_step_lean_dn", .d_ctl = d_ctl, .d_n = d_n, .with_n = true}, cfg, d_row_ids, d_grad_rows, n_cap,
                       d_master, d_row_state, stream);
}

extern "C" int scone_opt_step_lean_dh(scone_handle *h, int32_t kind, int32_t rounding, const int64_t *d_row_ids, const float *d_grad_rows,
                                      const uint64_t *d_n, uint64_t n_cap, float *d_master, float *d_row_state,
                                      const scone_opt_hyper *d_hyper, const scone_grad_ctl *d_ctl, void *stream) {
  return opt_step_lean(h, {.who = "scone_opt_step_lean_dh", .d_ctl = d_ctl, .d_n = d_n, .with_n = true, .d_hyper = d_hyper,
                           .with_hyper = true, .kind = kind, .rounding = rounding},
                       nullptr, d_row_ids, d_grad_rows, n_cap, d_master, d_row_state, stream);
}
