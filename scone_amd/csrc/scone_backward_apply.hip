// The lookup's backward applied in place (include/scone_hip.h, "backward applied in place"): scone_backward_rows and the in-place
// scone_opt_step_lean in one pass, so that grad_rows -- fp32 [U, d], the one table-sized-per-batch array of in-place training --
// is never stored.  The table rows and the row state end with the bits the two calls leave.
//
// Shape.  One wave owns one touched row.  The work list is the plan's bwd_multi list followed by its chunk list: a chunk that is
// a whole row (partial == 0) is that row, `dest` its segment; a chunk of a longer row is skipped here -- k_bwd_partials, a first
// small launch, has written its partial slot, a wave per chunk, so a hot unigram's hundreds of chunks are walked in parallel --
// and the row's bwd_multi entry adds the partials in chunk order, as k_bwd_combine does.  The walk is scone_bwd_plan.h's, shared
// with k_bwd_chunks: 16-byte grad_out loads, 16 in flight per lane, `a = a + c` in reference order.
//
// The finished fp32 gradient row goes to LDS: d * 4 bytes that belong to this wave alone (dynamic LDS, 4 * d * 4 bytes per
// workgroup, 64 KB at d = 4096).  The walk's lane owns 8 consecutive fp16 / bf16 elements, the update's lane owns elements
// 4p .. 4p + 3 of piece p = lane, lane + 64, ..: the contract's map for the row sum.  LDS turns one into the other and keeps the
// wide loads.  Then the body of k_opt_lean's in-place instantiations runs with G pointing at LDS; the per-element arithmetic, the
// row sum and the random bits are scone_opt_lean.h's and scone_opt_rows.h's, shared with k_opt_lean.
//
// Waves of a workgroup have different trip counts, so there is no __syncthreads() anywhere: a wave's LDS writes are ordered
// before its own reads (and its reads before the next row's writes) by a wavefront-scope fence; the LDS executes one wave's
// operations in order.  Plain vector stores only and no atomic at all: plan rows are owned, distinct and ascending, so there is
// no id to check and no status bit to raise.
#include "scone_bwd_plan.h"
#include "scone_opt_lean.h"

#define SCONE_BWD_APPLY_MAX_DIM 4096  // 4 waves x d x 4 bytes of LDS: 64 KB

namespace {

constexpr int BWD_THREADS = 256;  // four waves, as k_bwd_chunks and k_opt_lean

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// First launch (only when the plan has rows with several chunks): k_bwd_chunks restricted to those rows' chunks.
template <int DT, int NT, bool MEAN>
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_partials(const bwd_chunk *__restrict__ chunks, uint32_t n_chunks,
                                                              const uint32_t *__restrict__ ref_p, const float *__restrict__ w,
                                                              const uint8_t *__restrict__ g, int d, float *__restrict__ partial) {
  constexpr int E = bwd_piece<DT>::E;
  const int lane = threadIdx.x & 63;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BWD_THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t wave_stride = gridDim.x * (BWD_THREADS / 64);
  const int pieces = d / E;
  const size_t row_bytes = (size_t)d * (DT == SCONE_DT_F32 ? 4 : 2);
  for (uint32_t ci = wave0; ci < n_chunks; ci += wave_stride) {
    const bwd_chunk c = chunks[ci];
    if (!__builtin_amdgcn_readfirstlane(c.partial)) continue;  // a whole row: the fused kernel's
    const uint32_t begin = __builtin_amdgcn_readfirstlane(c.begin), count = __builtin_amdgcn_readfirstlane(c.count);
    float *dst = partial + (size_t)__builtin_amdgcn_readfirstlane(c.dest) * d;
    const uint32_t *rp = ref_p + begin;
    for (int tile0 = 0; tile0 < pieces; tile0 += NT * 64) {
      float acc[NT][E];
      bool on[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        on[t] = tile0 + t * 64 + lane < pieces;
#pragma unroll
        for (int e = 0; e < E; ++e) acc[t][e] = 0.0f;
      }
      bwd_walk_chunk<DT, NT, MEAN>(rp, count, w, g + (size_t)(tile0 + lane) * 16, row_bytes, on, acc);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (on[t]) {
          float4 *o = reinterpret_cast<float4 *>(dst + (size_t)(tile0 + t * 64 + lane) * E);
#pragma unroll
          for (int q = 0; q < E / 4; ++q) o[q] = make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
        }
      }
    }
  }
}

// The references of a whole row (one chunk, and a touched row has 6.6 references on the headline batch) for one column tile:
// bwd_walk's order, so the same bits as bwd_walk_chunk, but in steps of 4 (8 on a one-piece tile), 2 and 1.  Half the loads in
// flight of the chunk pass cost this kernel 32 registers less -- a fourth wave per SIMD -- and the step of 2 saves a row of 6 or
// 7 references one dependent round trip.
template <int DT, int NT, bool MEAN>
__device__ __forceinline__ void apply_walk(const uint32_t *__restrict__ rp, uint32_t count, const float *__restrict__ w,
                                           const uint8_t *gl, size_t row_bytes, const bool (&on)[NT],
                                           float (&acc)[NT][bwd_piece<DT>::E]) {
  constexpr int R = NT == 1 ? 8 : 4;
  uint32_t i = 0;
  if constexpr (R > 4)
    for (; i + R <= count; i += R) bwd_walk<DT, NT, MEAN, R>(rp + i, w, gl, row_bytes, on, acc);
  for (; i + 4 <= count; i += 4) bwd_walk<DT, NT, MEAN, 4>(rp + i, w, gl, row_bytes, on, acc);
  if (i + 2 <= count) {
    bwd_walk<DT, NT, MEAN, 2>(rp + i, w, gl, row_bytes, on, acc);
    i += 2;
  }
  if (i < count) bwd_walk<DT, NT, MEAN, 1>(rp + i, w, gl, row_bytes, on, acc);
}

// a stored piece widened to fp32: fp32 is the value, bf16 is bits << 16
__device__ __forceinline__ float4 widen(const float4 &x) { return x; }
__device__ __forceinline__ float4 widen(const uint2 &b) {
  return make_float4(__uint_as_float(b.x << 16), __uint_as_float(b.x & 0xFFFF0000u), __uint_as_float(b.y << 16),
                     __uint_as_float(b.y & 0xFFFF0000u));
}

struct apply_args {
  const bwd_chunk *chunks;
  const bwd_multi *multi;
  const uint32_t *ref_p;
  const float *w;
  const uint8_t *g;
  const float *partial;
  const uint32_t *row_id;
  float *row_state;
  uint32_t n_chunks, n_multi;
  unsigned long long row_begin;
  int d;
  scone_opt_scalars sc;
  lean_rand rnd;
  scone_row_store st;
};

template <int DT, int NT, bool MEAN, int FMT, int KIND, bool STOCH>
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_apply(const apply_args a) {
  static_assert(FMT == SCONE_FMT_F32 || FMT == SCONE_FMT_BF16, "only fp32 and bf16 rows are weights in place");
  static_assert(!STOCH || FMT == SCONE_FMT_BF16, "only a bf16 row is rounded");
  constexpr int E = bwd_piece<DT>::E;
  constexpr bool ROWWISE = KIND == SCONE_LEAN_ROWWISE_ADAGRAD;
  using wraw_t = typename std::conditional<FMT == SCONE_FMT_BF16, uint2, float4>::type;  // a 4-element piece of a row as stored
  extern __shared__ float4 bwd_apply_lds[];
  const int d = a.d;
  const int lane = threadIdx.x & 63;
  float4 *L = bwd_apply_lds + (size_t)(threadIdx.x >> 6) * (d >> 2);  // this wave's gradient row: d / 4 pieces of four floats
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BWD_THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t wave_stride = gridDim.x * (BWD_THREADS / 64);
  const unsigned long long items = (unsigned long long)a.n_chunks + a.n_multi;
  const int pieces = d >> 2;        // the update's 16-byte pieces of fp32
  const int gpieces = d / E;        // the walk's 16-byte pieces of grad_out
  const bool one_block = pieces <= OPT_NT * 64;
  const size_t row_bytes = (size_t)d * (DT == SCONE_DT_F32 ? 4 : 2);
  const scone_opt_scalars sc = a.sc;
  // Work item i: the rows with several chunks come first (they are the long items: at the end they would be the tail), then the
  // chunk list.  Both records are 16 bytes: a bwd_multi is (seg, slot0, n, -), a bwd_chunk (begin, count, dest, partial).  A
  // touched row has few references, so a row is a chain of dependent memory round trips; the record of the wave's NEXT item is
  // requested a whole row ahead, and that row's id before this row's update, which takes two trips out of the chain.
  auto item_at = [&](unsigned long long i) {
    return i >= a.n_multi ? *reinterpret_cast<const uint4 *>(a.chunks + (i - a.n_multi)) : *reinterpret_cast<const uint4 *>(a.multi + i);
  };
  auto skipped = [&](unsigned long long i, const uint4 &r) {  // a chunk of a longer row: k_bwd_partials' and the multi entry's
    return i >= a.n_multi && __builtin_amdgcn_readfirstlane(r.w) != 0;
  };
  auto row_id_of = [&](unsigned long long i, const uint4 &r) {
    return a.row_id[__builtin_amdgcn_readfirstlane(i >= a.n_multi ? r.z : r.x)];
  };
  uint4 cur = make_uint4(0u, 0u, 0u, 0u);
  uint32_t idv = 0;
  if (wave0 < items) {
    cur = item_at(wave0);
    if (!skipped(wave0, cur)) idv = row_id_of(wave0, cur);
  }
  for (unsigned long long it = wave0; it < items; it += wave_stride) {
    const unsigned long long nit = it + wave_stride;
    const bool more = nit < items;
    uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
    if (more) nxt = item_at(nit);
    if (skipped(it, cur)) {
      cur = nxt;
      idv = more && !skipped(nit, nxt) ? row_id_of(nit, nxt) : 0u;
      continue;
    }
    const bool whole = it >= a.n_multi;
    // ---- the row's weights and state are requested now, so that they travel while the gradient is summed: a row of up to one
    // block (d <= 1024) is held as it is stored, a wider row is loaded block by block by the update
    const unsigned long long id = __builtin_amdgcn_readfirstlane(idv);
    const unsigned long long lr = id - a.row_begin;
    float4 *W = reinterpret_cast<float4 *>(a.st.row(lr));
    uint2 *W16 = reinterpret_cast<uint2 *>(a.st.row(lr));  // a bf16 row: piece p is 8 bytes
    wraw_t wq[OPT_NT];
    if (one_block) {
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t)
        if (t * 64 + lane < pieces) wq[t] = reinterpret_cast<const wraw_t *>(W)[t * 64 + lane];
    }
    float s_old = 0.f;
    if (ROWWISE && lane == 0) s_old = a.row_state[lr];

    // ---- the row's gradient, into LDS
    if (whole) {
      const uint32_t begin = __builtin_amdgcn_readfirstlane(cur.x), count = __builtin_amdgcn_readfirstlane(cur.y);
      const uint32_t *rp = a.ref_p + begin;
      for (int tile0 = 0; tile0 < gpieces; tile0 += NT * 64) {
        float acc[NT][E];
        bool on[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          on[t] = tile0 + t * 64 + lane < gpieces;
#pragma unroll
          for (int e = 0; e < E; ++e) acc[t][e] = 0.0f;
        }
        apply_walk<DT, NT, MEAN>(rp, count, a.w, a.g + (size_t)(tile0 + lane) * 16, row_bytes, on, acc);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (on[t]) {
            float4 *o = L + (size_t)(tile0 + t * 64 + lane) * (E / 4);
#pragma unroll
            for (int q = 0; q < E / 4; ++q) o[q] = make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
          }
        }
      }
    } else {
      const uint32_t n = __builtin_amdgcn_readfirstlane(cur.z);
      const float *src0 = a.partial + (size_t)__builtin_amdgcn_readfirstlane(cur.y) * d;
      for (int p = lane; p < pieces; p += 64) {  // k_bwd_combine's sum: from +0.0f, the partials in chunk order
        const float *src = src0 + (size_t)p * 4;
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t j = 0;
        for (; j + 4 <= n; j += 4) {
          float4 v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const float4 *>(src + (size_t)(j + r) * d);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            s[0] = s[0] + v[r].x, s[1] = s[1] + v[r].y, s[2] = s[2] + v[r].z, s[3] = s[3] + v[r].w;
          }
        }
        for (; j < n; ++j) {
          const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)j * d);
          s[0] = s[0] + v.x, s[1] = s[1] + v.y, s[2] = s[2] + v.z, s[3] = s[3] + v.w;
        }
        L[p] = make_float4(s[0], s[1], s[2], s[3]);
      }
    }
    uint32_t next_idv = 0;
    if (more && !skipped(nit, nxt)) next_idv = row_id_of(nit, nxt);
    wave_lds_fence();  // this wave's writes, before its reads in the other lane map

    // ---- k_opt_lean's in-place body, G in LDS
    const float4 *G = L;
    const uint32_t row_key = STOCH ? scone_lean_row_key(a.rnd.seed, a.rnd.step, (uint64_t)id) : 0u;

    float4 g[OPT_NT], w[OPT_NT];
    bool on[OPT_NT];
    auto load_block = [&](int p0) {
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        on[t] = p < pieces;
        g[t] = w[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on[t]) {
          g[t] = G[p];
          w[t] = widen(one_block ? wq[t] : reinterpret_cast<const wraw_t *>(W)[p]);
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
      for (int s = 32; s >= 1; s >>= 1) q = q + __shfl_xor(q, s, 64);  // the contract's butterfly
      float s_new = 0.f;
      if (lane == 0) {
        const float g2 = q / (float)d;
        s_new = s_old + g2;
        a.row_state[lr] = s_new;
      }
      s_new = __shfl(s_new, 0, 64);
      den = sqrtf(s_new) + sc.eps;
    }

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
        if (STOCH) {
          const uint32_t j = (uint32_t)p << 2;
          if (on[t])
            W16[p] = make_uint2(lean_bf16_stochastic(w[t].x, row_key, j) | (lean_bf16_stochastic(w[t].y, row_key, j + 1) << 16),
                                lean_bf16_stochastic(w[t].z, row_key, j + 2) | (lean_bf16_stochastic(w[t].w, row_key, j + 3) << 16));
        } else if (p0 + t * 64 < pieces) {
          opt_store_piece<FMT>(a.st, nullptr, lr, d, p, on[t], w[t], lane);
        }
      }
    }
    wave_lds_fence();  // this row's reads, before the next row's writes
    cur = nxt;
    idv = next_idv;
  }
}

// ---------------------------------------------------------------- host side
template <int DT, int NT, bool MEAN>
void launch_variant(int fmt, int kind, bool stoch, const apply_args &a, unsigned blocks, size_t lds, hipStream_t s) {
#define SCONE_APPLY(FMT, KIND, STOCH) \
  hipLaunchKernelGGL((k_bwd_apply<DT, NT, MEAN, FMT, KIND, STOCH>), dim3(blocks), dim3(BWD_THREADS), lds, s, a)
  const bool sgd = kind == SCONE_LEAN_SGD;
  if (fmt == SCONE_FMT_F32) {
    if (sgd)
      SCONE_APPLY(SCONE_FMT_F32, SCONE_LEAN_SGD, false);
    else
      SCONE_APPLY(SCONE_FMT_F32, SCONE_LEAN_ROWWISE_ADAGRAD, false);
  } else if (stoch) {
    if (sgd)
      SCONE_APPLY(SCONE_FMT_BF16, SCONE_LEAN_SGD, true);
    else
      SCONE_APPLY(SCONE_FMT_BF16, SCONE_LEAN_ROWWISE_ADAGRAD, true);
  } else {
    if (sgd)
      SCONE_APPLY(SCONE_FMT_BF16, SCONE_LEAN_SGD, false);
    else
      SCONE_APPLY(SCONE_FMT_BF16, SCONE_LEAN_ROWWISE_ADAGRAD, false);
  }
#undef SCONE_APPLY
}

template <int DT, int NT, bool MEAN>
void launch_nt(const scone_bwd_plan *pl, int fmt, int kind, bool stoch, const apply_args &a, unsigned blocks, hipStream_t s) {
  if (pl->m.n_multi)
    hipLaunchKernelGGL((k_bwd_partials<DT, NT, MEAN>), dim3(scone_capped_blocks(((unsigned long long)pl->m.n_chunks + 3) / 4)),
                       dim3(BWD_THREADS), 0, s, pl->d_chunks, pl->m.n_chunks, pl->d_ref_p, pl->d_w, a.g, a.d, pl->d_partial);
  launch_variant<DT, NT, MEAN>(fmt, kind, stoch, a, blocks, (size_t)(BWD_THREADS / 64) * a.d * sizeof(float), s);
}

// the column tile of the walk: k_bwd_chunks' choice
template <int DT, bool MEAN>
void launch_dt(const scone_bwd_plan *pl, int fmt, int kind, bool stoch, const apply_args &a, unsigned blocks, hipStream_t s) {
  const int pieces = a.d / bwd_piece<DT>::E;
  if (pieces <= 64)
    launch_nt<DT, 1, MEAN>(pl, fmt, kind, stoch, a, blocks, s);
  else if (pieces <= 128)
    launch_nt<DT, 2, MEAN>(pl, fmt, kind, stoch, a, blocks, s);
  else
    launch_nt<DT, 4, MEAN>(pl, fmt, kind, stoch, a, blocks, s);
}

template <int DT>
void launch_reduce(const scone_bwd_plan *pl, int reduce, int fmt, int kind, bool stoch, const apply_args &a, unsigned blocks,
                   hipStream_t s) {
  if (reduce == SCONE_REDUCE_MEAN)
    launch_dt<DT, true>(pl, fmt, kind, stoch, a, blocks, s);
  else
    launch_dt<DT, false>(pl, fmt, kind, stoch, a, blocks, s);
}

}  // namespace

extern "C" int scone_backward_apply_lean(scone_handle *h, scone_bwd_plan *plan, const void *d_grad_out, int32_t grad_dtype,
                                         int32_t reduce, const scone_lean_cfg *cfg, float *d_row_state, scone_stream_t stream) {
  const char *who = "scone_backward_apply_lean";
  SCONE_TRY(opt_need_table(h, who, lean_check(cfg)));
  if (!plan) return scone_refuse(h, SCONE_EINVAL, who, "null plan");
  if (plan->h != h) return scone_refuse(h, SCONE_EINVAL, who, "the plan belongs to another handle");
  if (plan->index) return scone_refuse(h, SCONE_EINVAL, who, "an index plan's ids are not table rows (scone_backward_plan_index)");
  if (grad_dtype != SCONE_DT_F32 && grad_dtype != SCONE_DT_F16 && grad_dtype != SCONE_DT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who, "bad grad_dtype");
  if (reduce != SCONE_REDUCE_MEAN && reduce != SCONE_REDUCE_SUM) return scone_refuse(h, SCONE_EINVAL, who, "bad reduce");
  const int fmt = h->cfg.table_fmt;
  const bool stoch = cfg->rounding == SCONE_ROUND_STOCHASTIC;
  SCONE_TRY(lean_inplace_check(h, who, stoch, false, false));
  if (h->cfg.dim > SCONE_BWD_APPLY_MAX_DIM)
    return scone_refuse(h, SCONE_EINVAL, who,
                        "d > 4096 is not fused (a wave's gradient row must fit its share of LDS): call scone_backward_rows, then "
                        "scone_opt_step_lean");
  if (plan->m.n_segs == 0) return SCONE_OK;
  if (!d_grad_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  if (cfg->kind == SCONE_LEAN_ROWWISE_ADAGRAD && !d_row_state)
    return scone_refuse(h, SCONE_EINVAL, who, "row-wise Adagrad needs d_row_state (one fp32 per owned row)");
  SCONE_ON_DEVICE(h);
  apply_args a;
  a.chunks = plan->d_chunks, a.multi = plan->d_multi, a.ref_p = plan->d_ref_p, a.w = plan->d_w;
  a.g = reinterpret_cast<const uint8_t *>(d_grad_out), a.partial = plan->d_partial, a.row_id = plan->d_row_id;
  a.row_state = d_row_state, a.n_chunks = plan->m.n_chunks, a.n_multi = plan->m.n_multi;
  a.row_begin = h->cfg.row_begin, a.d = plan->dim;
  a.rnd.seed = cfg->seed, a.rnd.step = cfg->step;
  lean_scalars(cfg, &a.sc);
  const unsigned blocks = opt_begin(h, (unsigned long long)plan->m.n_chunks + plan->m.n_multi);  // drops a staged cache first
  a.st = scone_store_of(h);
  hipStream_t s = (hipStream_t)stream;
  if (grad_dtype == SCONE_DT_F32)
    launch_reduce<SCONE_DT_F32>(plan, reduce, fmt, cfg->kind, stoch, a, blocks, s);
  else if (grad_dtype == SCONE_DT_F16)
    launch_reduce<SCONE_DT_F16>(plan, reduce, fmt, cfg->kind, stoch, a, blocks, s);
  else
    launch_reduce<SCONE_DT_BF16>(plan, reduce, fmt, cfg->kind, stoch, a, blocks, s);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}
