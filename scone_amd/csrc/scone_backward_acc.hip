// The backward that accumulates (include/scone_hip.h, "gradient accumulation"): scone_backward_rows followed by
// scone_grad_merge_rows(old, new) in one pass over the plan, so that the new gradient -- fp32 [U, d] -- is never stored.  The
// caller has merged the id lists already (scone_grad_merge_map, a = the old gradient's ids, b = scone_backward_row_ids): src_old
// and src_new are that call's src_a and src_b, pos_new its pos_b.
//
// k_bwd_chunks_acc is k_bwd_chunks with another last step: the chunk that is a whole row u has its sum finished in registers
// (the walk is scone_bwd_plan.h's, shared with k_bwd_chunks: the order of the adds is stated there and nowhere else), then
// out[pos_new[u]] = old[src_old[..]] + acc -- one add, old the first operand, as scone_grad_merge_rows adds -- or acc itself
// where the old gradient does not have the row.  The chunks of a longer row go to the plan's partial slots unchanged;
// k_bwd_combine_acc adds them in chunk order, as k_bwd_combine does, and old last.  k_bwd_copy_old copies the rows only the old
// gradient has, a wave per output row.  Three launches at most, plain vector stores, no atomics.
#include "scone_bwd_plan.h"
#include "scone_opt_rows.h"  // OPT_NT and the grid of a row-parallel kernel

namespace {

constexpr int BWD_THREADS = 256;  // four waves, as k_bwd_chunks
constexpr uint32_t ACC_ABSENT = 0xFFFFFFFFu;

struct acc_args {
  const uint32_t *src_old;  // [n_out] row of the old gradient, or absent
  const uint32_t *src_new;  // [n_out] row of the plan, or absent
  const uint32_t *pos_new;  // [U] output row of plan row u
  const float *old_rows;
  float *out;
  unsigned long long n_out;
};

template <int DT, int NT, bool MEAN>
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_chunks_acc(const bwd_chunk *__restrict__ chunks, uint32_t n_chunks,
                                                                const uint32_t *__restrict__ ref_p, const float *__restrict__ w,
                                                                const uint8_t *__restrict__ g, int d, float *__restrict__ partial,
                                                                const acc_args a) {
  constexpr int E = bwd_piece<DT>::E;
  const int lane = threadIdx.x & 63;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BWD_THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t wave_stride = gridDim.x * (BWD_THREADS / 64);
  const int pieces = d / E;
  const size_t row_bytes = (size_t)d * (DT == SCONE_DT_F32 ? 4 : 2);
  for (uint32_t ci = wave0; ci < n_chunks; ci += wave_stride) {
    const bwd_chunk c = chunks[ci];
    const uint32_t begin = __builtin_amdgcn_readfirstlane(c.begin), count = __builtin_amdgcn_readfirstlane(c.count);
    const bool is_partial = __builtin_amdgcn_readfirstlane(c.partial) != 0;
    const uint32_t dest = __builtin_amdgcn_readfirstlane(c.dest);
    float *dst;
    const float *old = nullptr;
    if (is_partial) {
      dst = partial + (size_t)dest * d;
    } else {
      const uint32_t o = __builtin_amdgcn_readfirstlane(a.pos_new[dest]);
      if (o >= a.n_out) continue;  // never with the map of scone_grad_merge_map: no store leaves `out`
      const uint32_t so = __builtin_amdgcn_readfirstlane(a.src_old[o]);
      dst = a.out + (size_t)o * d;
      if (so != ACC_ABSENT) old = a.old_rows + (size_t)so * d;
    }
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
      if (old) {  // wave-uniform: the finished sum, then one add
        float4 ov[NT][E / 4];
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (on[t]) {
            const float4 *op = reinterpret_cast<const float4 *>(old + (size_t)(tile0 + t * 64 + lane) * E);
#pragma unroll
            for (int q = 0; q < E / 4; ++q) ov[t][q] = op[q];
          }
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (on[t]) {
#pragma unroll
            for (int q = 0; q < E / 4; ++q) {
              acc[t][4 * q] = ov[t][q].x + acc[t][4 * q];
              acc[t][4 * q + 1] = ov[t][q].y + acc[t][4 * q + 1];
              acc[t][4 * q + 2] = ov[t][q].z + acc[t][4 * q + 2];
              acc[t][4 * q + 3] = ov[t][q].w + acc[t][4 * q + 3];
            }
          }
      }
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

// A wave owns (row with several chunks, tile of 256 columns): the row's partials in chunk order from +0.0f, k_bwd_combine's sum,
// then old + that sum.
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_combine_acc(const bwd_multi *__restrict__ multi, uint32_t n_multi,
                                                                 const float *__restrict__ partial, int d, const acc_args a) {
  const int lane = threadIdx.x & 63;
  const uint32_t col_tiles = (uint32_t)((d + 255) / 256);
  const unsigned long long items = (unsigned long long)n_multi * col_tiles;
  const unsigned long long wave0 = blockIdx.x * (unsigned long long)(BWD_THREADS / 64) + (threadIdx.x >> 6);
  const unsigned long long stride = gridDim.x * (unsigned long long)(BWD_THREADS / 64);
  for (unsigned long long it = wave0; it < items; it += stride) {
    const bwd_multi mr = multi[it / col_tiles];
    const int col = (int)(it % col_tiles) * 256 + lane * 4;
    const uint32_t o = __builtin_amdgcn_readfirstlane(a.pos_new[mr.seg]);
    if (o >= a.n_out) continue;  // never with the map of scone_grad_merge_map
    if (col >= d) continue;      // d % 4 == 0: a lane's four columns are inside or outside together
    const uint32_t so = __builtin_amdgcn_readfirstlane(a.src_old[o]);
    float4 ov = make_float4(0.f, 0.f, 0.f, 0.f);
    if (so != ACC_ABSENT) ov = *reinterpret_cast<const float4 *>(a.old_rows + (size_t)so * d + col);  // in flight under the sum
    const float *src = partial + (size_t)mr.slot0 * d + col;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t j = 0;
    for (; j + 4 <= mr.n; j += 4) {
      float4 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const float4 *>(src + (size_t)(j + r) * d);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[0] = s[0] + v[r].x, s[1] = s[1] + v[r].y, s[2] = s[2] + v[r].z, s[3] = s[3] + v[r].w;
      }
    }
    for (; j < mr.n; ++j) {
      const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)j * d);
      s[0] = s[0] + v.x, s[1] = s[1] + v.y, s[2] = s[2] + v.z, s[3] = s[3] + v.w;
    }
    if (so != ACC_ABSENT) s[0] = ov.x + s[0], s[1] = ov.y + s[1], s[2] = ov.z + s[2], s[3] = ov.w + s[3];
    *reinterpret_cast<float4 *>(a.out + (size_t)o * d + col) = make_float4(s[0], s[1], s[2], s[3]);
  }
}

// the rows only the old gradient has: a wave per output row, every bit copied (k_grad_merge_rows' walk)
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_copy_old(int d, const acc_args a) {
  const int lane = threadIdx.x & 63;
  const int pieces = d >> 2;
  const unsigned long long nwaves = (unsigned long long)gridDim.x * (BWD_THREADS / 64);
  for (unsigned long long r = (unsigned long long)blockIdx.x * (BWD_THREADS / 64) + (threadIdx.x >> 6); r < a.n_out; r += nwaves) {
    if (__builtin_amdgcn_readfirstlane(a.src_new[r]) != ACC_ABSENT) continue;  // the other two kernels' row
    const uint32_t so = __builtin_amdgcn_readfirstlane(a.src_old[r]);
    const float4 *A = reinterpret_cast<const float4 *>(a.old_rows + (so != ACC_ABSENT ? so : 0u) * (unsigned long long)d);
    float4 *O = reinterpret_cast<float4 *>(a.out + r * (unsigned long long)d);
    for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
      float4 x[OPT_NT];
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        x[t] = make_float4(0.f, 0.f, 0.f, 0.f);  // a row nobody has (never with scone_grad_merge_map's map) is stored as zeros
        if (p < pieces && so != ACC_ABSENT) x[t] = A[p];
      }
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        if (p < pieces) O[p] = x[t];
      }
    }
  }
}

unsigned acc_blocks(const scone_handle *h, unsigned long long waves) {
  const unsigned blocks = scone_capped_blocks((waves + 3) / 4);
  return h->opt_max_blocks > 0 && blocks > (unsigned long long)h->opt_max_blocks ? (unsigned)h->opt_max_blocks : blocks;
}

template <int DT, bool MEAN>
void launch_chunks_acc(const scone_handle *h, const scone_bwd_plan *pl, const void *g, const acc_args &a, hipStream_t s) {
  const int d = pl->dim;
  const int pieces = d / bwd_piece<DT>::E;  // the column tile: k_bwd_chunks' choice
  const unsigned blocks = acc_blocks(h, pl->m.n_chunks);
  const uint8_t *gb = reinterpret_cast<const uint8_t *>(g);
#define SCONE_BWD_ACC_LAUNCH(NT)                                                                                                  \
  hipLaunchKernelGGL((k_bwd_chunks_acc<DT, NT, MEAN>), dim3(blocks), dim3(BWD_THREADS), 0, s, pl->d_chunks, pl->m.n_chunks, pl->d_ref_p, \
                     pl->d_w, gb, d, pl->d_partial, a)
  if (pieces <= 64)
    SCONE_BWD_ACC_LAUNCH(1);
  else if (pieces <= 128)
    SCONE_BWD_ACC_LAUNCH(2);
  else
    SCONE_BWD_ACC_LAUNCH(4);
#undef SCONE_BWD_ACC_LAUNCH
}

template <int DT>
void launch_acc(const scone_handle *h, const scone_bwd_plan *pl, const void *g, int reduce, const acc_args &a, hipStream_t s) {
  if (reduce == SCONE_REDUCE_MEAN)
    launch_chunks_acc<DT, true>(h, pl, g, a, s);
  else
    launch_chunks_acc<DT, false>(h, pl, g, a, s);
}

}  // namespace

extern "C" int scone_backward_rows_acc(scone_handle *h, scone_bwd_plan *plan, const void *d_grad_out, int32_t grad_dtype,
                                       int32_t reduce, const uint32_t *d_src_old, const uint32_t *d_src_new,
                                       const uint32_t *d_pos_new, uint64_t n_out, const float *d_rows_old, float *d_rows_out,
                                       scone_stream_t stream) {
  const char *who = "scone_backward_rows_acc";
  if (!h) return SCONE_EINVAL;
  if (!plan) return scone_refuse(h, SCONE_EINVAL, who, "null plan");
  if (plan->h != h) return scone_refuse(h, SCONE_EINVAL, who, "the plan belongs to another handle");
  if (h->cfg.dim == 0 || h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0");
  if (grad_dtype != SCONE_DT_F32 && grad_dtype != SCONE_DT_F16 && grad_dtype != SCONE_DT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who, "bad grad_dtype");
  if (reduce != SCONE_REDUCE_MEAN && reduce != SCONE_REDUCE_SUM) return scone_refuse(h, SCONE_EINVAL, who, "bad reduce");
  const uint32_t U = plan->m.n_segs;
  if (n_out >= 0xFFFFFFFFull) return scone_refuse(h, SCONE_EINVAL, who, "n_out must be below 2^32 - 1");
  if (n_out < U) return scone_refuse(h, SCONE_ERANGE, who, "n_out below the plan's n_rows: not the map of this plan");
  if (d_rows_out && d_rows_out == d_rows_old)
    return scone_refuse(h, SCONE_EINVAL, who, "the output must not overlap the old rows (d_rows_out equals d_rows_old)");
  if (n_out == 0) return SCONE_OK;
  if (!d_src_old || !d_src_new || !d_rows_out || (U && (!d_grad_out || !d_pos_new)))
    return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  acc_args a;
  a.src_old = d_src_old, a.src_new = d_src_new, a.pos_new = d_pos_new, a.old_rows = d_rows_old, a.out = d_rows_out, a.n_out = n_out;
  if (n_out > U)  // there are rows only the old gradient has
    hipLaunchKernelGGL(k_bwd_copy_old, dim3(acc_blocks(h, n_out)), dim3(BWD_THREADS), 0, s, plan->dim, a);
  if (U) {
    if (grad_dtype == SCONE_DT_F32)
      launch_acc<SCONE_DT_F32>(h, plan, d_grad_out, reduce, a, s);
    else if (grad_dtype == SCONE_DT_F16)
      launch_acc<SCONE_DT_F16>(h, plan, d_grad_out, reduce, a, s);
    else
      launch_acc<SCONE_DT_BF16>(h, plan, d_grad_out, reduce, a, s);
    if (plan->m.n_multi) {
      const unsigned long long items = (unsigned long long)plan->m.n_multi * ((plan->dim + 255) / 256);
      hipLaunchKernelGGL(k_bwd_combine_acc, dim3(acc_blocks(h, items)), dim3(BWD_THREADS), 0, s, plan->d_multi, plan->m.n_multi,
                         plan->d_partial, plan->dim, a);
    }
  }
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}
