// Backward of the dense side of the fused lookup: the gradients of wte and wpe (include/scone_hip.h, "backward of the dense
// side").
//
// out = (wte[tok] + reduce_k row_k) + wpe[pos]: the gradient of row i of wte (wpe) is the sum of grad_out[p, :] over the
// positions p with tok[p] == i (pos[p] == i).  That is the table's backward with one-element lists and the weight 1.0f, in a
// second id space, so an INDEX PLAN is a scone_bwd_plan built by the same sort / segment / chunk passes (scone_backward.hip) from
// the pairs (idx[p], p); everything that takes a plan -- scone_backward_rows, _row_ids, _counts, _rows_acc -- takes it as it is.
//
// The rectangle with default positions needs no plan at all: row t of grad_wpe has the references b * T + t, b ascending.
// scone_backward_wpe computes them (k_wpe_chunks: a wave owns (row t, chunk j of C batch rows)) and adds a row's partials in
// chunk order (k_wpe_combine) -- the order, the +0.0 starts and the separate roundings of the contract, hence its bits.
#include "scone_bwd_plan.h"
#include "scone_common.h"

namespace {

constexpr int IDX_THREADS = 256;

unsigned blocks_for(unsigned long long n) { return scone_capped_blocks((n + IDX_THREADS - 1) / IDX_THREADS); }

__device__ __forceinline__ bool idx_kept(const int32_t *__restrict__ idx, const int32_t *__restrict__ skip, long long p, long long n_ids) {
  const long long id = idx[p];
  return id >= 0 && id < n_ids && !(skip && skip[p] != 0);
}

// K_p (0 or 1), the weight 1.0f, and the scan's last element
__global__ void k_idx_count(const int32_t *__restrict__ idx, const int32_t *__restrict__ skip, long long ntok, long long n_ids,
                            uint32_t *__restrict__ kown, int32_t *__restrict__ kfull, float *__restrict__ w) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p <= ntok; p += (long long)gridDim.x * blockDim.x) {
    if (p == ntok) {
      kown[p] = 0;
      continue;
    }
    const uint32_t k = idx_kept(idx, skip, p, n_ids) ? 1u : 0u;
    kown[p] = k;
    kfull[p] = (int32_t)k;
    w[p] = 1.0f;
  }
}

__global__ void k_idx_expand(const int32_t *__restrict__ idx, const int32_t *__restrict__ skip, long long ntok, long long n_ids,
                             const uint32_t *__restrict__ ref_off, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < ntok; p += (long long)gridDim.x * blockDim.x) {
    if (!idx_kept(idx, skip, p, n_ids)) continue;
    const uint32_t at = ref_off[p];  // < the kept count <= ntok = max_refs
    keys[at] = (uint32_t)idx[p];
    vals[at] = (uint32_t)p;
  }
}

// the lookup's default position of every p: p % T, or the packed matcher's p - cu[s] with its clamps (k_match_ell_varlen)
__global__ void k_default_pos(const int32_t *__restrict__ cu, int n_seqs, int T, long long total, int32_t *__restrict__ out) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
    if (!cu) {
      out[p] = (int32_t)(p % T);
      continue;
    }
    int lo = 1, hi = n_seqs;  // smallest j in [1, n_seqs] with cu[j] > p (n_seqs if the array breaks its contract)
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cu[mid] > (int)p) hi = mid; else lo = mid + 1;
    }
    long long i = p - (long long)cu[lo - 1];
    i = i < 0 ? 0 : (i > p ? p : i);
    out[p] = (int32_t)i;
  }
}

// ---------------------------------------------------------------- grad_wpe of a rectangle with default positions
// RR references b0 .. b0 + RR - 1 of row t: bwd_walk (scone_bwd_plan.h) with the positions computed, p = b * T + t
template <int DT, int NT, int RR>
__device__ __forceinline__ void wpe_walk(const uint8_t *gl, size_t step_bytes, const bool (&on)[NT], float (&acc)[NT][bwd_piece<DT>::E]) {
  constexpr int E = bwd_piece<DT>::E;
  uint4 raw[RR][NT];
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    const uint8_t *row = gl + (size_t)r * step_bytes;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (on[t]) raw[r][t] = *reinterpret_cast<const uint4 *>(row + (size_t)t * 1024);
  }
#pragma unroll
  for (int r = 0; r < RR; ++r) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (on[t]) {
        float f[E];
        bwd_piece<DT>::to_f32(raw[r][t], f);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[t][e] = acc[t][e] + f[e];
      }
    }
  }
}

// A wave owns (row t, chunk j): the batch rows [j C, min(B, (j + 1) C)).  Lanes own 16-byte column pieces as in k_bwd_chunks;
// 16 / NT references at a time (16 independent 16-byte loads per lane in flight), what is left four at a time, then one by one;
// `a = a + c` in b order is the only dependent chain.  B <= C: the partial is the row; else it goes to slot t * n_chunks + j.
template <int DT, int NT>
__global__ __launch_bounds__(IDX_THREADS) void k_wpe_chunks(const uint8_t *__restrict__ g, int B, int T, int rows, int d, int n_chunks,
                                                            float *__restrict__ out, float *__restrict__ partial) {
  constexpr int E = bwd_piece<DT>::E;
  constexpr int R = 16 / NT;
  const int lane = threadIdx.x & 63;
  const unsigned long long wave0 =
      __builtin_amdgcn_readfirstlane((unsigned)(blockIdx.x * (IDX_THREADS / 64) + (threadIdx.x >> 6)));
  const unsigned long long stride = (unsigned long long)gridDim.x * (IDX_THREADS / 64);
  const unsigned long long items = (unsigned long long)rows * n_chunks;
  const int pieces = d / E;
  const size_t row_bytes = (size_t)d * (DT == SCONE_DT_F32 ? 4 : 2);
  const size_t step_bytes = row_bytes * (size_t)T;  // from (b, t) to (b + 1, t)
  for (unsigned long long it = wave0; it < items; it += stride) {
    const int t = (int)(it / n_chunks), j = (int)(it % n_chunks);
    const int b0 = j * SCONE_BWD_CHUNK;
    const int count = B - b0 < SCONE_BWD_CHUNK ? B - b0 : SCONE_BWD_CHUNK;
    float *dst = n_chunks > 1 ? partial + (size_t)it * d : out + (size_t)t * d;
    for (int tile0 = 0; tile0 < pieces; tile0 += NT * 64) {
      float acc[NT][E];
      bool on[NT];
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        on[q] = tile0 + q * 64 + lane < pieces;
#pragma unroll
        for (int e = 0; e < E; ++e) acc[q][e] = 0.0f;
      }
      const uint8_t *gl = g + ((size_t)b0 * T + t) * row_bytes + (size_t)(tile0 + lane) * 16;
      int i = 0;
      if constexpr (R > 4)
        for (; i + R <= count; i += R) wpe_walk<DT, NT, R>(gl + (size_t)i * step_bytes, step_bytes, on, acc);
      for (; i + 4 <= count; i += 4) wpe_walk<DT, NT, 4>(gl + (size_t)i * step_bytes, step_bytes, on, acc);
      for (; i < count; ++i) wpe_walk<DT, NT, 1>(gl + (size_t)i * step_bytes, step_bytes, on, acc);
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        if (on[q]) {
          float4 *o = reinterpret_cast<float4 *>(dst + (size_t)(tile0 + q * 64 + lane) * E);
#pragma unroll
          for (int v = 0; v < E / 4; ++v) o[v] = make_float4(acc[q][4 * v], acc[q][4 * v + 1], acc[q][4 * v + 2], acc[q][4 * v + 3]);
        }
      }
    }
  }
}

// B > C: a wave owns (row t, tile of 256 columns) and adds the row's n_chunks partials in chunk order, as k_bwd_combine does
__global__ __launch_bounds__(IDX_THREADS) void k_wpe_combine(const float *__restrict__ partial, int rows, int d, int n_chunks,
                                                             float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const unsigned col_tiles = (unsigned)((d + 255) / 256);
  const unsigned long long items = (unsigned long long)rows * col_tiles;
  const unsigned long long wave0 = blockIdx.x * (unsigned long long)(IDX_THREADS / 64) + (threadIdx.x >> 6);
  const unsigned long long stride = gridDim.x * (unsigned long long)(IDX_THREADS / 64);
  for (unsigned long long it = wave0; it < items; it += stride) {
    const int t = (int)(it / col_tiles);
    const int col = (int)(it % col_tiles) * 256 + lane * 4;
    if (col >= d) continue;  // d % 4 == 0: a lane's four columns are inside or outside together
    const float *src = partial + (size_t)t * n_chunks * d + col;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int j = 0;
    for (; j + 4 <= n_chunks; j += 4) {
      float4 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const float4 *>(src + (size_t)(j + r) * d);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[0] = a[0] + v[r].x, a[1] = a[1] + v[r].y, a[2] = a[2] + v[r].z, a[3] = a[3] + v[r].w;
      }
    }
    for (; j < n_chunks; ++j) {
      const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)j * d);
      a[0] = a[0] + v.x, a[1] = a[1] + v.y, a[2] = a[2] + v.z, a[3] = a[3] + v.w;
    }
    *reinterpret_cast<float4 *>(out + (size_t)t * d + col) = make_float4(a[0], a[1], a[2], a[3]);
  }
}

template <int DT>
void launch_wpe_chunks(const void *g, int B, int T, int rows, int d, int n_chunks, float *out, float *partial, hipStream_t s) {
  const int pieces = d / bwd_piece<DT>::E;
  const unsigned blocks = scone_capped_blocks(((unsigned long long)rows * n_chunks + 3) / 4);
  const uint8_t *gb = reinterpret_cast<const uint8_t *>(g);
#define SCONE_WPE_LAUNCH(NT) \
  hipLaunchKernelGGL((k_wpe_chunks<DT, NT>), dim3(blocks), dim3(IDX_THREADS), 0, s, gb, B, T, rows, d, n_chunks, out, partial)
  if (pieces <= 64)  // the tile rule of k_bwd_chunks
    SCONE_WPE_LAUNCH(1);
  else if (pieces <= 128)
    SCONE_WPE_LAUNCH(2);
  else
    SCONE_WPE_LAUNCH(4);
#undef SCONE_WPE_LAUNCH
}

int wpe_chunks_of(int B) { return (B + SCONE_BWD_CHUNK - 1) / SCONE_BWD_CHUNK; }

}  // namespace

// ---------------------------------------------------------------- the index source of a plan build (scone_bwd_plan.h)
int scone_bwd_index_pairs(scone_handle *h, const bwd_plan_src &src, long long ntok, const bwd_plan_bufs &b, hipStream_t s) {
  hipLaunchKernelGGL(k_idx_count, dim3(blocks_for(ntok + 1)), dim3(IDX_THREADS), 0, s, src.tok, src.skip, ntok, src.n_ids, b.kown,
                     b.kfull, b.w);
  SCONE_HIP(h, hipGetLastError());
  size_t n1 = b.scratch_bytes;
  SCONE_TRY(scone_bwd_scan_u32(h, b.scratch, n1, b.kown, b.ref_off, (size_t)(ntok + 1), s));
  hipLaunchKernelGGL(k_idx_expand, dim3(blocks_for(ntok)), dim3(IDX_THREADS), 0, s, src.tok, src.skip, ntok, src.n_ids, b.ref_off,
                     b.keys, b.vals);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_backward_plan_index(scone_handle *h, const int32_t *d_idx, int64_t ntok, int64_t n_ids, const int32_t *d_skip,
                                         scone_bwd_plan **out, uint64_t *h_n_rows, uint64_t *h_n_refs, scone_stream_t stream) {
  static const char who[] = "scone_backward_plan_index";
  if (!h) return SCONE_EINVAL;
  if (!out) return scone_refuse(h, SCONE_EINVAL, who, "null out");
  *out = nullptr;
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0");
  if (ntok < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative ntok");
  if (ntok >= (1ll << 32)) return scone_refuse(h, SCONE_EINVAL, who, "too many positions for one plan (references are numbered in 32 bits)");
  if (n_ids <= 0 || n_ids >= 0xFFFFFFFFll) return scone_refuse(h, SCONE_EINVAL, who, "n_ids must be in [1, 2^32 - 1)");
  if (ntok > 0 && !d_idx) return scone_refuse(h, SCONE_EINVAL, who, "null d_idx");
  SCONE_ON_DEVICE(h);
  bwd_plan_src src = {};
  src.kind = BWD_SRC_INDEX, src.tok = d_idx, src.skip = d_skip, src.n_ids = n_ids;
  return scone_bwd_plan_make(h, src, ntok, (unsigned long long)ntok, out, h_n_rows, h_n_refs, (hipStream_t)stream);
}

extern "C" int scone_backward_default_positions(scone_handle *h, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t T,
                                                int64_t total_tokens, int32_t *d_pos_out, scone_stream_t stream) {
  static const char who[] = "scone_backward_default_positions";
  if (!h) return SCONE_EINVAL;
  if (total_tokens < 0 || n_seqs < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative n_seqs or total_tokens");
  if (total_tokens > 0x7FFFFFFFll) return scone_refuse(h, SCONE_EINVAL, who, "total_tokens above 2^31 - 1");
  if (!d_cu_seqlens && total_tokens > 0 && (T <= 0 || total_tokens % T != 0))
    return scone_refuse(h, SCONE_EINVAL, who, "a rectangle needs T > 0 and total_tokens % T == 0");
  if (total_tokens == 0 || (d_cu_seqlens && n_seqs == 0)) return SCONE_OK;  // as scone_embed_varlen: no sequences, no positions
  if (!d_pos_out) return scone_refuse(h, SCONE_EINVAL, who, "null d_pos_out");
  SCONE_ON_DEVICE(h);
  hipLaunchKernelGGL(k_default_pos, dim3(blocks_for(total_tokens)), dim3(IDX_THREADS), 0, (hipStream_t)stream, d_cu_seqlens,
                     (int)n_seqs, (int)T, (long long)total_tokens, d_pos_out);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_backward_wpe_scratch(int32_t B, int32_t T, int32_t d, uint64_t *bytes) {
  if (!bytes || B < 0 || T < 0 || d < 0) return SCONE_EINVAL;
  *bytes = B > SCONE_BWD_CHUNK ? (uint64_t)T * wpe_chunks_of(B) * (uint64_t)d * sizeof(float) : 0;
  return SCONE_OK;
}

extern "C" int scone_backward_wpe(scone_handle *h, const void *d_grad_out, int32_t grad_dtype, int32_t B, int32_t T, int64_t n_pos,
                                  float *d_grad_wpe_out, void *d_scratch, scone_stream_t stream) {
  static const char who[] = "scone_backward_wpe";
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0");
  if (grad_dtype != SCONE_DT_F32 && grad_dtype != SCONE_DT_F16 && grad_dtype != SCONE_DT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who, "bad grad_dtype");
  if (B < 0 || T < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative B or T");
  if (n_pos <= 0) return scone_refuse(h, SCONE_EINVAL, who, "n_pos must be positive");
  if ((long long)B * T > 0x7FFFFFFFll) return scone_refuse(h, SCONE_EINVAL, who, "B * T above 2^31 - 1");
  if ((long long)B * T == 0) return SCONE_OK;
  const int n_chunks = wpe_chunks_of(B);
  if (!d_grad_out || !d_grad_wpe_out || (n_chunks > 1 && !d_scratch)) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  const int rows = (int)(n_pos < T ? n_pos : T);  // rows t >= n_pos do not exist: their positions are out of range in the lookup
  const int d = h->cfg.dim;
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  float *partial = reinterpret_cast<float *>(d_scratch);
  if (grad_dtype == SCONE_DT_F32)
    launch_wpe_chunks<SCONE_DT_F32>(d_grad_out, B, T, rows, d, n_chunks, d_grad_wpe_out, partial, s);
  else if (grad_dtype == SCONE_DT_F16)
    launch_wpe_chunks<SCONE_DT_F16>(d_grad_out, B, T, rows, d, n_chunks, d_grad_wpe_out, partial, s);
  else
    launch_wpe_chunks<SCONE_DT_BF16>(d_grad_out, B, T, rows, d, n_chunks, d_grad_wpe_out, partial, s);
  SCONE_HIP(h, hipGetLastError());
  if (n_chunks > 1) {
    const unsigned long long items = (unsigned long long)rows * ((d + 255) / 256);
    hipLaunchKernelGGL(k_wpe_combine, dim3(scone_capped_blocks((items + 3) / 4)), dim3(IDX_THREADS), 0, s, partial, rows, d, n_chunks,
                       d_grad_wpe_out);
    SCONE_HIP(h, hipGetLastError());
  }
  return SCONE_OK;
}
