// Gradient accumulation (include/scone_hip.h, "gradient accumulation"): the sum of two sparse row gradients, each an ascending
// list of distinct int64 row ids with fp32 rows [n, d] -- what scone_backward_rows returns.  scone_grad_merge_map builds the
// union of the id lists and the maps between the three row numberings; scone_grad_merge_rows moves the rows.
//
// Map.  Every id finds its place by a lower-bound binary search in the OTHER list, so nothing here sorts and no id is ever an
// address.  With la(j) = #{a < b[j]} and lb(i) = #{b < a[i]}, and x[j] = 1 where b[j] has no partner in a, S = the exclusive
// scan of x over [0, n_b] (S[n_b] = the total):
//   pos_b[j] = la(j) + S[j]      pos_a[i] = i + S[lb(i)]      n_out = n_a + S[n_b]
// A search returns a value in [0, n] whatever the list holds and S[k] <= k, so pos_a < n_a + n_b and pos_b < n_a + n_b for ANY
// input: a list outside the contract (not ascending, not distinct) raises SCONE_ST_BAD_ID by a neighbour check and scatters to
// unspecified places inside the buffers.  src_a / src_b are filled with "absent" over their whole capacity first, so an entry
// is absent or an index the scatter wrote.
// Four short launches: (1) fill + search of b + flags and their sums per tile of 1024, (2) one workgroup scans the tile sums,
// (3) every tile scans its flags in place, (4) the scatter of both lists.  The scan is this file's (two levels, integer, any
// grid gives the same values), so scone_grad_merge_scratch is arithmetic and needs no device.
//
// Rows.  k_grad_merge_rows has the shape of the row-parallel optimizer kernels (scone_opt_rows.h): one wave per output row, a
// grid-stride loop, lane l owns the 16-byte pieces l, l + 64, .. and a row is walked in blocks of OPT_NT * 64 pieces with the
// loads of BOTH operands issued before the block's adds.  A row one list has is copied (float4 loads and stores: every bit,
// -0.0 and NaN payloads included); a row both have is a + b, one IEEE fp32 add (-ffp-contract=off, subnormals kept).  One
// launch, plain vector stores, no atomics.
#include "scone_common.h"
#include "scone_opt_rows.h"  // OPT_NT and the grid of a row-parallel optimizer kernel

namespace {

constexpr int GM_THREADS = 256;
constexpr int GM_PER = 4;                        // consecutive flags per thread of a tile
constexpr int GM_TILE = GM_THREADS * GM_PER;     // 1024
constexpr uint32_t GM_ABSENT = 0xFFFFFFFFu;

// #{x[k] < v}: in [0, n] whatever x holds
__device__ __forceinline__ unsigned long long gm_lower_bound(const int64_t *__restrict__ x, unsigned long long n, int64_t v) {
  unsigned long long lo = 0, hi = n;
  while (lo < hi) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    if (x[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// the exclusive scan of one value per thread over the workgroup (256 threads); *total = the workgroup's sum.  lds: 4 words.
__device__ __forceinline__ uint32_t gm_block_excl(uint32_t v, uint32_t *lds, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t o = __shfl_up(inc, s, 64);
    if (lane >= s) inc += o;
  }
  __syncthreads();  // lds may still be read by the previous call
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < GM_THREADS / 64; ++k) {
    const uint32_t t = lds[k];
    if (k < wave) base += t;
    sum += t;
  }
  *total = sum;
  return base + inc - v;
}

// (1) src_a / src_b = absent over [0, n_a + n_b); for every j <= n_b: pos_b[j] = la(j) (its final value needs S), flag[j] = b[j]
// has no partner (flag[n_b] = 0); tile_sum[t] = the flags of tile t.  A workgroup owns whole tiles.
__global__ __launch_bounds__(GM_THREADS) void k_gm_search_b(const int64_t *__restrict__ a, unsigned long long n_a,
                                                            const int64_t *__restrict__ b, unsigned long long n_b,
                                                            uint32_t *__restrict__ src_a, uint32_t *__restrict__ src_b,
                                                            uint32_t *__restrict__ pos_b, uint32_t *__restrict__ flag,
                                                            uint32_t *__restrict__ tile_sum, unsigned long long n_tiles,
                                                            uint32_t *__restrict__ status) {
  __shared__ uint32_t lds[GM_THREADS / 64];
  const unsigned long long cap = n_a + n_b;
  for (unsigned long long i = blockIdx.x * (unsigned long long)GM_THREADS + threadIdx.x; i < cap;
       i += (unsigned long long)gridDim.x * GM_THREADS) {
    src_a[i] = GM_ABSENT;
    src_b[i] = GM_ABSENT;
  }
  bool bad = false;
  for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < GM_PER; ++k) {
      const unsigned long long j = t * GM_TILE + (unsigned long long)threadIdx.x * GM_PER + k;
      if (j > n_b) continue;
      uint32_t f = 0;
      if (j < n_b) {
        const int64_t v = b[j];
        if (j > 0 && v <= b[j - 1]) bad = true;
        const unsigned long long la = gm_lower_bound(a, n_a, v);
        f = (la < n_a && a[la] == v) ? 0u : 1u;
        pos_b[j] = (uint32_t)la;
      }
      flag[j] = f;
      mine += f;
    }
    uint32_t total;
    (void)gm_block_excl(mine, lds, &total);
    if (threadIdx.x == 0) tile_sum[t] = total;
  }
  if (bad) atomicOr(status, SCONE_ST_BAD_ID);
}

// (2) one workgroup: tile_sum -> its exclusive scan, in place
__global__ __launch_bounds__(GM_THREADS) void k_gm_scan_tiles(uint32_t *__restrict__ tile_sum, unsigned long long n_tiles) {
  __shared__ uint32_t lds[GM_THREADS / 64];
  uint32_t carry = 0;
  for (unsigned long long t0 = 0; t0 < n_tiles; t0 += GM_THREADS) {
    const unsigned long long t = t0 + threadIdx.x;
    const uint32_t v = t < n_tiles ? tile_sum[t] : 0u;
    uint32_t total;
    const uint32_t ex = gm_block_excl(v, lds, &total);
    if (t < n_tiles) tile_sum[t] = carry + ex;
    carry += total;
  }
}

// (3) flag -> S, in place: a tile reads its own flags only
__global__ __launch_bounds__(GM_THREADS) void k_gm_scan_flags(uint32_t *__restrict__ flag, unsigned long long n_b,
                                                              const uint32_t *__restrict__ tile_off, unsigned long long n_tiles) {
  __shared__ uint32_t lds[GM_THREADS / 64];
  for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const unsigned long long j0 = t * GM_TILE + (unsigned long long)threadIdx.x * GM_PER;
    uint32_t f[GM_PER], mine = 0;
#pragma unroll
    for (int k = 0; k < GM_PER; ++k) {
      f[k] = j0 + k <= n_b ? flag[j0 + k] : 0u;
      mine += f[k];
    }
    uint32_t total;
    uint32_t run = tile_off[t] + gm_block_excl(mine, lds, &total);
#pragma unroll
    for (int k = 0; k < GM_PER; ++k) {
      if (j0 + k <= n_b) flag[j0 + k] = run;
      run += f[k];
    }
  }
}

// (4) the scatter: threads [0, n_b) place b, threads [n_b, n_b + n_a) place a
__global__ __launch_bounds__(GM_THREADS) void k_gm_scatter(const int64_t *__restrict__ a, unsigned long long n_a,
                                                           const int64_t *__restrict__ b, unsigned long long n_b,
                                                           const uint32_t *__restrict__ S, int64_t *__restrict__ ids_out,
                                                           uint32_t *__restrict__ src_a, uint32_t *__restrict__ src_b,
                                                           uint32_t *__restrict__ pos_a, uint32_t *__restrict__ pos_b,
                                                           uint64_t *__restrict__ n_out, uint32_t *__restrict__ status) {
  const unsigned long long cap = n_a + n_b;
  bool bad = false;
  for (unsigned long long i = blockIdx.x * (unsigned long long)GM_THREADS + threadIdx.x; i < cap;
       i += (unsigned long long)gridDim.x * GM_THREADS) {
    if (i < n_b) {
      const unsigned long long pos = (unsigned long long)pos_b[i] + S[i];  // <= n_a + i
      pos_b[i] = (uint32_t)pos;
      ids_out[pos] = b[i];
      src_b[pos] = (uint32_t)i;
    } else {
      const unsigned long long k = i - n_b;
      const int64_t v = a[k];
      if (k > 0 && v <= a[k - 1]) bad = true;
      const unsigned long long pos = k + S[gm_lower_bound(b, n_b, v)];  // <= k + n_b
      pos_a[k] = (uint32_t)pos;
      ids_out[pos] = v;
      src_a[pos] = (uint32_t)k;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = n_a + S[n_b];
  if (bad) atomicOr(status, SCONE_ST_BAD_ID);
}

unsigned long long gm_tiles(unsigned long long n_b) { return n_b / GM_TILE + 1; }  // tiles of the n_b + 1 flags
unsigned long long gm_flag_words(unsigned long long n_b) { return (n_b + 1 + 3) & ~3ull; }  // the tile words start 16-byte aligned

// One wave per output row.  sa / sb are wave-uniform; a row neither list has (only a list outside the contract leaves one) is
// stored as zeros, so the call's output is a function of its inputs.
__global__ __launch_bounds__(256) void k_grad_merge_rows(const uint32_t *__restrict__ src_a, const uint32_t *__restrict__ src_b,
                                                         unsigned long long n_out, int d, const float *__restrict__ rows_a,
                                                         const float *__restrict__ rows_b, float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int pieces = d >> 2;
  const unsigned long long nwaves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  for (unsigned long long r = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_out; r += nwaves) {
    const uint32_t sa = __builtin_amdgcn_readfirstlane(src_a[r]), sb = __builtin_amdgcn_readfirstlane(src_b[r]);
    const bool has_a = sa != GM_ABSENT, has_b = sb != GM_ABSENT;
    const float4 *A = reinterpret_cast<const float4 *>(rows_a + (has_a ? sa : 0u) * (unsigned long long)d);
    const float4 *B = reinterpret_cast<const float4 *>(rows_b + (has_b ? sb : 0u) * (unsigned long long)d);
    float4 *O = reinterpret_cast<float4 *>(out + r * (unsigned long long)d);
    if (has_a && has_b) {  // wave-uniform
      for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
        float4 x[OPT_NT], y[OPT_NT];
#pragma unroll
        for (int t = 0; t < OPT_NT; ++t) {  // both streams of a block in flight before any add
          const int p = p0 + t * 64 + lane;
          if (p < pieces) {
            x[t] = A[p];
            y[t] = B[p];
          }
        }
#pragma unroll
        for (int t = 0; t < OPT_NT; ++t) {
          const int p = p0 + t * 64 + lane;
          if (p < pieces) O[p] = make_float4(x[t].x + y[t].x, x[t].y + y[t].y, x[t].z + y[t].z, x[t].w + y[t].w);
        }
      }
    } else {  // a copy, never an add to zero
      const float4 *S = has_a ? A : B;
      const bool any = has_a || has_b;
      for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
        float4 x[OPT_NT];
#pragma unroll
        for (int t = 0; t < OPT_NT; ++t) {
          const int p = p0 + t * 64 + lane;
          x[t] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p < pieces && any) x[t] = S[p];
        }
#pragma unroll
        for (int t = 0; t < OPT_NT; ++t) {
          const int p = p0 + t * 64 + lane;
          if (p < pieces) O[p] = x[t];
        }
      }
    }
  }
}

}  // namespace

extern "C" int scone_grad_merge_scratch(uint64_t n_a, uint64_t n_b, uint64_t *bytes) {
  if (!bytes) return SCONE_EINVAL;
  (void)n_a;  // the scratch holds a word per id of b (and per tile of 1024): a is searched, never flagged
  *bytes = 4 * (gm_flag_words(n_b) + ((gm_tiles(n_b) + 3) & ~3ull));
  return SCONE_OK;
}

extern "C" int scone_grad_merge_map(scone_handle *h, const int64_t *d_ids_a, uint64_t n_a, const int64_t *d_ids_b, uint64_t n_b,
                                    int64_t *d_ids_out, uint32_t *d_src_a, uint32_t *d_src_b, uint32_t *d_pos_a, uint32_t *d_pos_b,
                                    void *d_scratch, uint64_t *d_n_out, uint64_t *h_n_out, scone_stream_t stream) {
  const char *who = "scone_grad_merge_map";
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (n_a >= 0xFFFFFFFFull || n_b >= 0xFFFFFFFFull || n_a + n_b >= 0xFFFFFFFFull)
    return scone_refuse(h, SCONE_EINVAL, who, "n_a + n_b must be below 2^32 - 1 (rows are numbered in 32 bits, 0xFFFFFFFF is absent)");
  if (!d_scratch || !d_n_out) return scone_refuse(h, SCONE_EINVAL, who, "null d_scratch or d_n_out");
  if ((n_a && (!d_ids_a || !d_pos_a)) || (n_b && (!d_ids_b || !d_pos_b)) || ((n_a + n_b) && (!d_ids_out || !d_src_a || !d_src_b)))
    return scone_refuse(h, SCONE_EINVAL, who, "null pointer (only the arrays of an empty list may be null)");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  uint32_t *flag = reinterpret_cast<uint32_t *>(d_scratch);
  uint32_t *tile = flag + gm_flag_words(n_b);
  const unsigned long long tiles = gm_tiles(n_b), cap = n_a + n_b;
  const unsigned long long fill_blocks = (cap + GM_THREADS - 1) / GM_THREADS;
  hipLaunchKernelGGL(k_gm_search_b, dim3(scone_capped_blocks(tiles > fill_blocks ? tiles : fill_blocks)), dim3(GM_THREADS), 0, s, d_ids_a,
                     (unsigned long long)n_a, d_ids_b, (unsigned long long)n_b, d_src_a, d_src_b, d_pos_b, flag, tile, tiles, h->d_status);
  hipLaunchKernelGGL(k_gm_scan_tiles, dim3(1), dim3(GM_THREADS), 0, s, tile, tiles);
  hipLaunchKernelGGL(k_gm_scan_flags, dim3(scone_capped_blocks(tiles)), dim3(GM_THREADS), 0, s, flag, (unsigned long long)n_b, tile, tiles);
  hipLaunchKernelGGL(k_gm_scatter, dim3(scone_capped_blocks(fill_blocks)), dim3(GM_THREADS), 0, s, d_ids_a, (unsigned long long)n_a,
                     d_ids_b, (unsigned long long)n_b, flag, d_ids_out, d_src_a, d_src_b, d_pos_a, d_pos_b, d_n_out, h->d_status);
  SCONE_HIP(h, hipGetLastError());
  if (h_n_out) {
    SCONE_HIP(h, hipMemcpyAsync(h_n_out, d_n_out, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SCONE_HIP(h, hipStreamSynchronize(s));
  }
  return SCONE_OK;
}

extern "C" int scone_grad_merge_rows(scone_handle *h, const uint32_t *d_src_a, const uint32_t *d_src_b, uint64_t n_out,
                                     const float *d_rows_a, const float *d_rows_b, float *d_rows_out, scone_stream_t stream) {
  const char *who = "scone_grad_merge_rows";
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (h->cfg.dim % 4 != 0) return scone_refuse(h, SCONE_EINVAL, who, "dim must be a multiple of 4 (rows are moved in 16-byte pieces)");
  if (n_out >= 0xFFFFFFFFull) return scone_refuse(h, SCONE_EINVAL, who, "n_out must be below 2^32 - 1");
  if (d_rows_out && (d_rows_out == d_rows_a || d_rows_out == d_rows_b))
    return scone_refuse(h, SCONE_EINVAL, who, "the output must not overlap an input (d_rows_out equals d_rows_a or d_rows_b)");
  if (n_out == 0) return SCONE_OK;
  if (!d_src_a || !d_src_b || !d_rows_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_ON_DEVICE(h);
  unsigned blocks = scone_capped_blocks((n_out + 3) / 4);  // a wave per row, capped as scone_opt_step's grid is
  if (h->opt_max_blocks > 0 && blocks > (unsigned long long)h->opt_max_blocks) blocks = (unsigned)h->opt_max_blocks;
  hipLaunchKernelGGL(k_grad_merge_rows, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_src_a, d_src_b, (unsigned long long)n_out,
                     h->cfg.dim, d_rows_a, d_rows_b, d_rows_out);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}
