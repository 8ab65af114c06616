// The squared norm of the sparse table gradient and the control block the optimizer steps read (include/scone_hip.h, "gradient
// norm, clipping and skipped steps"): scone_grad_sqnorm reduces grad_rows [n, d] to one double in a fixed order, and
// scone_grad_ctl_set turns a few such terms into a clip coefficient and a skip flag that stay on the device.
//
// Shape.  k_grad_row_sq is k_opt_step's walk without the update: one wave per row, a grid-stride loop over the rows, lane l
// owns the 16-byte pieces l, l + 64, .. and a row is read in blocks of OPT_NT * 64 pieces whose loads are all issued before the
// block's arithmetic.  A lane adds its elements in ascending j whatever the block boundaries are; the lanes are combined by the
// butterfly of the lean step's row sum.  k_grad_tile_sq adds the 1024 row sums of a tile and k_grad_total_sq the tiles, each
// by 256 strided partial sums and a tree in LDS, so no sum depends on the grid, on SCONE_OPT_MAX_BLOCKS or on the run.
//
// Arithmetic.  IEEE double throughout.  (double)g * (double)g is exact (48 significant bits), so fma(x, x, a) rounds exactly as
// a + x * x does; every other operation is one addition.  No atomics; plain vector stores only.
#include "scone_common.h"
#include "scone_opt_rows.h"  // OPT_NT and the grid of a row-parallel optimizer kernel

#include <cmath>

namespace {

constexpr int GN_TILE = 1024;    // rows per tile: part of the contract
constexpr int GN_THREADS = 256;  // threads of a tile's and the total's workgroup: part of the contract

__device__ __forceinline__ double gn_add_sq(double a, const float4 &g) {
  a = fma((double)g.x, (double)g.x, a);
  a = fma((double)g.y, (double)g.y, a);
  a = fma((double)g.z, (double)g.z, a);
  a = fma((double)g.w, (double)g.w, a);
  return a;
}

// Q_r: one wave per row; a piece the lane does not have is all +0.0f, and a + (+0.0 * +0.0) keeps every bit of a (a is never -0.0)
// NSRC (scone_opt_rows.h): n by value, or the count scone_grad_sqnorm_dn reads from the device
template <typename NSRC>
__global__ __launch_bounds__(256) void k_grad_row_sq(const float *__restrict__ grad, NSRC nsrc, int d, double *__restrict__ row_sq) {
  const unsigned long long n = nsrc.get();
  const int lane = threadIdx.x & 63;
  const int pieces = d >> 2;
  const unsigned long long nwaves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  for (unsigned long long r = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n; r += nwaves) {
    const float4 *G = reinterpret_cast<const float4 *>(grad + r * (unsigned long long)d);
    double a = 0.0;
    for (int p0 = 0; p0 < pieces; p0 += OPT_NT * 64) {
      float4 g[OPT_NT];
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) {
        const int p = p0 + t * 64 + lane;
        g[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < pieces) g[t] = G[p];
      }
#pragma unroll
      for (int t = 0; t < OPT_NT; ++t) a = gn_add_sq(a, g[t]);
    }
    for (int s = 32; s >= 1; s >>= 1) a = a + __shfl_xor(a, s, 64);  // the contract's butterfly: every lane ends with the same bits
    if (lane == 0) row_sq[r] = a;
  }
}

// the tree both reductions end with: b_t = b_t + b_(t + s) for t < s, s = 128 .. 1; thread 0 returns the sum
__device__ __forceinline__ double gn_tree(double b, double *lds) {
  const int t = threadIdx.x;
  lds[t] = b;
  __syncthreads();
  for (int s = GN_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  return lds[0];
}

// P_k: the row sums of tile k; thread t adds rows 1024k + t + 256i, i = 0 .. 3, in range
// (scone_grad_sqnorm_dn: the tiles are those of n_cap rows; one past n adds nothing and is stored as +0.0)
template <typename NSRC>
__global__ __launch_bounds__(GN_THREADS) void k_grad_tile_sq(const double *__restrict__ row_sq, NSRC nsrc, unsigned long long n_tiles,
                                                             double *__restrict__ tile_sq) {
  __shared__ double lds[GN_THREADS];
  const unsigned long long n = nsrc.get();
  for (unsigned long long k = blockIdx.x; k < n_tiles; k += gridDim.x) {
    double b = 0.0;
#pragma unroll
    for (int i = 0; i < GN_TILE / GN_THREADS; ++i) {
      const unsigned long long r = k * GN_TILE + threadIdx.x + (unsigned long long)i * GN_THREADS;
      if (r < n) b = b + row_sq[r];
    }
    const double sum = gn_tree(b, lds);
    if (threadIdx.x == 0) tile_sq[k] = sum;
    __syncthreads();  // lds is reused by the next tile of this workgroup
  }
}

// the total: one workgroup; thread t adds P_(t + 256i) in ascending i
__global__ __launch_bounds__(GN_THREADS) void k_grad_total_sq(const double *__restrict__ tile_sq, unsigned long long n_tiles,
                                                              double *__restrict__ out) {
  __shared__ double lds[GN_THREADS];
  double b = 0.0;
  for (unsigned long long k = threadIdx.x; k < n_tiles; k += GN_THREADS) b = b + tile_sq[k];
  const double sum = gn_tree(b, lds);
  if (threadIdx.x == 0) *out = sum;
}

// where k_grad_ctl_set takes grad_scale from: the launch (checked finite on the host), or the scone_opt_hyper block of
// scone_grad_ctl_set_dh, where a value that is not finite can only be answered on the device
struct gn_scale_value {
  double v;
  __device__ __forceinline__ double get() const { return v; }
  __device__ __forceinline__ bool finite(double) const { return true; }
};
struct gn_scale_device {
  const scone_opt_hyper *__restrict__ hy;
  __device__ __forceinline__ double get() const { return hy->grad_scale; }
  __device__ __forceinline__ bool finite(double x) const {
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
  }
};

// one thread, every operation one IEEE double rounding; sqrt and / are hipcc's correctly rounded defaults
template <typename GSRC>
__global__ void k_grad_ctl_set(const double *__restrict__ terms, int n_terms, GSRC gsrc, double max_norm, int skip_nonfinite,
                               scone_grad_ctl *__restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double grad_scale = gsrc.get();
  double total = 0.0;
  for (int i = 0; i < n_terms; ++i) total = total + terms[i];
  const double norm64 = sqrt(total) * fabs(grad_scale);
  const double c = max_norm / (norm64 + 1e-6);
  const bool finite = ((unsigned long long)__double_as_longlong(total) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
  ctl->sqnorm = total;
  ctl->norm = (float)norm64;
  ctl->coef = c < 1.0 ? (float)c : 1.0f;  // a NaN compares false: 1.0f
  ctl->skip = skip_nonfinite && !finite ? 1u : 0u;
  ctl->reserved = 0u;
  if (!gsrc.finite(grad_scale)) {  // scone_grad_ctl_set_dh only: the by-value call has refused such a scale on the host
    ctl->coef = 1.0f;
    ctl->skip = 1u;
  }
}

unsigned long long gn_tiles(unsigned long long n) { return n / GN_TILE + (n % GN_TILE ? 1 : 0); }

}  // namespace

extern "C" int scone_grad_sqnorm_scratch(uint64_t n, uint64_t *n_doubles) {
  if (!n_doubles) return SCONE_EINVAL;
  *n_doubles = n + gn_tiles(n);
  return SCONE_OK;
}

extern "C" int scone_grad_sqnorm(scone_handle *h, const float *d_grad_rows, uint64_t n, double *d_scratch, double *d_sq_out,
                                 scone_stream_t stream) {
  const char *who = "scone_grad_sqnorm";
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (h->cfg.dim % 4 != 0) return scone_refuse(h, SCONE_EINVAL, who, "dim must be a multiple of 4 (rows are read in 16-byte pieces)");
  if (!d_sq_out) return scone_refuse(h, SCONE_EINVAL, who, "null d_sq_out");
  if (n > 0 && (!d_grad_rows || !d_scratch)) return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_grad_rows and d_scratch are needed when n > 0)");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  const unsigned long long tiles = gn_tiles(n);
  if (n > 0) {
    unsigned blocks = scone_capped_blocks((n + 3) / 4);  // a wave per row, capped as scone_opt_step's grid is
    if (h->opt_max_blocks > 0 && blocks > (unsigned long long)h->opt_max_blocks) blocks = (unsigned)h->opt_max_blocks;
    hipLaunchKernelGGL(k_grad_row_sq<opt_n_value>, dim3(blocks), dim3(256), 0, s, d_grad_rows, opt_n_value{n}, h->cfg.dim, d_scratch);
    hipLaunchKernelGGL(k_grad_tile_sq<opt_n_value>, dim3(scone_capped_blocks(tiles)), dim3(GN_THREADS), 0, s, d_scratch, opt_n_value{n},
                       tiles, d_scratch + n);
  }
  hipLaunchKernelGGL(k_grad_total_sq, dim3(1), dim3(GN_THREADS), 0, s, d_scratch ? d_scratch + n : nullptr, tiles, d_sq_out);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_grad_sqnorm_dn(scone_handle *h, const float *d_grad_rows, const uint64_t *d_n, uint64_t n_cap, double *d_scratch,
                                    double *d_sq_out, scone_stream_t stream) {
  const char *who = "scone_grad_sqnorm_dn";
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (h->cfg.dim % 4 != 0) return scone_refuse(h, SCONE_EINVAL, who, "dim must be a multiple of 4 (rows are read in 16-byte pieces)");
  if (!d_sq_out) return scone_refuse(h, SCONE_EINVAL, who, "null d_sq_out");
  if (!d_n) return scone_refuse(h, SCONE_EINVAL, who, "null d_n");
  if (n_cap > 0 && (!d_grad_rows || !d_scratch))
    return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_grad_rows and d_scratch are needed when n_cap > 0)");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  const opt_n_device nsrc{reinterpret_cast<const unsigned long long *>(d_n), n_cap};
  const unsigned long long tiles = gn_tiles(n_cap);  // every tile of the capacity: those past n hold +0.0
  if (n_cap > 0) {
    unsigned blocks = scone_capped_blocks((n_cap + 3) / 4);  // a wave per row, capped as scone_opt_step's grid is
    if (h->opt_max_blocks > 0 && blocks > (unsigned long long)h->opt_max_blocks) blocks = (unsigned)h->opt_max_blocks;
    hipLaunchKernelGGL(k_grad_row_sq<opt_n_device>, dim3(blocks), dim3(256), 0, s, d_grad_rows, nsrc, h->cfg.dim, d_scratch);
    hipLaunchKernelGGL(k_grad_tile_sq<opt_n_device>, dim3(scone_capped_blocks(tiles)), dim3(GN_THREADS), 0, s, d_scratch, nsrc, tiles,
                       d_scratch + n_cap);
  }
  hipLaunchKernelGGL(k_grad_total_sq, dim3(1), dim3(GN_THREADS), 0, s, d_scratch ? d_scratch + n_cap : nullptr, tiles, d_sq_out);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_grad_ctl_set(scone_handle *h, const double *d_terms, int32_t n_terms, double grad_scale, double max_norm,
                                  int32_t skip_nonfinite, scone_grad_ctl *d_ctl, scone_stream_t stream) {
  const char *who = "scone_grad_ctl_set";
  if (!h) return SCONE_EINVAL;
  if (n_terms < 1 || n_terms > 64) return scone_refuse(h, SCONE_EINVAL, who, "n_terms must be 1 .. 64");
  if (!d_terms || !d_ctl) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  if (!std::isfinite(grad_scale)) return scone_refuse(h, SCONE_EINVAL, who, "grad_scale must be finite");
  if (!(max_norm > 0.0)) return scone_refuse(h, SCONE_EINVAL, who, "max_norm must be > 0 (+inf: no clipping)");
  SCONE_ON_DEVICE(h);
  hipLaunchKernelGGL(k_grad_ctl_set<gn_scale_value>, dim3(1), dim3(1), 0, (hipStream_t)stream, d_terms, (int)n_terms,
                     gn_scale_value{grad_scale}, max_norm, (int)skip_nonfinite, d_ctl);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_grad_ctl_set_dh(scone_handle *h, const double *d_terms, int32_t n_terms, const scone_opt_hyper *d_hyper,
                                     double max_norm, int32_t skip_nonfinite, scone_grad_ctl *d_ctl, void *stream) {
  const char *who = "scone_grad_ctl_set_dh";
  if (!h) return SCONE_EINVAL;
  if (n_terms < 1 || n_terms > 64) return scone_refuse(h, SCONE_EINVAL, who, "n_terms must be 1 .. 64");
  if (!d_terms || !d_ctl) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  if (!d_hyper) return scone_refuse(h, SCONE_EINVAL, who, "null d_hyper");
  if (!(max_norm > 0.0)) return scone_refuse(h, SCONE_EINVAL, who, "max_norm must be > 0 (+inf: no clipping)");
  SCONE_ON_DEVICE(h);
  hipLaunchKernelGGL(k_grad_ctl_set<gn_scale_device>, dim3(1), dim3(1), 0, (hipStream_t)stream, d_terms, (int)n_terms,
                     gn_scale_device{d_hyper}, max_norm, (int)skip_nonfinite, d_ctl);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}
