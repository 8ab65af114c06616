// The lookup's backward: deterministic sparse row gradients of the f-gram table (include/scone_hip.h, "backward").
//
// The gradient of a table row is the sum, over every (position p, place k) that lists the row, of grad_out[p, :] (times
// 1 / K_p for the mean).  It needs the id lists and grad_out only -- never a table row -- so this file stands beside the lookup
// kernels, not inside them, and works for every row format, placement and shard.
//
// Plan (scone_backward_plan*): match with the lookup's own launchers (or take the caller's CSR lists), expand the records to
// (row, p) pairs in (p, k) order, sort them stably by row (rocPRIM radix_sort_pairs over the bits of n_rows), flag and scan the
// segment heads, cut every segment into chunks of SCONE_BWD_CHUNK consecutive references and give every chunk of a row with
// several chunks a partial slot.  The pair arrays are sized by the most references the batch can have and padded with the key
// n_rows, which sorts behind every row, so that the only host round trip is the one that returns U and the reference count.
//
// Rows (scone_backward_rows): a wave owns a chunk; lanes own 16-byte column pieces of grad_out; the references are walked in
// order, 16 loads per lane in flight, `a = a + c` the only dependent chain.  A one-chunk row is stored straight to grad_rows, the
// chunks of a longer row to their partial slots, which a second small pass adds in chunk order.  No atomics on floating-point
// data anywhere: the result is a pure function of the inputs.  The multiply (mean) and the add are separate roundings -- the
// library is built with -ffp-contract=off and nothing here calls fmaf.
#include "scone_bwd_plan.h"
#include "scone_common.h"

#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

namespace {

constexpr int BWD_THREADS = 256;

__device__ __forceinline__ uint32_t ell_counts(const int32_t *__restrict__ ell, long long p, int W) { return (uint32_t)ell[p * W + W - 2]; }

// ---------------------------------------------------------------- plan helpers (short grid-stride kernels)
// K_own, K_full and the mean's weight of every position, from the match records
__global__ void k_bwd_count_ell(const int32_t *__restrict__ ell, long long ntok, int W, uint32_t *__restrict__ kown,
                                int32_t *__restrict__ kfull, float *__restrict__ w) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p <= ntok; p += (long long)gridDim.x * blockDim.x) {
    if (p == ntok) {
      kown[p] = 0;  // the scan's last element: ref_off[ntok] = the total
      continue;
    }
    const uint32_t c = ell_counts(ell, p, W);
    const int kf = (int)(c >> 8);
    kown[p] = c & 0xFFu;
    kfull[p] = kf;
    w[p] = kf > 0 ? 1.0f / (float)kf : 1.0f;
  }
}

__global__ void k_bwd_expand_ell(const int32_t *__restrict__ ell, long long ntok, int W, const uint32_t *__restrict__ ref_off,
                                 uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < ntok; p += (long long)gridDim.x * blockDim.x) {
    const uint32_t k = ell_counts(ell, p, W) & 0xFFu;
    const uint32_t at = ref_off[p];
    for (uint32_t j = 0; j < k && j < (uint32_t)(W - 2); ++j) {
      keys[at + j] = (uint32_t)ell[p * W + j];
      vals[at + j] = (uint32_t)p;
    }
  }
}

// the caller's lists: K_p = the list length; ids outside the table raise SCONE_ST_BAD_ID and are skipped, ids outside the owned
// range are skipped.  Offsets are clamped into [0, total], so no read leaves d_ids[0, total) whatever they hold.  Clamped lists
// may overlap (offsets that decrease and rise again), so the owned references of a batch can outnumber `total`: the count
// kernel adds them up (an integer atomic: the sum does not depend on the order) and that sum sizes the plan.
__device__ __forceinline__ void csr_range(const int32_t *__restrict__ off, long long p, long long total, long long *b, long long *e) {
  long long lo = off[p], hi = off[p + 1];
  lo = lo < 0 ? 0 : (lo > total ? total : lo);
  hi = hi < lo ? lo : (hi > total ? total : hi);
  *b = lo, *e = hi;
}

__global__ void k_bwd_count_csr(const int32_t *__restrict__ off, const int32_t *__restrict__ ids, long long ntok, long long total,
                                long long n_rows, long long row_begin, long long row_end, uint32_t *__restrict__ kown,
                                int32_t *__restrict__ kfull, float *__restrict__ w, uint32_t *__restrict__ status,
                                unsigned long long *__restrict__ own_total) {
  unsigned long long mine = 0;  // owned references of this thread's positions: one atomic per wave after the loop
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p <= ntok; p += (long long)gridDim.x * blockDim.x) {
    if (p == ntok) {
      kown[p] = 0;
      continue;
    }
    long long b, e;
    csr_range(off, p, total, &b, &e);
    uint32_t own = 0;
    bool bad = false;
    for (long long i = b; i < e; ++i) {
      const long long id = ids[i];
      if (id < 0 || id >= n_rows)
        bad = true;
      else if (id >= row_begin && id < row_end)
        ++own;
    }
    if (bad) atomicOr(status, SCONE_ST_BAD_ID);
    mine += own;
    const long long kf = e - b;
    kown[p] = own;
    kfull[p] = (int32_t)kf;
    w[p] = kf > 0 ? 1.0f / (float)kf : 1.0f;
  }
  // every lane of the wave is here (the loop has no early exit); blockDim.x is a multiple of 64
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) mine += __shfl_down(mine, step, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(own_total, mine);
}

__global__ void k_bwd_expand_csr(const int32_t *__restrict__ off, const int32_t *__restrict__ ids, long long ntok, long long total,
                                 long long n_rows, long long row_begin, long long row_end, const uint32_t *__restrict__ ref_off,
                                 uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < ntok; p += (long long)gridDim.x * blockDim.x) {
    long long b, e;
    csr_range(off, p, total, &b, &e);
    uint32_t at = ref_off[p];
    const uint32_t end = ref_off[p + 1];
    for (long long i = b; i < e; ++i) {
      const long long id = ids[i];
      if (id >= 0 && id < n_rows && id >= row_begin && id < row_end && at < end) {
        keys[at] = (uint32_t)id;
        vals[at] = (uint32_t)p;
        ++at;
      }
    }
  }
}

// keys [n_refs, max_refs) = pad_key (n_rows): behind every row after the sort
__global__ void k_bwd_pad(const uint32_t *__restrict__ ref_total, unsigned long long max_refs, uint32_t pad_key,
                          uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const unsigned long long n = *ref_total;
  for (unsigned long long i = n + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < max_refs;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    keys[i] = pad_key;
    vals[i] = 0;
  }
}

__global__ void k_bwd_heads(const uint32_t *__restrict__ keys, unsigned long long max_refs, uint32_t pad_key,
                            uint32_t *__restrict__ flags) {
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < max_refs;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const uint32_t k = keys[i];
    flags[i] = (k < pad_key && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
  }
}

// incl = inclusive scan of the head flags: segment u starts where incl steps to u + 1
__global__ void k_bwd_segs(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ incl,
                           unsigned long long max_refs, const uint32_t *__restrict__ ref_total, uint32_t *__restrict__ seg_start,
                           uint32_t *__restrict__ row_id, bwd_meta *__restrict__ meta) {
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < max_refs;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    if (flags[i]) {
      seg_start[incl[i] - 1] = (uint32_t)i;
      row_id[incl[i] - 1] = keys[i];
    }
    if (i == max_refs - 1) {
      const uint32_t U = incl[i];
      seg_start[U] = *ref_total;
      meta->n_segs = U;
      meta->n_refs = *ref_total;
    }
  }
}

// chunks and partial slots of every segment; entries [U, seg_cap] are zero so that the scans' totals stand at [seg_cap]
__global__ void k_bwd_seg_chunks(const uint32_t *__restrict__ seg_start, const bwd_meta *__restrict__ meta, unsigned long long seg_cap,
                                 uint32_t *__restrict__ nch, unsigned long long *__restrict__ nmulti) {
  const uint32_t U = meta->n_segs;
  for (unsigned long long u = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; u <= seg_cap;
       u += (unsigned long long)gridDim.x * blockDim.x) {
    uint32_t c = 0;
    if (u < U) {
      const uint32_t len = seg_start[u + 1] - seg_start[u];
      c = (len + SCONE_BWD_CHUNK - 1) / SCONE_BWD_CHUNK;
    }
    nch[u] = c;
    nmulti[u] = c > 1 ? ((1ull << 32) | c) : 0ull;  // high word: rows with several chunks; low word: their chunks = slots
  }
}

__global__ void k_bwd_fill(const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ ch_base,
                           const unsigned long long *__restrict__ multi_base, unsigned long long seg_cap, bwd_meta *__restrict__ meta,
                           bwd_chunk *__restrict__ chunks, bwd_multi *__restrict__ multi) {
  const uint32_t U = meta->n_segs;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    meta->n_chunks = ch_base[seg_cap];
    meta->n_multi = (uint32_t)(multi_base[seg_cap] >> 32);
    meta->n_slots = (uint32_t)(multi_base[seg_cap] & 0xFFFFFFFFull);
  }
  for (unsigned long long u = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; u < U;
       u += (unsigned long long)gridDim.x * blockDim.x) {
    const uint32_t b = seg_start[u], len = seg_start[u + 1] - b;
    const uint32_t n = (len + SCONE_BWD_CHUNK - 1) / SCONE_BWD_CHUNK;
    const uint32_t c0 = ch_base[u];
    const uint32_t slot0 = (uint32_t)(multi_base[u] & 0xFFFFFFFFull);
    for (uint32_t j = 0; j < n; ++j) {
      bwd_chunk c;
      c.begin = b + j * SCONE_BWD_CHUNK;
      c.count = (j + 1 < n) ? (uint32_t)SCONE_BWD_CHUNK : len - j * SCONE_BWD_CHUNK;
      c.dest = n > 1 ? slot0 + j : (uint32_t)u;
      c.partial = n > 1 ? 1u : 0u;
      chunks[c0 + j] = c;
    }
    if (n > 1) {
      bwd_multi mr;
      mr.seg = (uint32_t)u, mr.slot0 = slot0, mr.n = n, mr.pad = 0;
      multi[multi_base[u] >> 32] = mr;
    }
  }
}

__global__ void k_bwd_row_ids(const uint32_t *__restrict__ row_id, uint32_t U, int64_t *__restrict__ out) {
  for (unsigned long long u = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; u < U;
       u += (unsigned long long)gridDim.x * blockDim.x)
    out[u] = (int64_t)row_id[u];
}

// ---------------------------------------------------------------- chunk pass (the walk itself: scone_bwd_plan.h)
// A wave owns a chunk.  Lane l owns the 16-byte pieces l, l + 64, .. (NT of them) of a column tile of NT * 64 pieces; wider rows
// loop over column tiles OUTSIDE the reference walk, so the NT * E accumulators stay in registers.  The references are walked
// 16 / NT at a time (16 independent 16-byte loads per lane in flight whatever the tile width: a chunk of a hot row is one
// dependent chain of memory latencies otherwise), what is left four at a time, then one by one.
template <int DT, int NT, bool MEAN>
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_chunks(const bwd_chunk *__restrict__ chunks, uint32_t n_chunks,
                                                            const uint32_t *__restrict__ ref_p, const float *__restrict__ w,
                                                            const uint8_t *__restrict__ g, int d, float *__restrict__ grad_rows,
                                                            float *__restrict__ partial) {
  constexpr int E = bwd_piece<DT>::E;
  const int lane = threadIdx.x & 63;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BWD_THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t wave_stride = gridDim.x * (BWD_THREADS / 64);
  const int pieces = d / E;
  const size_t row_bytes = (size_t)d * (DT == SCONE_DT_F32 ? 4 : 2);
  for (uint32_t ci = wave0; ci < n_chunks; ci += wave_stride) {
    const bwd_chunk c = chunks[ci];
    const uint32_t begin = __builtin_amdgcn_readfirstlane(c.begin), count = __builtin_amdgcn_readfirstlane(c.count);
    float *dst = (__builtin_amdgcn_readfirstlane(c.partial) ? partial : grad_rows) + (size_t)__builtin_amdgcn_readfirstlane(c.dest) * d;
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
      const uint8_t *gl = g + (size_t)(tile0 + lane) * 16;
      bwd_walk_chunk<DT, NT, MEAN>(rp, count, w, gl, row_bytes, on, acc);
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

// Second pass: a wave owns (row with several chunks, tile of 256 columns) and adds the row's partials in chunk order.
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_combine(const bwd_multi *__restrict__ multi, uint32_t n_multi,
                                                             const float *__restrict__ partial, int d, float *__restrict__ grad_rows) {
  const int lane = threadIdx.x & 63;
  const uint32_t col_tiles = (uint32_t)((d + 255) / 256);
  const unsigned long long items = (unsigned long long)n_multi * col_tiles;
  const unsigned long long wave0 = blockIdx.x * (unsigned long long)(BWD_THREADS / 64) + (threadIdx.x >> 6);
  const unsigned long long stride = gridDim.x * (unsigned long long)(BWD_THREADS / 64);
  for (unsigned long long it = wave0; it < items; it += stride) {
    const bwd_multi mr = multi[it / col_tiles];
    const int col = (int)(it % col_tiles) * 256 + lane * 4;
    if (col >= d) continue;  // d % 4 == 0: a lane's four columns are inside or outside together
    const float *src = partial + (size_t)mr.slot0 * d + col;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t j = 0;
    for (; j + 4 <= mr.n; j += 4) {
      float4 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const float4 *>(src + (size_t)(j + r) * d);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[0] = a[0] + v[r].x, a[1] = a[1] + v[r].y, a[2] = a[2] + v[r].z, a[3] = a[3] + v[r].w;
      }
    }
    for (; j < mr.n; ++j) {
      const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)j * d);
      a[0] = a[0] + v.x, a[1] = a[1] + v.y, a[2] = a[2] + v.z, a[3] = a[3] + v.w;
    }
    *reinterpret_cast<float4 *>(grad_rows + (size_t)mr.seg * d + col) = make_float4(a[0], a[1], a[2], a[3]);
  }
}

// ---------------------------------------------------------------- host side
unsigned blocks_for(unsigned long long n) { return scone_capped_blocks((n + BWD_THREADS - 1) / BWD_THREADS); }

// device scratch that lives for one plan call
struct tmp_buf {
  void *p = nullptr;
  ~tmp_buf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
  template <typename T>
  T *as() { return reinterpret_cast<T *>(p); }
};

int bits_for(unsigned long long values) {  // bits that hold 0 .. values - 1
  int b = 1;
  while (b < 32 && (1ull << b) < values) ++b;
  return b;
}

void plan_free(scone_bwd_plan *pl) {
  if (!pl) return;
  scone_device_guard guard(pl->device);
  if (pl->d_kfull) (void)hipFree(pl->d_kfull);
  if (pl->d_w) (void)hipFree(pl->d_w);
  if (pl->d_ref_p) (void)hipFree(pl->d_ref_p);
  if (pl->d_row_id) (void)hipFree(pl->d_row_id);
  if (pl->d_chunks) (void)hipFree(pl->d_chunks);
  if (pl->d_multi) (void)hipFree(pl->d_multi);
  if (pl->d_partial) (void)hipFree(pl->d_partial);
  if (pl->d_meta) (void)hipFree(pl->d_meta);
  delete pl;
}

// Everything after the argument checks.  `max_refs` is the most references the batch can have; the caller's lists are counted
// here first (their clamped ranges may overlap, so d_offsets[ntok] bounds nothing) and max_refs becomes the owned count.
int plan_build(scone_handle *h, scone_bwd_plan *pl, const bwd_plan_src &src, unsigned long long max_refs, hipStream_t s) {
  const long long ntok = pl->ntok;
  SCONE_HIP(h, hipMalloc(&pl->d_meta, sizeof(bwd_meta)));
  SCONE_HIP(h, hipMemsetAsync(pl->d_meta, 0, sizeof(bwd_meta), s));
  tmp_buf kown, own_total;
  if (src.kind == BWD_SRC_CSR && ntok > 0) {
    SCONE_HIP(h, hipMalloc(&pl->d_kfull, (size_t)ntok * 4));
    SCONE_HIP(h, hipMalloc(&pl->d_w, (size_t)ntok * 4));
    SCONE_HIP(h, kown.alloc((size_t)(ntok + 1) * 4));
    SCONE_HIP(h, own_total.alloc(8));
    SCONE_HIP(h, hipMemsetAsync(own_total.p, 0, 8, s));
    hipLaunchKernelGGL(k_bwd_count_csr, dim3(blocks_for(ntok + 1)), dim3(BWD_THREADS), 0, s, src.offsets, src.ids, ntok,
                       src.csr_total, (long long)h->cfg.n_rows, (long long)h->cfg.row_begin, (long long)h->cfg.row_end,
                       kown.as<uint32_t>(), pl->d_kfull, pl->d_w, h->d_status, own_total.as<unsigned long long>());
    SCONE_HIP(h, hipGetLastError());
    unsigned long long owned_refs = 0;
    SCONE_HIP(h, hipMemcpyAsync(&owned_refs, own_total.p, 8, hipMemcpyDeviceToHost, s));
    SCONE_HIP(h, hipStreamSynchronize(s));
    if (owned_refs >= (1ull << 32))
      return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_csr: too many references for one plan (they are numbered in 32 bits)");
    max_refs = owned_refs;
  }
  if (ntok == 0 || max_refs == 0) {  // an empty plan: no positions, or lists that hold no owned id
    if (ntok > 0 && !pl->d_kfull) {
      SCONE_HIP(h, hipMalloc(&pl->d_kfull, (size_t)ntok * 4));
      SCONE_HIP(h, hipMemsetAsync(pl->d_kfull, 0, (size_t)ntok * 4, s));
    }
    SCONE_HIP(h, hipStreamSynchronize(s));
    return SCONE_OK;
  }
  const bwd_plan_sizes z = src.kind == BWD_SRC_INDEX
                               ? scone_bwd_plan_sizes_ids(max_refs, (unsigned long long)src.n_ids, (unsigned long long)src.n_ids)
                               : scone_bwd_plan_sizes(h, max_refs);
  const unsigned long long seg_cap = z.seg_cap;

  if (!pl->d_kfull) SCONE_HIP(h, hipMalloc(&pl->d_kfull, (size_t)ntok * 4));
  if (!pl->d_w) SCONE_HIP(h, hipMalloc(&pl->d_w, (size_t)ntok * 4));
  SCONE_HIP(h, hipMalloc(&pl->d_ref_p, (size_t)max_refs * 4));
  SCONE_HIP(h, hipMalloc(&pl->d_row_id, (size_t)(seg_cap + 1) * 4));
  SCONE_HIP(h, hipMalloc(&pl->d_chunks, (size_t)z.chunk_cap * sizeof(bwd_chunk)));
  SCONE_HIP(h, hipMalloc(&pl->d_multi, (size_t)z.multi_cap * sizeof(bwd_multi)));

  tmp_buf ref_off, keys, keys2, vals, flags, incl, seg_start, nch, ch_base, nmulti, multi_base, scratch;
  if (!kown.p) SCONE_HIP(h, kown.alloc((size_t)(ntok + 1) * 4));
  SCONE_HIP(h, ref_off.alloc((size_t)(ntok + 1) * 4));
  SCONE_HIP(h, keys.alloc((size_t)max_refs * 4));
  SCONE_HIP(h, keys2.alloc((size_t)max_refs * 4));
  SCONE_HIP(h, vals.alloc((size_t)max_refs * 4));
  SCONE_HIP(h, flags.alloc((size_t)max_refs * 4));
  SCONE_HIP(h, incl.alloc((size_t)max_refs * 4));
  SCONE_HIP(h, seg_start.alloc((size_t)(seg_cap + 2) * 4));
  SCONE_HIP(h, nch.alloc((size_t)(seg_cap + 1) * 4));
  SCONE_HIP(h, ch_base.alloc((size_t)(seg_cap + 1) * 4));
  SCONE_HIP(h, nmulti.alloc((size_t)(seg_cap + 1) * 8));
  SCONE_HIP(h, multi_base.alloc((size_t)(seg_cap + 1) * 8));
  size_t need = 0;  // one scratch for the sort and the four scans
  SCONE_TRY(scone_bwd_plan_scratch(h, ntok, z, s, &need));
  SCONE_HIP(h, scratch.alloc(need));

  bwd_plan_bufs b = {};
  b.kfull = pl->d_kfull, b.w = pl->d_w, b.ref_p = pl->d_ref_p, b.row_id = pl->d_row_id, b.chunks = pl->d_chunks, b.multi = pl->d_multi;
  b.meta = pl->d_meta;
  b.kown = kown.as<uint32_t>(), b.ref_off = ref_off.as<uint32_t>();
  b.keys = keys.as<uint32_t>(), b.keys2 = keys2.as<uint32_t>(), b.vals = vals.as<uint32_t>();
  b.flags = flags.as<uint32_t>(), b.incl = incl.as<uint32_t>(), b.seg_start = seg_start.as<uint32_t>();
  b.nch = nch.as<uint32_t>(), b.ch_base = ch_base.as<uint32_t>();
  b.nmulti = nmulti.as<unsigned long long>(), b.multi_base = multi_base.as<unsigned long long>();
  b.scratch = scratch.p, b.scratch_bytes = need;
  SCONE_TRY(scone_bwd_plan_enqueue(h, src, ntok, z, b, s));
  // the one synchronisation: U, the reference count, and what sizes the partials buffer
  SCONE_HIP(h, hipMemcpyAsync(&pl->m, pl->d_meta, sizeof(bwd_meta), hipMemcpyDeviceToHost, s));
  SCONE_HIP(h, hipStreamSynchronize(s));
  if (pl->m.n_chunks > z.chunk_cap || pl->m.n_multi > z.multi_cap || pl->m.n_segs > seg_cap)
    return scone_fail(h, SCONE_ESTATE, "scone_backward_plan: inconsistent plan");
  if (pl->m.n_slots) SCONE_HIP(h, hipMalloc(&pl->d_partial, (size_t)pl->m.n_slots * pl->dim * sizeof(float)));
  return SCONE_OK;
}

int plan_common_checks(scone_handle *h, scone_bwd_plan **out, const char *who_dim, const char *who_d8) {
  if (!h) return SCONE_EINVAL;
  if (!out) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan: null out");
  *out = nullptr;
  if (h->cfg.dim == 0) return scone_fail(h, SCONE_EINVAL, who_dim);
  if (h->cfg.dim % 8 != 0) return scone_fail(h, SCONE_EINVAL, who_d8);
  if (h->cfg.n_rows >= 0xFFFFFFFFull) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan: tables of 2^32 - 1 rows or more are not supported");
  return SCONE_OK;
}

int plan_finish(scone_handle *h, scone_bwd_plan *pl, int rc, scone_bwd_plan **out, uint64_t *h_n_rows, uint64_t *h_n_refs) {
  if (rc) {
    plan_free(pl);
    return rc;
  }
  *out = pl;
  if (h_n_rows) *h_n_rows = pl->m.n_segs;
  if (h_n_refs) *h_n_refs = pl->m.n_refs;
  return SCONE_OK;
}

scone_bwd_plan *plan_new(scone_handle *h, long long ntok) {
  scone_bwd_plan *pl = new (std::nothrow) scone_bwd_plan();
  if (!pl) return nullptr;
  pl->h = h, pl->device = h->device, pl->dim = h->cfg.dim, pl->ntok = ntok;
  return pl;
}

template <int DT, bool MEAN>
void launch_chunks_nt(const scone_bwd_plan *pl, const void *g, float *grad_rows, hipStream_t s) {
  static constexpr int E = DT == SCONE_DT_F32 ? 4 : 8;  // elements of a 16-byte piece of grad_out: the column tile is chosen from it
  static_assert(E == bwd_piece<DT>::E, "the tile rule below counts scone_bwd_plan.h's pieces");
  const int d = pl->dim;
  const int pieces = d / E;
  const unsigned blocks = scone_capped_blocks(((unsigned long long)pl->m.n_chunks + 3) / 4);
  const uint8_t *gb = reinterpret_cast<const uint8_t *>(g);
#define SCONE_BWD_LAUNCH(NT)                                                                                                   \
  hipLaunchKernelGGL((k_bwd_chunks<DT, NT, MEAN>), dim3(blocks), dim3(BWD_THREADS), 0, s, pl->d_chunks, pl->m.n_chunks, pl->d_ref_p, \
                     pl->d_w, gb, d, grad_rows, pl->d_partial)
  if (pieces <= 64)
    SCONE_BWD_LAUNCH(1);
  else if (pieces <= 128)
    SCONE_BWD_LAUNCH(2);
  else
    SCONE_BWD_LAUNCH(4);
#undef SCONE_BWD_LAUNCH
}

template <int DT>
void launch_chunks(const scone_bwd_plan *pl, const void *g, int reduce, float *grad_rows, hipStream_t s) {
  if (reduce == SCONE_REDUCE_MEAN)
    launch_chunks_nt<DT, true>(pl, g, grad_rows, s);
  else
    launch_chunks_nt<DT, false>(pl, g, grad_rows, s);
}

}  // namespace

// ---------------------------------------------------------------- the build both plan forms share (scone_bwd_plan.h)
unsigned long long scone_bwd_cand_per_token(const scone_handle *h) {
  if (h->cfg.lookup_mode == SCONE_MODE_LONGEST_SUFFIX) return 1;
  return (unsigned long long)h->cfg.max_n * (h->cfg.max_n + 1) / 2;
}

bwd_plan_sizes scone_bwd_plan_sizes(const scone_handle *h, unsigned long long max_refs) {
  return scone_bwd_plan_sizes_ids(max_refs, h->cfg.n_rows, h->cfg.row_end - h->cfg.row_begin);
}

bwd_plan_sizes scone_bwd_plan_sizes_ids(unsigned long long max_refs, unsigned long long n_ids, unsigned long long owned) {
  bwd_plan_sizes z;
  z.max_refs = max_refs;
  z.seg_cap = max_refs < owned ? max_refs : owned;
  z.chunk_cap = max_refs / SCONE_BWD_CHUNK + z.seg_cap + 1;
  z.multi_cap = max_refs / SCONE_BWD_CHUNK + 1;
  z.end_bit = bits_for(n_ids + 1);
  z.pad_key = (uint32_t)n_ids;
  return z;
}

int scone_bwd_scan_u32(scone_handle *h, void *scratch, size_t scratch_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s) {
  SCONE_HIP(h, rocprim::exclusive_scan(scratch, scratch_bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), s));
  return SCONE_OK;
}

int scone_bwd_plan_make(scone_handle *h, const bwd_plan_src &src, long long ntok, unsigned long long max_refs, scone_bwd_plan **out,
                        uint64_t *h_n_rows, uint64_t *h_n_refs, hipStream_t s) {
  scone_bwd_plan *pl = plan_new(h, ntok);
  if (!pl) return scone_fail(h, SCONE_ENOMEM, "scone_backward_plan: out of memory");
  pl->index = src.kind == BWD_SRC_INDEX;
  return plan_finish(h, pl, plan_build(h, pl, src, max_refs, s), out, h_n_rows, h_n_refs);
}

int scone_bwd_plan_scratch(scone_handle *h, long long ntok, const bwd_plan_sizes &z, hipStream_t s, size_t *need_out) {
  uint32_t *u = nullptr;
  unsigned long long *ull = nullptr;
  size_t need = 0, n1 = 0;
  SCONE_HIP(h, rocprim::radix_sort_pairs(nullptr, n1, u, u, u, u, (size_t)z.max_refs, 0, z.end_bit, s));
  need = n1;
  SCONE_HIP(h, rocprim::exclusive_scan(nullptr, n1, u, u, 0u, (size_t)(ntok + 1), rocprim::plus<uint32_t>(), s));
  need = n1 > need ? n1 : need;
  SCONE_HIP(h, rocprim::inclusive_scan(nullptr, n1, u, u, (size_t)z.max_refs, rocprim::plus<uint32_t>(), s));
  need = n1 > need ? n1 : need;
  SCONE_HIP(h, rocprim::exclusive_scan(nullptr, n1, u, u, 0u, (size_t)(z.seg_cap + 1), rocprim::plus<uint32_t>(), s));
  need = n1 > need ? n1 : need;
  SCONE_HIP(h, rocprim::exclusive_scan(nullptr, n1, ull, ull, 0ull, (size_t)(z.seg_cap + 1), rocprim::plus<unsigned long long>(), s));
  need = n1 > need ? n1 : need;
  *need_out = need;
  return SCONE_OK;
}

int scone_bwd_plan_enqueue(scone_handle *h, const bwd_plan_src &src, long long ntok, const bwd_plan_sizes &z, const bwd_plan_bufs &b,
                           hipStream_t s) {
  const unsigned long long n_rows = h->cfg.n_rows, max_refs = z.max_refs, seg_cap = z.seg_cap;
  const uint32_t pad_key = z.pad_key;
  const size_t need = b.scratch_bytes;
  size_t n1;
  // (1) id lists -> K_own / K_full / w per position, the reference offsets, the (row, p) pairs in (p, k) order
  if (src.kind == BWD_SRC_INDEX) {
    SCONE_TRY(scone_bwd_index_pairs(h, src, ntok, b, s));
  } else if (src.kind == BWD_SRC_CSR) {  // counted by the caller
    n1 = need;
    SCONE_HIP(h, rocprim::exclusive_scan(b.scratch, n1, b.kown, b.ref_off, 0u, (size_t)(ntok + 1), rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_bwd_expand_csr, dim3(blocks_for(ntok)), dim3(BWD_THREADS), 0, s, src.offsets, src.ids, ntok, src.csr_total,
                       (long long)n_rows, (long long)h->cfg.row_begin, (long long)h->cfg.row_end, b.ref_off, b.keys, b.vals);
    SCONE_HIP(h, hipGetLastError());
  } else {
    // the workspace of THIS stream, held only while the match that writes its records and the kernels that read them are
    // enqueued -- unless the records have a buffer of their own
    scone_ws_lock ws(b.ell ? nullptr : scone_ws_acquire(h, s));
    int32_t *ell = b.ell;
    if (!ell) {
      if (!ws.w) return scone_fail(h, SCONE_ENOMEM, "scone_backward_plan: out of memory");
      SCONE_TRY(scone_ensure_ell(h, ws.w, ntok));
      ell = ws.w->d_ell;
    }
    int rc;
    if (src.kind == BWD_SRC_RECT)
      rc = scone_launch_match_ell(h, src.tok, src.B, src.T, ell, s);
    else
      rc = scone_launch_match_ell_varlen(h, src.tok, src.cu, src.n_seqs, ntok, ell, nullptr, s);
    if (rc) return rc;
    const int W = SCONE_ELL_W(h->cfg.max_n);
    hipLaunchKernelGGL(k_bwd_count_ell, dim3(blocks_for(ntok + 1)), dim3(BWD_THREADS), 0, s, ell, ntok, W, b.kown, b.kfull, b.w);
    SCONE_HIP(h, hipGetLastError());
    n1 = need;
    SCONE_HIP(h, rocprim::exclusive_scan(b.scratch, n1, b.kown, b.ref_off, 0u, (size_t)(ntok + 1), rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_bwd_expand_ell, dim3(blocks_for(ntok)), dim3(BWD_THREADS), 0, s, ell, ntok, W, b.ref_off, b.keys, b.vals);
    SCONE_HIP(h, hipGetLastError());
  }
  const uint32_t *ref_total = b.ref_off + ntok;
  hipLaunchKernelGGL(k_bwd_pad, dim3(blocks_for(max_refs)), dim3(BWD_THREADS), 0, s, ref_total, max_refs, pad_key, b.keys, b.vals);
  SCONE_HIP(h, hipGetLastError());
  // (2) stable sort by row: the references of a row stay in (p, k) order
  n1 = need;
  SCONE_HIP(h, rocprim::radix_sort_pairs(b.scratch, n1, b.keys, b.keys2, b.vals, b.ref_p, (size_t)max_refs, 0, z.end_bit, s));
  // (3) segment heads -> U, segment starts, row ids
  hipLaunchKernelGGL(k_bwd_heads, dim3(blocks_for(max_refs)), dim3(BWD_THREADS), 0, s, b.keys2, max_refs, pad_key, b.flags);
  SCONE_HIP(h, hipGetLastError());
  n1 = need;
  SCONE_HIP(h, rocprim::inclusive_scan(b.scratch, n1, b.flags, b.incl, (size_t)max_refs, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_bwd_segs, dim3(blocks_for(max_refs)), dim3(BWD_THREADS), 0, s, b.keys2, b.flags, b.incl, max_refs, ref_total,
                     b.seg_start, b.row_id, b.meta);
  SCONE_HIP(h, hipGetLastError());
  // (4) chunk descriptors and the partial slot of every chunk of a row with several
  hipLaunchKernelGGL(k_bwd_seg_chunks, dim3(blocks_for(seg_cap + 1)), dim3(BWD_THREADS), 0, s, b.seg_start, b.meta, seg_cap, b.nch,
                     b.nmulti);
  SCONE_HIP(h, hipGetLastError());
  n1 = need;
  SCONE_HIP(h, rocprim::exclusive_scan(b.scratch, n1, b.nch, b.ch_base, 0u, (size_t)(seg_cap + 1), rocprim::plus<uint32_t>(), s));
  n1 = need;
  SCONE_HIP(h, rocprim::exclusive_scan(b.scratch, n1, b.nmulti, b.multi_base, 0ull, (size_t)(seg_cap + 1),
                                       rocprim::plus<unsigned long long>(), s));
  hipLaunchKernelGGL(k_bwd_fill, dim3(blocks_for(seg_cap)), dim3(BWD_THREADS), 0, s, b.seg_start, b.ch_base, b.multi_base, seg_cap,
                     b.meta, b.chunks, b.multi);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

// Above this many items rocPRIM's radix sort leaves its merge sort for the onesweep kernels, which use a private segment
// (scratch): the one kind of kernel in a plan that a captured graph is not given (scone_backward_plan_dn refuses the capture).
unsigned long long scone_bwd_sort_merge_limit() { return rocprim::radix_sort_config<>::merge_sort_limit; }

int scone_bwd_plan_checks(scone_handle *h, const char *who) {
  if (h->cfg.dim == 0) return scone_refuse(h, SCONE_EINVAL, who, "handle has no table (dim == 0)");
  if (h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0");
  if (h->cfg.n_rows >= 0xFFFFFFFFull) return scone_refuse(h, SCONE_EINVAL, who, "tables of 2^32 - 1 rows or more are not supported");
  return SCONE_OK;
}

extern "C" int scone_backward_chunk(void) { return SCONE_BWD_CHUNK; }

extern "C" int scone_backward_plan(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, scone_bwd_plan **out,
                                   uint64_t *h_n_rows, uint64_t *h_n_refs, scone_stream_t stream) {
  int rc = plan_common_checks(h, out, "scone_backward_plan: handle has no table (dim == 0)", "scone_backward_plan: needs d % 8 == 0");
  if (rc) return rc;
  if (B < 0 || T < 0) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan: negative B or T");
  const long long ntok = (long long)B * T;
  if (ntok > 0 && !d_tok) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan: null d_tok");
  const unsigned long long max_refs = (unsigned long long)ntok * scone_bwd_cand_per_token(h);
  if (ntok > 0x7FFFFFFFll || max_refs >= (1ull << 32))
    return scone_fail(h, SCONE_EINVAL, "scone_backward_plan: too many tokens for one plan (references are numbered in 32 bits)");
  SCONE_ON_DEVICE(h);
  scone_bwd_plan *pl = plan_new(h, ntok);
  if (!pl) return scone_fail(h, SCONE_ENOMEM, "scone_backward_plan: out of memory");
  bwd_plan_src src = {};
  src.kind = BWD_SRC_RECT, src.tok = d_tok, src.B = B, src.T = T;
  return plan_finish(h, pl, plan_build(h, pl, src, max_refs, (hipStream_t)stream), out, h_n_rows, h_n_refs);
}

extern "C" int scone_backward_plan_varlen(scone_handle *h, const int32_t *d_tok, const int32_t *d_cu_seqlens, int32_t n_seqs,
                                          int64_t total_tokens, scone_bwd_plan **out, uint64_t *h_n_rows, uint64_t *h_n_refs,
                                          scone_stream_t stream) {
  int rc = plan_common_checks(h, out, "scone_backward_plan_varlen: handle has no table (dim == 0)",
                              "scone_backward_plan_varlen: needs d % 8 == 0");
  if (rc) return rc;
  if (n_seqs < 0 || total_tokens < 0) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_varlen: negative n_seqs or total_tokens");
  if (total_tokens > 0x7FFFFFFFll) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_varlen: total_tokens above 2^31 - 1");
  if (h->cfg.stage_tokens && h->rows_host)
    return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_varlen: not for stage_tokens > 0 (as scone_embed_varlen)");
  long long ntok = total_tokens;
  if (n_seqs == 0) ntok = 0;  // as scone_embed_varlen: a batch without sequences is empty
  if (ntok > 0 && (!d_tok || !d_cu_seqlens)) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_varlen: null pointer");
  const unsigned long long max_refs = (unsigned long long)ntok * scone_bwd_cand_per_token(h);
  if (max_refs >= (1ull << 32))
    return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_varlen: too many tokens for one plan (references are numbered in 32 bits)");
  SCONE_ON_DEVICE(h);
  scone_bwd_plan *pl = plan_new(h, ntok);
  if (!pl) return scone_fail(h, SCONE_ENOMEM, "scone_backward_plan_varlen: out of memory");
  bwd_plan_src src = {};
  src.kind = BWD_SRC_PACKED, src.tok = d_tok, src.cu = d_cu_seqlens, src.n_seqs = n_seqs;
  return plan_finish(h, pl, plan_build(h, pl, src, max_refs, (hipStream_t)stream), out, h_n_rows, h_n_refs);
}

extern "C" int scone_backward_plan_csr(scone_handle *h, const int32_t *d_offsets, const int32_t *d_ids, int64_t ntok,
                                       scone_bwd_plan **out, uint64_t *h_n_rows, uint64_t *h_n_refs, scone_stream_t stream) {
  int rc = plan_common_checks(h, out, "scone_backward_plan_csr: handle has no table (dim == 0)", "scone_backward_plan_csr: needs d % 8 == 0");
  if (rc) return rc;
  if (ntok < 0) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_csr: negative ntok");
  if (ntok > 0x7FFFFFFFll) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_csr: ntok above 2^31 - 1");
  if (ntok > 0 && !d_offsets) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_csr: null d_offsets");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  // the lists' total is the caller's, on the device: this form reads it first (one more synchronisation than the token forms)
  int32_t total = 0;
  if (ntok > 0) {
    SCONE_HIP(h, hipMemcpyAsync(&total, d_offsets + ntok, 4, hipMemcpyDeviceToHost, s));
    SCONE_HIP(h, hipStreamSynchronize(s));
    if (total < 0) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_csr: negative d_offsets[ntok]");
    if (total > 0 && !d_ids) return scone_fail(h, SCONE_EINVAL, "scone_backward_plan_csr: null d_ids");
  }
  scone_bwd_plan *pl = plan_new(h, ntok);
  if (!pl) return scone_fail(h, SCONE_ENOMEM, "scone_backward_plan_csr: out of memory");
  bwd_plan_src src = {};
  src.kind = BWD_SRC_CSR, src.offsets = d_offsets, src.ids = d_ids, src.csr_total = total;
  return plan_finish(h, pl, plan_build(h, pl, src, (unsigned long long)total, s), out, h_n_rows, h_n_refs);
}

extern "C" int scone_backward_rows(scone_handle *h, scone_bwd_plan *plan, const void *d_grad_out, int32_t grad_dtype,
                                   int32_t reduce, int64_t *d_row_ids_out, float *d_grad_rows_out, uint64_t rows_cap,
                                   scone_stream_t stream) {
  if (!h) return SCONE_EINVAL;
  if (!plan) return scone_fail(h, SCONE_EINVAL, "scone_backward_rows: null plan");
  if (plan->h != h) return scone_fail(h, SCONE_EINVAL, "scone_backward_rows: the plan belongs to another handle");
  if (grad_dtype != SCONE_DT_F32 && grad_dtype != SCONE_DT_F16 && grad_dtype != SCONE_DT_BF16)
    return scone_fail(h, SCONE_EINVAL, "scone_backward_rows: bad grad_dtype");
  if (reduce != SCONE_REDUCE_MEAN && reduce != SCONE_REDUCE_SUM) return scone_fail(h, SCONE_EINVAL, "scone_backward_rows: bad reduce");
  const uint32_t U = plan->m.n_segs;
  if (rows_cap < U) return scone_fail(h, SCONE_ERANGE, "scone_backward_rows: rows_cap below the plan's n_rows");
  if (U == 0) return SCONE_OK;
  if (!d_grad_out || !d_row_ids_out || !d_grad_rows_out) return scone_fail(h, SCONE_EINVAL, "scone_backward_rows: null pointer");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_bwd_row_ids, dim3(blocks_for(U)), dim3(BWD_THREADS), 0, s, plan->d_row_id, U, d_row_ids_out);
  SCONE_HIP(h, hipGetLastError());
  if (grad_dtype == SCONE_DT_F32)
    launch_chunks<SCONE_DT_F32>(plan, d_grad_out, reduce, d_grad_rows_out, s);
  else if (grad_dtype == SCONE_DT_F16)
    launch_chunks<SCONE_DT_F16>(plan, d_grad_out, reduce, d_grad_rows_out, s);
  else
    launch_chunks<SCONE_DT_BF16>(plan, d_grad_out, reduce, d_grad_rows_out, s);
  SCONE_HIP(h, hipGetLastError());
  if (plan->m.n_multi) {
    const unsigned long long items = (unsigned long long)plan->m.n_multi * ((plan->dim + 255) / 256);
    hipLaunchKernelGGL(k_bwd_combine, dim3(scone_capped_blocks((items + 3) / 4)), dim3(BWD_THREADS), 0, s, plan->d_multi, plan->m.n_multi,
                       plan->d_partial, plan->dim, d_grad_rows_out);
    SCONE_HIP(h, hipGetLastError());
  }
  return SCONE_OK;
}

extern "C" int scone_backward_row_ids(scone_handle *h, scone_bwd_plan *plan, int64_t *d_row_ids_out, uint64_t rows_cap,
                                      scone_stream_t stream) {
  if (!h) return SCONE_EINVAL;
  if (!plan) return scone_fail(h, SCONE_EINVAL, "scone_backward_row_ids: null plan");
  if (plan->h != h) return scone_fail(h, SCONE_EINVAL, "scone_backward_row_ids: the plan belongs to another handle");
  const uint32_t U = plan->m.n_segs;
  if (rows_cap < U) return scone_fail(h, SCONE_ERANGE, "scone_backward_row_ids: rows_cap below the plan's n_rows");
  if (U == 0) return SCONE_OK;
  if (!d_row_ids_out) return scone_fail(h, SCONE_EINVAL, "scone_backward_row_ids: null pointer");
  SCONE_ON_DEVICE(h);
  hipLaunchKernelGGL(k_bwd_row_ids, dim3(blocks_for(U)), dim3(BWD_THREADS), 0, (hipStream_t)stream, plan->d_row_id, U, d_row_ids_out);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_backward_counts(scone_handle *h, scone_bwd_plan *plan, int32_t *d_k_out, scone_stream_t stream) {
  if (!h) return SCONE_EINVAL;
  if (!plan) return scone_fail(h, SCONE_EINVAL, "scone_backward_counts: null plan");
  if (plan->h != h) return scone_fail(h, SCONE_EINVAL, "scone_backward_counts: the plan belongs to another handle");
  if (plan->ntok == 0) return SCONE_OK;
  if (!d_k_out) return scone_fail(h, SCONE_EINVAL, "scone_backward_counts: null d_k_out");
  SCONE_ON_DEVICE(h);
  SCONE_HIP(h, hipMemcpyAsync(d_k_out, plan->d_kfull, (size_t)plan->ntok * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SCONE_OK;
}

extern "C" void scone_backward_plan_destroy(scone_bwd_plan *plan) { plan_free(plan); }
