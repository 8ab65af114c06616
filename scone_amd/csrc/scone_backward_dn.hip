// The backward whose counts stay on the device (include/scone_hip.h, "backward and optimizer step without a host
// synchronisation").  A scone_bwd_ctx owns, at the worst-case sizes of a batch of max_tokens positions, every buffer
// scone_backward_plan allocates per call: the match records, the scratch of the build, the plan arrays and the partial slots.
// scone_backward_plan_dn runs the SAME enqueue sequence as scone_backward_plan (scone_bwd_plan_enqueue, scone_backward.hip) over
// those buffers and stops before the readback: bwd_meta stays in the context.  scone_backward_rows_dn then walks the plan with
// kernels that read U, the chunk count and the multi-chunk row count from bwd_meta -- wave-uniform scalar loads -- over grids
// sized from the host-known bounds, grid-stride.  The walk of a chunk is scone_bwd_plan.h's, the one k_bwd_chunks uses, and the
// partials are added in chunk order as k_bwd_combine adds them: the bits are those of scone_backward_rows.
//
// Nothing here synchronises, allocates or frees after scone_backward_ctx_create; scone_backward_ctx_counts is the one
// synchronising read.  No atomics on floating-point data; the one atomic is the integer atomicOr on the status word.
#include "scone_bwd_plan.h"
#include "scone_common.h"

#include <new>

struct scone_bwd_ctx {
  scone_handle *h = nullptr;
  int device = 0;
  int dim = 0;
  long long max_tokens = 0;
  bwd_plan_sizes cap = {};           // the sizes at max_tokens
  unsigned long long slot_cap = 0;   // partial slots at cap.max_refs (scone_backward_ctx_partial_slots)
  // the current plan: host-known bounds only -- its counts are in d_meta
  long long ntok = 0;
  bwd_plan_sizes cur = {};
  void *slab = nullptr;  // everything below is carved from it
  uint64_t bytes = 0;
  bwd_plan_bufs b = {};
  float *d_partial = nullptr;  // [slot_cap, dim]
};

namespace {

constexpr int BWD_THREADS = 256;

// what the caller's buffers and the context's arrays hold: a plan outside them is refused by every workgroup before a store
struct bwd_dn_caps {
  unsigned long long rows_cap, chunk_cap, multi_cap, slot_cap;
};

__device__ __forceinline__ bool dn_fits(const bwd_meta *__restrict__ m, const bwd_dn_caps &c) {
  return m->n_segs <= c.rows_cap && m->n_chunks <= c.chunk_cap && m->n_multi <= c.multi_cap && m->n_slots <= c.slot_cap;
}

// *d_n_out and the row ids.  U > rows_cap: *d_n_out = 0, SCONE_ST_ROWS_OVERFLOW, and no other store by any kernel of the call.
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_head_dn(const bwd_meta *__restrict__ meta, bwd_dn_caps caps,
                                                             const uint32_t *__restrict__ row_id, int64_t *__restrict__ out,
                                                             unsigned long long *__restrict__ n_out, uint32_t *__restrict__ status) {
  const bool ok = dn_fits(meta, caps);
  const uint32_t U = meta->n_segs;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *n_out = ok ? U : 0ull;
    if (!ok) atomicOr(status, SCONE_ST_ROWS_OVERFLOW);
  }
  if (!ok) return;
  for (unsigned long long u = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; u < U;
       u += (unsigned long long)gridDim.x * blockDim.x)
    out[u] = (int64_t)row_id[u];
}

__global__ void k_bwd_zero_n(unsigned long long *__restrict__ n_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = 0ull;
}

// k_bwd_chunks (scone_backward.hip) with the chunk count read from the plan: a wave owns a chunk, grid-stride
template <int DT, int NT, bool MEAN>
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_chunks_dn(const bwd_meta *__restrict__ meta, bwd_dn_caps caps,
                                                               const bwd_chunk *__restrict__ chunks, const uint32_t *__restrict__ ref_p,
                                                               const float *__restrict__ w, const uint8_t *__restrict__ g, int d,
                                                               float *__restrict__ grad_rows, float *__restrict__ partial) {
  if (!dn_fits(meta, caps)) return;  // wave-uniform (scalar loads), before any store
  const uint32_t n_chunks = meta->n_chunks;
  constexpr int E = bwd_piece<DT>::E;
  const int lane = threadIdx.x & 63;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BWD_THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t wave_stride = gridDim.x * (BWD_THREADS / 64);
  const int pieces = d / E;
  const size_t row_bytes = (size_t)d * (DT == SCONE_DT_F32 ? 4 : 2);
  for (unsigned long long ci = wave0; ci < n_chunks; ci += wave_stride) {
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

// k_bwd_combine with the row count read from the plan: a wave owns (row with several chunks, tile of 256 columns)
__global__ __launch_bounds__(BWD_THREADS) void k_bwd_combine_dn(const bwd_meta *__restrict__ meta, bwd_dn_caps caps,
                                                                const bwd_multi *__restrict__ multi, const float *__restrict__ partial,
                                                                int d, float *__restrict__ grad_rows) {
  if (!dn_fits(meta, caps)) return;
  const uint32_t n_multi = meta->n_multi;
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
// The grids walk device counts grid-stride, so they need not cover the bound: a few resident rounds of the chip are enough, and
// a grid of the bound's size would mostly be workgroups that find nothing to do.
unsigned dn_blocks(const scone_handle *h, unsigned long long items_per_block_bound) {
  const unsigned long long chip = (unsigned long long)(h->n_cus > 0 ? h->n_cus : 256) * 64;
  return scone_capped_blocks(items_per_block_bound < chip ? items_per_block_bound : chip);
}

// Partial slots of a plan of R references, chunks of C: a row of r > C references has ceil(r / C) <= (r - 1) / C + 1 chunks.
// With m such rows holding R' <= R references, slots <= (R' - m) / C + m, and m <= R' / (C + 1), so
//   slots <= R' / C + m (1 - 1 / C) <= R' (1 / C + (C - 1) / (C (C + 1))) = 2 R' / (C + 1) <= 2 R / (C + 1),
// reached when every row has C + 1 references.  An integer below a real bound is below its floor.
unsigned long long partial_slots_bound(unsigned long long max_refs) { return 2 * max_refs / (SCONE_BWD_CHUNK + 1); }
// ... and a slot is a chunk, of which a table of few rows has few
unsigned long long slot_bound(const bwd_plan_sizes &z) {
  const unsigned long long a = partial_slots_bound(z.max_refs);
  return a < z.chunk_cap ? a : z.chunk_cap;
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

template <int DT, bool MEAN>
void launch_chunks_dn_nt(const scone_bwd_ctx *c, const bwd_dn_caps &caps, const void *g, float *grad_rows, hipStream_t s) {
  constexpr int E = bwd_piece<DT>::E;
  const int d = c->dim;
  const int pieces = d / E;
  const unsigned blocks = dn_blocks(c->h, (c->cur.chunk_cap + 3) / 4);
  const uint8_t *gb = reinterpret_cast<const uint8_t *>(g);
#define SCONE_BWD_LAUNCH(NT)                                                                                               \
  hipLaunchKernelGGL((k_bwd_chunks_dn<DT, NT, MEAN>), dim3(blocks), dim3(BWD_THREADS), 0, s, c->b.meta, caps, c->b.chunks, \
                     c->b.ref_p, c->b.w, gb, d, grad_rows, c->d_partial)
  if (pieces <= 64)  // the tile rule of scone_backward_rows
    SCONE_BWD_LAUNCH(1);
  else if (pieces <= 128)
    SCONE_BWD_LAUNCH(2);
  else
    SCONE_BWD_LAUNCH(4);
#undef SCONE_BWD_LAUNCH
}

template <int DT>
void launch_chunks_dn(const scone_bwd_ctx *c, const bwd_dn_caps &caps, const void *g, int reduce, float *grad_rows, hipStream_t s) {
  if (reduce == SCONE_REDUCE_MEAN)
    launch_chunks_dn_nt<DT, true>(c, caps, g, grad_rows, s);
  else
    launch_chunks_dn_nt<DT, false>(c, caps, g, grad_rows, s);
}

int ctx_check(scone_handle *h, const scone_bwd_ctx *ctx, const char *who) {
  if (!h) return SCONE_EINVAL;
  if (!ctx) return scone_refuse(h, SCONE_EINVAL, who, "null ctx");
  if (ctx->h != h) return scone_refuse(h, SCONE_EINVAL, who, "the context belongs to another handle");
  return SCONE_OK;
}

// the build of scone_backward_plan over the context's buffers, without the readback
int plan_dn(scone_handle *h, scone_bwd_ctx *ctx, const char *who, const bwd_plan_src &src, long long ntok, hipStream_t s) {
  if (ntok > ctx->max_tokens) return scone_refuse(h, SCONE_ERANGE, who, "more positions than the context's max_tokens");
  const bwd_plan_sizes z = scone_bwd_plan_sizes(h, (unsigned long long)ntok * scone_bwd_cand_per_token(h));
  SCONE_ON_DEVICE(h);
  if (s != nullptr && z.max_refs > scone_bwd_sort_merge_limit()) {
    // Above rocPRIM's merge-sort limit the sort runs onesweep kernels, which use a private segment.  Replaying a captured graph
    // that holds them ended in a memory aperture violation on the runtime this was developed on (a plan of 6.3M references,
    // profiles/r24a), so such a plan is not captured: called eagerly it is as stream-ordered and sync-free as any other.
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess) {
      (void)hipGetLastError();
      capturing = hipStreamCaptureStatusNone;
    }
    if (capturing != hipStreamCaptureStatusNone)
      return scone_refuse(h, SCONE_EINVAL, who, "a plan of more than 2^20 possible references is not captured (call it eagerly)");
  }
  if (ntok > 0 && z.max_refs > 0) {
    // the bounds grow with ntok, so they fit whatever max_tokens was sized for; rocPRIM's scratch is asked again because
    // nothing promises that it grows with the size (the context took the largest of a ladder of sizes)
    size_t need = 0;
    SCONE_TRY(scone_bwd_plan_scratch(h, ntok, z, s, &need));
    if (need > ctx->b.scratch_bytes || z.max_refs > ctx->cap.max_refs || z.seg_cap > ctx->cap.seg_cap ||
        z.chunk_cap > ctx->cap.chunk_cap || z.multi_cap > ctx->cap.multi_cap || slot_bound(z) > ctx->slot_cap)
      return scone_refuse(h, SCONE_ESTATE, who, "the context's buffers do not hold this plan");
  }
  SCONE_HIP(h, hipMemsetAsync(ctx->b.meta, 0, sizeof(bwd_meta), s));
  ctx->ntok = ntok, ctx->cur = z;
  if (ntok == 0 || z.max_refs == 0) return SCONE_OK;  // an empty plan: every count is zero
  return scone_bwd_plan_enqueue(h, src, ntok, z, ctx->b, s);
}

}  // namespace

extern "C" int scone_backward_ctx_partial_slots(uint64_t max_refs, uint64_t *slots) {
  if (!slots || max_refs >= (1ull << 32)) return SCONE_EINVAL;
  *slots = partial_slots_bound(max_refs);
  return SCONE_OK;
}

extern "C" int scone_backward_ctx_create(scone_handle *h, int64_t max_tokens, scone_bwd_ctx **out) {
  const char *who = "scone_backward_ctx_create";
  if (!h) return SCONE_EINVAL;
  if (!out) return scone_refuse(h, SCONE_EINVAL, who, "null out");
  *out = nullptr;
  SCONE_TRY(scone_bwd_plan_checks(h, who));
  if (max_tokens < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative max_tokens");
  const unsigned long long cand = scone_bwd_cand_per_token(h);
  if (max_tokens > 0x7FFFFFFFll || (unsigned long long)max_tokens * cand >= (1ull << 32))
    return scone_refuse(h, SCONE_EINVAL, who, "too many tokens for one plan (references are numbered in 32 bits)");
  SCONE_ON_DEVICE(h);
  scone_bwd_ctx *c = new (std::nothrow) scone_bwd_ctx();
  if (!c) return scone_refuse(h, SCONE_ENOMEM, who, "out of memory");
  c->h = h, c->device = h->device, c->dim = h->cfg.dim, c->max_tokens = max_tokens;
  const unsigned long long ntok = (unsigned long long)max_tokens;
  c->cap = scone_bwd_plan_sizes(h, ntok * cand);
  c->slot_cap = slot_bound(c->cap);
  c->cur = scone_bwd_plan_sizes(h, 0);
  const bwd_plan_sizes &z = c->cap;
  // the bounds the buffers are sized by, held against each other: a row with slots has at least two, and a slot is a chunk
  if (c->slot_cap > z.chunk_cap || c->slot_cap > 2 * z.multi_cap) {
    delete c;
    return scone_refuse(h, SCONE_ESTATE, who, "inconsistent bounds");
  }
  // rocPRIM's scratch: the largest need over a ladder of batch sizes below max_tokens (plans re-check their own)
  size_t scratch = 0;
  for (unsigned long long t = ntok; t > 0; t >>= 1) {
    size_t need = 0;
    const int rc = scone_bwd_plan_scratch(h, (long long)t, scone_bwd_plan_sizes(h, t * cand), nullptr, &need);
    if (rc) {
      delete c;
      return rc;
    }
    scratch = need > scratch ? need : scratch;
  }
  const size_t W = SCONE_ELL_W(h->cfg.max_n);
  const size_t sizes[] = {
      sizeof(bwd_meta),                                  // 0 meta
      (size_t)ntok * 4,                                  // 1 kfull
      (size_t)ntok * 4,                                  // 2 w
      (size_t)z.max_refs * 4,                            // 3 ref_p
      (size_t)(z.seg_cap + 1) * 4,                       // 4 row_id
      (size_t)z.chunk_cap * sizeof(bwd_chunk),           // 5 chunks
      (size_t)z.multi_cap * sizeof(bwd_multi),           // 6 multi
      (size_t)(ntok + 1) * 4,                            // 7 kown
      (size_t)(ntok + 1) * 4,                            // 8 ref_off
      (size_t)z.max_refs * 4,                            // 9 keys
      (size_t)z.max_refs * 4,                            // 10 keys2
      (size_t)z.max_refs * 4,                            // 11 vals
      (size_t)z.max_refs * 4,                            // 12 flags
      (size_t)z.max_refs * 4,                            // 13 incl
      (size_t)(z.seg_cap + 2) * 4,                       // 14 seg_start
      (size_t)(z.seg_cap + 1) * 4,                       // 15 nch
      (size_t)(z.seg_cap + 1) * 4,                       // 16 ch_base
      (size_t)(z.seg_cap + 1) * 8,                       // 17 nmulti
      (size_t)(z.seg_cap + 1) * 8,                       // 18 multi_base
      scratch,                                           // 19 rocPRIM
      (size_t)ntok * W * 4,                              // 20 match records
      (size_t)c->slot_cap * (size_t)c->dim * 4,          // 21 partial slots
  };
  constexpr int NBUF = sizeof(sizes) / sizeof(sizes[0]);
  size_t off[NBUF + 1];
  off[0] = 0;
  for (int i = 0; i < NBUF; ++i) off[i + 1] = off[i] + up256(sizes[i] ? sizes[i] : 16);
  hipError_t e = hipMalloc(&c->slab, off[NBUF]);
  if (e == hipSuccess) e = hipMemset(c->slab, 0, up256(sizeof(bwd_meta)));  // no plan yet: an empty one
  if (e != hipSuccess) {
    if (c->slab) (void)hipFree(c->slab);
    delete c;
    return scone_hip_fail(h, e, "scone_backward_ctx_create: hipMalloc");
  }
  c->bytes = off[NBUF];
  uint8_t *base = reinterpret_cast<uint8_t *>(c->slab);
  auto at = [&](int i) { return reinterpret_cast<void *>(base + off[i]); };
  bwd_plan_bufs &b = c->b;
  b.meta = (bwd_meta *)at(0), b.kfull = (int32_t *)at(1), b.w = (float *)at(2), b.ref_p = (uint32_t *)at(3);
  b.row_id = (uint32_t *)at(4), b.chunks = (bwd_chunk *)at(5), b.multi = (bwd_multi *)at(6);
  b.kown = (uint32_t *)at(7), b.ref_off = (uint32_t *)at(8), b.keys = (uint32_t *)at(9), b.keys2 = (uint32_t *)at(10);
  b.vals = (uint32_t *)at(11), b.flags = (uint32_t *)at(12), b.incl = (uint32_t *)at(13), b.seg_start = (uint32_t *)at(14);
  b.nch = (uint32_t *)at(15), b.ch_base = (uint32_t *)at(16);
  b.nmulti = (unsigned long long *)at(17), b.multi_base = (unsigned long long *)at(18);
  b.scratch = at(19), b.scratch_bytes = scratch;
  b.ell = (int32_t *)at(20);
  c->d_partial = (float *)at(21);
  *out = c;
  return SCONE_OK;
}

extern "C" int scone_backward_ctx_bytes(scone_bwd_ctx *ctx, uint64_t *bytes) {
  if (!ctx || !bytes) return SCONE_EINVAL;
  *bytes = ctx->bytes;
  return SCONE_OK;
}

extern "C" void scone_backward_ctx_destroy(scone_bwd_ctx *ctx) {
  if (!ctx) return;
  scone_device_guard guard(ctx->device);
  if (ctx->slab) (void)hipFree(ctx->slab);
  delete ctx;
}

extern "C" int scone_backward_plan_dn(scone_handle *h, scone_bwd_ctx *ctx, const int32_t *d_tok, int32_t B, int32_t T,
                                      scone_stream_t stream) {
  const char *who = "scone_backward_plan_dn";
  SCONE_TRY(ctx_check(h, ctx, who));
  if (B < 0 || T < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative B or T");
  const long long ntok = (long long)B * T;
  if (ntok > 0 && !d_tok) return scone_refuse(h, SCONE_EINVAL, who, "null d_tok");
  bwd_plan_src src = {};
  src.kind = BWD_SRC_RECT, src.tok = d_tok, src.B = B, src.T = T;
  return plan_dn(h, ctx, who, src, ntok, (hipStream_t)stream);
}

extern "C" int scone_backward_plan_varlen_dn(scone_handle *h, scone_bwd_ctx *ctx, const int32_t *d_tok, const int32_t *d_cu_seqlens,
                                             int32_t n_seqs, int64_t total_tokens, scone_stream_t stream) {
  const char *who = "scone_backward_plan_varlen_dn";
  SCONE_TRY(ctx_check(h, ctx, who));
  if (n_seqs < 0 || total_tokens < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative n_seqs or total_tokens");
  if (total_tokens > 0x7FFFFFFFll) return scone_refuse(h, SCONE_EINVAL, who, "total_tokens above 2^31 - 1");
  if (h->cfg.stage_tokens && h->rows_host) return scone_refuse(h, SCONE_EINVAL, who, "not for stage_tokens > 0 (as scone_embed_varlen)");
  long long ntok = total_tokens;
  if (n_seqs == 0) ntok = 0;  // as scone_embed_varlen: a batch without sequences is empty
  if (ntok > 0 && (!d_tok || !d_cu_seqlens)) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  bwd_plan_src src = {};
  src.kind = BWD_SRC_PACKED, src.tok = d_tok, src.cu = d_cu_seqlens, src.n_seqs = n_seqs;
  return plan_dn(h, ctx, who, src, ntok, (hipStream_t)stream);
}

extern "C" int scone_backward_ctx_counts(scone_bwd_ctx *ctx, uint64_t *h_n_rows, uint64_t *h_n_refs, scone_stream_t stream) {
  if (!ctx) return SCONE_EINVAL;
  scone_handle *h = ctx->h;
  SCONE_ON_DEVICE(h);
  bwd_meta m = {};
  SCONE_HIP(h, hipMemcpyAsync(&m, ctx->b.meta, sizeof(bwd_meta), hipMemcpyDeviceToHost, (hipStream_t)stream));
  SCONE_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  // the bounds the buffers were sized by, asserted against what the build counted
  if (m.n_segs > ctx->cur.seg_cap || m.n_chunks > ctx->cur.chunk_cap || m.n_multi > ctx->cur.multi_cap ||
      m.n_slots > slot_bound(ctx->cur) || m.n_refs > ctx->cur.max_refs)
    return scone_refuse(h, SCONE_ESTATE, "scone_backward_ctx_counts", "inconsistent plan");
  if (h_n_rows) *h_n_rows = m.n_segs;
  if (h_n_refs) *h_n_refs = m.n_refs;
  return SCONE_OK;
}

extern "C" int scone_backward_rows_dn(scone_handle *h, scone_bwd_ctx *ctx, const void *d_grad_out, int32_t grad_dtype, int32_t reduce,
                                      int64_t *d_row_ids_out, float *d_grad_rows_out, uint64_t rows_cap, uint64_t *d_n_out,
                                      scone_stream_t stream) {
  const char *who = "scone_backward_rows_dn";
  SCONE_TRY(ctx_check(h, ctx, who));
  if (grad_dtype != SCONE_DT_F32 && grad_dtype != SCONE_DT_F16 && grad_dtype != SCONE_DT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who, "bad grad_dtype");
  if (reduce != SCONE_REDUCE_MEAN && reduce != SCONE_REDUCE_SUM) return scone_refuse(h, SCONE_EINVAL, who, "bad reduce");
  if (!d_n_out) return scone_refuse(h, SCONE_EINVAL, who, "null d_n_out");
  const bool empty = ctx->ntok == 0 || ctx->cur.max_refs == 0;
  if (!empty && (!d_grad_out || (rows_cap > 0 && (!d_row_ids_out || !d_grad_rows_out))))
    return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  if (empty) {
    hipLaunchKernelGGL(k_bwd_zero_n, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned long long *>(d_n_out));
    SCONE_HIP(h, hipGetLastError());
    return SCONE_OK;
  }
  bwd_dn_caps caps;
  caps.rows_cap = rows_cap, caps.chunk_cap = ctx->cur.chunk_cap, caps.multi_cap = ctx->cur.multi_cap;
  caps.slot_cap = slot_bound(ctx->cur);
  const unsigned long long id_bound = ctx->cur.seg_cap < rows_cap ? ctx->cur.seg_cap : rows_cap;
  hipLaunchKernelGGL(k_bwd_head_dn, dim3(dn_blocks(h, (id_bound + BWD_THREADS - 1) / BWD_THREADS)), dim3(BWD_THREADS), 0, s, ctx->b.meta,
                     caps, ctx->b.row_id, d_row_ids_out, reinterpret_cast<unsigned long long *>(d_n_out), h->d_status);
  SCONE_HIP(h, hipGetLastError());
  if (grad_dtype == SCONE_DT_F32)
    launch_chunks_dn<SCONE_DT_F32>(ctx, caps, d_grad_out, reduce, d_grad_rows_out, s);
  else if (grad_dtype == SCONE_DT_F16)
    launch_chunks_dn<SCONE_DT_F16>(ctx, caps, d_grad_out, reduce, d_grad_rows_out, s);
  else
    launch_chunks_dn<SCONE_DT_BF16>(ctx, caps, d_grad_out, reduce, d_grad_rows_out, s);
  SCONE_HIP(h, hipGetLastError());
  if (caps.slot_cap) {  // host-known: no batch of this size can have a row of several chunks otherwise
    const unsigned long long items = ctx->cur.multi_cap * (unsigned long long)((ctx->dim + 255) / 256);
    hipLaunchKernelGGL(k_bwd_combine_dn, dim3(dn_blocks(h, (items + 3) / 4)), dim3(BWD_THREADS), 0, s, ctx->b.meta, caps, ctx->b.multi,
                       ctx->d_partial, ctx->dim, d_grad_rows_out);
    SCONE_HIP(h, hipGetLastError());
  }
  return SCONE_OK;
}
