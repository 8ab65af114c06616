// What the backward's kernels share -- k_bwd_chunks / k_bwd_combine (scone_backward.hip) and the fused backward + lean step
// (scone_backward_apply.hip): the plan a batch is cut into, and how one wave walks the references of a chunk.
//
// A plan is the sorted reference stream of a batch: the references of a row are consecutive, in (p, k) order, cut into chunks of
// SCONE_BWD_CHUNK; a row with several chunks has a partial slot per chunk and one bwd_multi entry.  The order in which a chunk's
// references are added (bwd_walk) and the order in which a row's partials are added (chunk order) are the gradient's contract.
#pragma once

#include "scone_common.h"

#ifndef SCONE_BWD_CHUNK
#define SCONE_BWD_CHUNK 128  // part of the contract (scone_backward_chunk); chosen by measurement, DESIGN.md 4.4b
#endif
static_assert(SCONE_BWD_CHUNK >= 64 && SCONE_BWD_CHUNK <= 512 && (SCONE_BWD_CHUNK & (SCONE_BWD_CHUNK - 1)) == 0,
              "SCONE_BWD_CHUNK: a power of two in [64, 512]");

// device-side totals of a plan, copied to the host by the plan's one synchronisation
struct bwd_meta {
  uint32_t n_refs;    // references (owned rows only)
  uint32_t n_segs;    // U: distinct rows with a reference
  uint32_t n_chunks;  // work items of the chunk pass
  uint32_t n_multi;   // rows with more than one chunk
  uint32_t n_slots;   // partial slots = chunks of those rows
  uint32_t pad[3];
};

// one work item of the chunk pass: references [begin, begin + count) of the sorted stream go to row `dest` of grad_rows
// (partial == 0) or to partial slot `dest` (partial == 1)
struct __attribute__((aligned(16))) bwd_chunk {
  uint32_t begin, count, dest, partial;
};
// one row with several chunks: grad_rows[seg] = partial[slot0] + ... + partial[slot0 + n - 1], in that order
struct __attribute__((aligned(16))) bwd_multi {
  uint32_t seg, slot0, n, pad;
};

struct scone_bwd_plan {
  scone_handle *h = nullptr;
  int device = 0;
  int dim = 0;
  long long ntok = 0;
  bool index = false;  // an index plan (scone_backward_plan_index): its ids are those of the caller's id space, not table rows
  bwd_meta m = {};
  // kept for the life of the plan
  int32_t *d_kfull = nullptr;     // [ntok] K_p, the full hit count
  float *d_w = nullptr;           // [ntok] 1.0f / (float)K_p (1.0f where K_p == 0: never read)
  uint32_t *d_ref_p = nullptr;    // [max_refs] position of every reference, sorted stably by row
  uint32_t *d_row_id = nullptr;   // [seg_cap + 1] row of segment u
  bwd_chunk *d_chunks = nullptr;  // [chunk_cap]
  bwd_multi *d_multi = nullptr;   // [multi_cap]
  float *d_partial = nullptr;     // [n_slots, dim]
  bwd_meta *d_meta = nullptr;
};

// ---- one plan build, whoever owns its buffers (scone_backward.hip): scone_backward_plan* allocate them per call and read the
// totals back; a scone_bwd_ctx (scone_backward_dn.hip) holds them at its worst-case sizes and leaves the totals on the device.
enum { BWD_SRC_RECT = 0, BWD_SRC_PACKED = 1, BWD_SRC_CSR = 2, BWD_SRC_INDEX = 3 };

struct bwd_plan_src {
  int kind;
  const int32_t *tok;      // the tokens; the ids idx [ntok] of an index plan
  int32_t B, T;            // rectangle
  const int32_t *cu;       // packed
  int32_t n_seqs;
  const int32_t *offsets;  // CSR
  const int32_t *ids;
  long long csr_total;
  const int32_t *skip;     // index plan: position p has no reference where skip[p] != 0 (may be null)
  long long n_ids;         // index plan: the size of its id space
};

// what a plan of at most max_refs references can need: all host-known
struct bwd_plan_sizes {
  unsigned long long max_refs;   // items sorted and scanned, whatever the batch holds
  unsigned long long seg_cap;    // most distinct rows: min(max_refs, owned rows)
  unsigned long long chunk_cap;  // most chunks
  unsigned long long multi_cap;  // most rows with several chunks
  int end_bit;                   // the sort's key bits: those of the pad key
  uint32_t pad_key;              // the size of the plan's id space (n_rows of the table; n_ids of an index plan): behind every id
};

struct bwd_plan_bufs {
  // the plan
  int32_t *kfull;     // [ntok]
  float *w;           // [ntok]
  uint32_t *ref_p;    // [max_refs]
  uint32_t *row_id;   // [seg_cap + 1]
  bwd_chunk *chunks;  // [chunk_cap]
  bwd_multi *multi;   // [multi_cap]
  bwd_meta *meta;     // zeroed by the caller
  // scratch of the build
  uint32_t *kown, *ref_off;            // [ntok + 1]
  uint32_t *keys, *keys2, *vals;       // [max_refs]
  uint32_t *flags, *incl;              // [max_refs]
  uint32_t *seg_start;                 // [seg_cap + 2]
  uint32_t *nch, *ch_base;             // [seg_cap + 1]
  unsigned long long *nmulti, *multi_base;  // [seg_cap + 1]
  void *scratch;  // rocPRIM's, scone_bwd_plan_scratch bytes
  size_t scratch_bytes;
  int32_t *ell;  // the match records [ntok, SCONE_ELL_W]; null: those of the workspace of the call's stream (token forms)
};

bwd_plan_sizes scone_bwd_plan_sizes(const scone_handle *h, unsigned long long max_refs);
// the same for any id space: ids in [0, n_ids), of which `owned` can have a reference
bwd_plan_sizes scone_bwd_plan_sizes_ids(unsigned long long max_refs, unsigned long long n_ids, unsigned long long owned);
// the bytes the sort and the four scans of a build need at most (host only: no device work)
int scone_bwd_plan_scratch(scone_handle *h, long long ntok, const bwd_plan_sizes &z, hipStream_t s, size_t *need);
// enqueues the whole build on s: no allocation but the workspace's (b.ell == null), no synchronisation.  ntok > 0, max_refs > 0.
// The CSR form's kown / kfull / w are counted by the caller (it needs the owned count first).
int scone_bwd_plan_enqueue(scone_handle *h, const bwd_plan_src &src, long long ntok, const bwd_plan_sizes &z, const bwd_plan_bufs &b,
                           hipStream_t s);
// a new plan of `ntok` positions built from `src` (which allocates, and synchronises s once) and handed out, or freed on failure
int scone_bwd_plan_make(scone_handle *h, const bwd_plan_src &src, long long ntok, unsigned long long max_refs, scone_bwd_plan **out,
                        uint64_t *h_n_rows, uint64_t *h_n_refs, hipStream_t s);
// step (1) of a build from BWD_SRC_INDEX (scone_backward_index.hip): K_p / w, the reference offsets, the (id, p) pairs
int scone_bwd_index_pairs(scone_handle *h, const bwd_plan_src &src, long long ntok, const bwd_plan_bufs &b, hipStream_t s);
// rocPRIM's exclusive scan of n uint32 with the build's scratch
int scone_bwd_scan_u32(scone_handle *h, void *scratch, size_t scratch_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s);
// references a position can have: max_n (max_n + 1) / 2, or 1 in longest_suffix mode
unsigned long long scone_bwd_cand_per_token(const scone_handle *h);
// the largest sort that stays with rocPRIM's merge sort (no kernel with a private segment)
unsigned long long scone_bwd_sort_merge_limit();
// plan_common_checks' refusals for entry point `who`
int scone_bwd_plan_checks(scone_handle *h, const char *who);

// 16 bytes of grad_out as fp32: 4 elements (fp32) or 8 (fp16 / bf16); every conversion is exact
template <int DT>
struct bwd_piece {
  static constexpr int E = DT == SCONE_DT_F32 ? 4 : 8;
  static __device__ __forceinline__ void to_f32(const uint4 &r, float *f) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    if constexpr (DT == SCONE_DT_F32) {
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(w[i]);
    } else if constexpr (DT == SCONE_DT_F16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[2 * i] = __half2float(__ushort_as_half((unsigned short)(w[i] & 0xFFFFu)));
        f[2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(w[i] >> 16)));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
      }
    }
  }
};

// RR references of a chunk: their positions and weights are wave-uniform scalars, their RR * NT loads are independent, and only
// the adds form a chain -- in reference order, which is the contract.
template <int DT, int NT, bool MEAN, int RR>
__device__ __forceinline__ void bwd_walk(const uint32_t *__restrict__ ref_p, const float *__restrict__ w, const uint8_t *gl,
                                         size_t row_bytes, const bool (&on)[NT], float (&acc)[NT][bwd_piece<DT>::E]) {
  constexpr int E = bwd_piece<DT>::E;
  uint4 raw[RR][NT];
  float wr[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    const uint32_t p = ref_p[r];
    wr[r] = MEAN ? w[p] : 1.0f;
    const uint8_t *row = gl + (size_t)p * row_bytes;
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
        for (int e = 0; e < E; ++e) {
          const float cc = MEAN ? f[e] * wr[r] : f[e];
          acc[t][e] = acc[t][e] + cc;
        }
      }
    }
  }
}

// All the references of one chunk for one column tile of NT * 64 pieces: 16 / NT at a time (16 independent 16-byte loads per lane
// in flight whatever the tile width: a chunk of a hot row is one dependent chain of memory latencies otherwise), what is left
// four at a time, then one by one.  `acc` starts at +0.0f.
template <int DT, int NT, bool MEAN>
__device__ __forceinline__ void bwd_walk_chunk(const uint32_t *__restrict__ rp, uint32_t count, const float *__restrict__ w,
                                               const uint8_t *gl, size_t row_bytes, const bool (&on)[NT],
                                               float (&acc)[NT][bwd_piece<DT>::E]) {
  constexpr int R = 16 / NT;
  uint32_t i = 0;
  if constexpr (R > 4)
    for (; i + R <= count; i += R) bwd_walk<DT, NT, MEAN, R>(rp + i, w, gl, row_bytes, on, acc);
  for (; i + 4 <= count; i += 4) bwd_walk<DT, NT, MEAN, 4>(rp + i, w, gl, row_bytes, on, acc);
  for (; i < count; ++i) bwd_walk<DT, NT, MEAN, 1>(rp + i, w, gl, row_bytes, on, acc);
}
