// scone_embed_select: the fused lookup at CHOSEN positions only (a decoding step's last token of every sequence, the last k
// tokens of a speculative-verify step, the new chunk of a chunked prefill), matched against context that is already on the
// device.  One launch, one wave per selected position, no workspace:
//
//   wave j -> p = sel[j] (wave-uniform) -> range check -> the sequence of p (p % T, or the scalar upper-bound search over cu
//   of k_embed_fused<VARLEN>, with the same clamps) -> lanes < NC probe the candidate windows of p -> ballot -> kfull, kown
//   and the id list as scalars -> the K-way body, switch (kown)
//
// The bodies are the library's own and are called, not copied: embed_token<> at the specialised dims (768 / 1024 / 1280 where
// wave_geom<>::OK), embed_units<> -- the unit-walking body of k_embed_wave_any -- for every other d % 8 == 0.  The second road
// is the one-launch match + gather that d = 2048 / 4096 / ... and INT4 / MXFP4 at 768 / 1280 did not have.
// Everything per OUTPUT is indexed by j: the dense base row, the caller's position id and the output row.  Rectangular or
// packed is a wave-uniform run-time branch on cu != nullptr (the kernel is launch-bound; a template parameter would double
// the instantiations).
#pragma once

#include "scone_embed_wave.h"

namespace scone_gather {

struct select_args {
  table_view tv;
  const int32_t *tok;  // [total]
  long long total;
  int T;               // rectangle: row length (cu == null)
  const int32_t *cu;   // packed: [n_seqs + 1], or null
  int n_seqs;
  const int32_t *sel;  // [n_sel] positions in [0, total)
  long long n_sel;
  const void *wte;     // [vocab, d], row tok[p] -- or
  long long vocab;
  const void *base;    // dense [n_sel, d], row j
  const void *wpe;
  long long n_pos;
  const int32_t *pos;  // [n_sel] or null (the place of p inside its sequence)
  int reduce;
  int mode;
  int max_n;
  const void *zero_row;
  void *out;           // [n_sel, d]
  uint32_t *status;
};

// D > 0: the specialised body (wave_geom<FMT, D>::OK); D == 0: any d % 8 == 0, passed as `d`.
// q.BT = total tokens, q.T = the rectangle's row length, q.vocab < 0: `wte` is the dense base [n_sel, d].
template <int FMT, typename OutT, int D, int MAXN>
__global__ __launch_bounds__(256) void k_embed_select(const scone_row_store rows, const void *__restrict__ scales_v,
                                                      const scone_index_view ix, const int32_t *__restrict__ tok,
                                                      const int32_t *__restrict__ sel, const int32_t *__restrict__ pos,
                                                      const OutT *wte, const OutT *__restrict__ wpe,
                                                      const uint8_t *__restrict__ zero_row, OutT *out,
                                                      uint32_t *__restrict__ status, const wave_params q, long long n_sel,
                                                      const int32_t *__restrict__ cu, int n_seqs, int d) {
  constexpr int NC = MAXN * (MAXN + 1) / 2;
  const uint32_t lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (j >= n_sel) return;
  const int32_t pv = __builtin_amdgcn_readfirstlane(sel[j]);
  if (pv < 0 || (long long)pv >= q.BT) {  // nothing is read for it, row j is not written
    if (lane == 0) atomicOr(status, SCONE_ST_BAD_TOKEN);
    return;
  }
  const long long p = pv;
  int i, T;
  if (cu) {
    int lo = 1, hi = n_seqs;  // smallest s in [1, n_seqs] with cu[s] > p
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cu[mid] > (int)p) hi = mid; else lo = mid + 1;
    }
    // i in [0, p] and the room behind p in [0, total - p]: no token outside tok[0, total) is read whatever cu holds
    long long ii = p - (long long)cu[lo - 1], rr = (long long)cu[lo] - p;
    ii = ii < 0 ? 0 : (ii > p ? p : ii);
    rr = rr < 0 ? 0 : (rr > q.BT - p ? q.BT - p : rr);
    i = (int)ii, T = (int)(ii + rr);
  } else {
    i = (int)(p % q.T), T = q.T;
  }

  // ---- match: lane c probes candidate window c of token p (as k_embed_fused) ---------------------------
  int32_t my_id = -1;
  if ((int)lane < NC) {
    int n, s;
    cand_ns((int)lane, n, s);
    const bool wanted = q.mode == SCONE_MODE_COVER || (s == n - 1 && n >= 2);
    if (wanted && n <= q.max_n && i - s >= 0 && i - s + n <= T) {
      uint32_t k[SCONE_MAX_N] = {0u, 0u, 0u, 0u};
      bool ok = true;
#pragma unroll
      for (int t = 0; t < MAXN; ++t) {
        if (t < n) {
          const int32_t v = tok[p - s + t];
          ok = ok && v >= 0;
          k[t] = (uint32_t)v;
        }
      }
      if (ok) my_id = scone_lookup_key(ix, k, n);
    }
  }
  unsigned long long hit = __ballot(my_id >= 0);
  if (q.mode == SCONE_MODE_LONGEST_SUFFIX && hit) {
    hit = 1ull << (63 - __builtin_clzll(hit));  // Algorithm 2: the longest f-gram ending here is the highest hit lane
    if (!((hit >> lane) & 1ull)) my_id = -1;
  }
  unsigned long long own = __ballot(my_id >= 0 && (long long)my_id >= q.row_begin && (long long)my_id < q.row_end);
  const int kfull = __popcll(hit), kown = __popcll(own);
  int32_t rec[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int l = own ? __builtin_ctzll(own) : 0;
    rec[k] = __builtin_amdgcn_readlane(my_id, l);
    own &= own - 1;
  }

  // ---- gather + reduce + combine: base row, position id and output row are those of OUTPUT j -----------
  const int dd = D > 0 ? D : d;
  const int32_t tokv = (wte && q.vocab >= 0) ? tok[p] : 0;
  const int32_t posv = wpe ? (pos ? pos[j] : i) : 0;
  const bool tok_ok = wte && (q.vocab < 0 || (tokv >= 0 && (long long)tokv < q.vocab));
  const bool pos_ok = wpe && posv >= 0 && (long long)posv < q.n_pos;
  if ((wte && !tok_ok) || (wpe && !pos_ok)) {
    if (lane == 0) atomicOr(status, SCONE_ST_BAD_TOKEN);
  }
  // paper mode: a matched f-gram REPLACES the base row (Algorithm 2)
  const bool use_wte = tok_ok && !(q.mode == SCONE_MODE_LONGEST_SUFFIX && kfull > 0);
  const uint8_t *wte_row = use_wte ? reinterpret_cast<const uint8_t *>(wte + (q.vocab < 0 ? j : (long long)tokv) * dd) : zero_row;
  const uint8_t *wpe_row = pos_ok ? reinterpret_cast<const uint8_t *>(wpe + (long long)posv * dd) : zero_row;
  uint8_t *out_row = reinterpret_cast<uint8_t *>(out + j * dd);
  if constexpr (D > 0) {
    constexpr int NWO = wave_geom<FMT, (D > 0 ? D : 1024)>::EPL * (int)sizeof(OutT) / 4;
    uint32_t wpe_words[NWO];
#pragma unroll
    for (int w = 0; w < NWO; ++w) wpe_words[w] = 0u;
#define SCONE_CASE(K)                                                                                            \
  case K:                                                                                                        \
    if constexpr (K <= NC)                                                                                       \
      embed_token<FMT, OutT, D, K, false, false>(rows, scales_v, rec, q.row_begin, kfull, q.reduce, wte_row, wpe_row, \
                                                 wpe_words, out_row, lane);                                      \
    break;
    switch (kown) {
      SCONE_CASE(0) SCONE_CASE(1) SCONE_CASE(2) SCONE_CASE(3) SCONE_CASE(4) SCONE_CASE(5) SCONE_CASE(6)
      SCONE_CASE(7) SCONE_CASE(8) SCONE_CASE(9) SCONE_CASE(10)
      default: break;
    }
#undef SCONE_CASE
  } else {
#define SCONE_CASE(K)                                                                                            \
  case K:                                                                                                        \
    if constexpr (K <= NC)                                                                                       \
      embed_units<FMT, OutT, K, false>(rows, scales_v, rec, q.row_begin, d, kfull, q.reduce, wte_row, wpe_row, out_row, \
                                       lane);                                                                    \
    break;
    switch (kown) {
      SCONE_CASE(0) SCONE_CASE(1) SCONE_CASE(2) SCONE_CASE(3) SCONE_CASE(4) SCONE_CASE(5) SCONE_CASE(6)
      SCONE_CASE(7) SCONE_CASE(8) SCONE_CASE(9) SCONE_CASE(10)
      default: break;
    }
#undef SCONE_CASE
  }
}

template <int FMT, typename OutT>
int launch_select_out(scone_handle *h, const select_args &a, hipStream_t s) {
  wave_params q = {};
  q.BT = a.total, q.T = a.T, q.max_n = a.max_n;
  q.row_begin = a.tv.row_begin, q.row_end = a.tv.row_end;
  q.vocab = a.vocab, q.n_pos = a.n_pos, q.reduce = a.reduce, q.mode = a.mode;
  const void *wte = a.wte;
  if (q.vocab < 0) q.vocab = 0;            // (a caller's negative vocab keeps meaning "no token is in range")
  if (a.base) wte = a.base, q.vocab = -1;  // the dense base [n_sel, d] travels in the kernel's wte parameter
  scone_index_view ix;
  scone_index_view_of(h, &ix);
  const unsigned long long blocks = ((unsigned long long)a.n_sel + 3) / 4;
  if (!scone_grid_fits(blocks, 256)) return scone_fail(h, SCONE_EINVAL, "scone_embed_select: too many selected positions for one launch");
#define SCONE_SELECT(DD, NN)                                                                                      \
  hipLaunchKernelGGL((k_embed_select<FMT, OutT, DD, NN>), dim3((unsigned)blocks), dim3(256), 0, s, a.tv.st,       \
                     (const void *)a.tv.scales, ix, a.tok, a.sel, a.pos, (const OutT *)wte, (const OutT *)a.wpe,  \
                     (const uint8_t *)a.zero_row, (OutT *)a.out, a.status, q, a.n_sel, a.cu, a.n_seqs, a.tv.d)
#define SCONE_SELECT_N(DD)                                            \
  do {                                                                \
    if (a.max_n <= 3) SCONE_SELECT(DD, 3); else SCONE_SELECT(DD, 4);  \
    SCONE_HIP(h, hipGetLastError());                                  \
    return SCONE_OK;                                                  \
  } while (0)
  if constexpr (wave_geom<FMT, 768>::OK) {
    if (a.tv.d == 768) SCONE_SELECT_N(768);
  }
  if constexpr (wave_geom<FMT, 1024>::OK) {
    if (a.tv.d == 1024) SCONE_SELECT_N(1024);
  }
  if constexpr (wave_geom<FMT, 1280>::OK) {
    if (a.tv.d == 1280) SCONE_SELECT_N(1280);
  }
  SCONE_SELECT_N(0);  // any other d % 8 == 0 (and INT4 / MXFP4 at 768 / 1280): the unit-walking body
#undef SCONE_SELECT_N
#undef SCONE_SELECT
}

template <int FMT>
int launch_select_fmt(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s) {
  switch (out_dtype) {
    case SCONE_DT_F32: return launch_select_out<FMT, float>(h, a, s);
    case SCONE_DT_F16: return launch_select_out<FMT, __half>(h, a, s);
    case SCONE_DT_BF16: return launch_select_out<FMT, __hip_bfloat16>(h, a, s);
    default: return scone_fail(h, SCONE_EINVAL, "scone_embed_select: bad out_dtype");
  }
}

// one translation unit per table format (scone_select_<fmt>.hip), as the scone_gather_<fmt>.hip units
int launch_select_f32(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s);
int launch_select_f16(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s);
int launch_select_i8(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s);
int launch_select_i4(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s);
int launch_select_bf16(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s);
int launch_select_mxfp4(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s);

}  // namespace scone_gather
