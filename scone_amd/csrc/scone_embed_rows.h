// The fused lookup over a batch's LIVE rows (scone_embed_rows, scone_embed_rows_varlen): the gather half of scone_embed with the
// rows taken from a caller's compact [n, d] array keyed by ascending row ids, not from the handle's table.
//
//   k_embed_rows   after k_match_ell / k_match_ell_varlen: every d % 8 == 0, rows fp32 / fp16 / bf16
//
// The match records hold TABLE ids; the rows live at the SLOT of an id in the caller's sorted list.  The new work is that
// id -> slot step, and it is done lane-parallel ACROSS tokens: a wave takes a group of consecutive tokens whose records fill
// its 64 lanes (8 tokens at record width 8, 4 at width 16) with one coalesced load, and every lane that holds an id (entry
// j < K_own of its token, id >= 0) runs the lower-bound search over d_row_ids[0, n_live) with vector loads: the ~log2(n_live)
// dependent L2 latencies are paid once per GROUP, by up to 64 lanes at once.  (One id at a time on wave-uniform scalar
// loads, as everything else that steers a token is fetched here, would pay them once per ID: about 19 per id and 100 per
// token on the headline batch.)  The slot, or the "missing" mark n_live, stays in the lane's register.
//
// The wave then walks the tokens of its group one at a time exactly as k_embed_wave_any does: the token's slots move to
// scalars (v_readlane), token / position / base rows are resolved by that kernel's rules, and a switch on K calls
// embed_units<FMT, OutT, K, false> (scone_embed_wave.h) as it stands -- the arithmetic is that function's, row_codec<FMT>
// and all.  The row store handed to it is built here: rows [0, n_live) are the caller's, row n_live is the handle's zero
// row (d * 4 zero bytes: as wide as any row of these three types).  A missing id reads that row, which adds +0.0; K stays
// the full hit count.  Every slot is in [0, n_live], so no address outside d_rows[0, n_live) and the zero row is formed,
// whatever the list holds.
#pragma once

#include "scone_embed_wave.h"

namespace scone_gather {

struct live_rows_view {
  const uint8_t *rows;             // [n, d] of the row type
  const int64_t *ids;              // [n] ascending, distinct
  unsigned long long n;            // rows (capacity when d_n is given)
  const unsigned long long *d_n;   // null, or the live count on the device
};

// Grid cap in workgroups per compute unit.  A workgroup is one wave per SIMD and the kernel's registers leave room for 4 to 7
// of them on a CU (fp32 and fp16 rows 4-5, bf16 rows 5-7), so 6 per CU is one residency round: the waves of a larger grid would
// only queue behind it, and every resident wave strides over an equal share of the groups.
#ifndef SCONE_ROWS_BLOCKS_PER_CU
#define SCONE_ROWS_BLOCKS_PER_CU 6
#endif

template <int FMT, typename OutT, int MAXN>
__global__ __launch_bounds__(256) void k_embed_rows(const live_rows_view live, const int32_t *__restrict__ ell,
                                                    const int32_t *__restrict__ tok, const int32_t *__restrict__ pos,
                                                    const OutT *wte, const OutT *__restrict__ wpe,
                                                    const uint8_t *__restrict__ zero_row, OutT *out,
                                                    uint32_t *__restrict__ status, const wave_params q, int d) {
  static_assert(FMT == SCONE_FMT_F32 || FMT == SCONE_FMT_F16 || FMT == SCONE_FMT_BF16, "live rows are plain fp32 / fp16 / bf16 rows");
  constexpr int NC = MAXN * (MAXN + 1) / 2;
  constexpr int W = MAXN <= 3 ? 8 : 16;
  constexpr int G = 64 / W;  // tokens per group
  const uint32_t lane = threadIdx.x & 63;
  const long long wave0 = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long nwaves = (long long)gridDim.x * 4;
  const long long groups = (q.BT + G - 1) / G;

  unsigned long long nl = live.n;  // one scalar load of the device count, clamped to the capacity
  if (live.d_n) {
    const unsigned long long dn = *live.d_n;
    nl = dn < nl ? dn : nl;
  }
  const uint32_t n_live = (uint32_t)nl;  // <= 2^31 - 1 (entry point)
  scone_row_store rows;
  rows.hot = const_cast<uint8_t *>(live.rows);
  rows.cold = const_cast<uint8_t *>(zero_row);  // local row n_live: what a missing id reads
  rows.n_hot = n_live;
  rows.row_bytes = (unsigned)d * (unsigned)(row_codec<FMT>::BPE4 / 4);

  const int j = (int)(lane & (W - 1));        // entry of the record this lane holds
  const int meta_lane = (int)(lane | (W - 2)) & ~1;  // the lane that holds K_own | K_full << 8 of the same token

  for (long long g = wave0; g < groups; g += nwaves) {
    const long long p0 = g * G;
    // ---- the group's records, one coalesced load; id -> slot, every lane its own id --------------------------------
    const long long pl = p0 + (long long)(lane / W);
    const bool have = pl < q.BT;
    const int32_t v = have ? ell[pl * W + j] : 0;
    const int kown_l = __shfl(v, meta_lane) & 0xFF;
    const bool is_id = have && j < kown_l && j < NC;
    uint32_t lo = 0, len = is_id && v >= 0 ? n_live : 0u;
    while (len > 0) {  // lower bound of v in ids[0, n_live): every index read is below n_live
      const uint32_t half = len >> 1;
      if (live.ids[lo + half] < (int64_t)v)
        lo += half + 1, len -= half + 1;
      else
        len = half;
    }
    bool found = false;
    if (is_id && v >= 0 && lo < n_live) found = live.ids[lo] == (int64_t)v;
    const int32_t slot = found ? (int32_t)lo : (int32_t)n_live;
    if (__ballot(is_id && !found) != 0ull && lane == 0) atomicOr(status, SCONE_ST_BAD_ID);

    // ---- the tokens of the group, one at a time: as k_embed_wave_any ------------------------------------------------
    for (int tl = 0; tl < G; ++tl) {
      const long long p = p0 + tl;
      if (p >= q.BT) break;
      const int meta = __builtin_amdgcn_readlane(v, tl * W + W - 2);
      const int kown = meta & 0xFF, kfull = meta >> 8;
      int32_t rec[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) rec[k] = __builtin_amdgcn_readlane(slot, tl * W + k);
      const uint8_t *wte_row = zero_row, *wpe_row = zero_row;
      const int32_t tokv = (wte && q.vocab >= 0) ? tok[p] : 0;  // dense base (q.vocab < 0): row p of `wte`, no token id needed
      const int32_t posv = wpe ? (pos ? pos[p] : (int32_t)(p % q.T)) : 0;
      const bool tok_ok = wte && (q.vocab < 0 || (tokv >= 0 && (long long)tokv < q.vocab));
      const bool pos_ok = wpe && posv >= 0 && (long long)posv < q.n_pos;
      if ((wte && !tok_ok) || (wpe && !pos_ok)) {
        if (lane == 0) atomicOr(status, SCONE_ST_BAD_TOKEN);
      }
      if (tok_ok && !(q.mode == SCONE_MODE_LONGEST_SUFFIX && kfull > 0))
        wte_row = reinterpret_cast<const uint8_t *>(wte + (q.vocab < 0 ? p : (long long)tokv) * d);
      if (pos_ok) wpe_row = reinterpret_cast<const uint8_t *>(wpe + (long long)posv * d);
      uint8_t *out_row = reinterpret_cast<uint8_t *>(out + p * d);
#define SCONE_CASE(K)                                                                                                     \
  case K:                                                                                                                 \
    if constexpr (K <= NC)                                                                                                \
      embed_units<FMT, OutT, K, false>(rows, nullptr, rec, 0ll, d, kfull, q.reduce, wte_row, wpe_row, out_row, lane);     \
    break;
      switch (kown) {
        SCONE_CASE(0) SCONE_CASE(1) SCONE_CASE(2) SCONE_CASE(3) SCONE_CASE(4) SCONE_CASE(5) SCONE_CASE(6)
        SCONE_CASE(7) SCONE_CASE(8) SCONE_CASE(9) SCONE_CASE(10)
        default: break;
      }
#undef SCONE_CASE
    }
  }
}

template <int FMT, typename OutT>
int launch_rows_out(scone_handle *h, const live_rows_view &live, const embed_args &a, hipStream_t s) {
  wave_params q = {};
  q.BT = a.BT, q.T = a.T, q.max_n = a.max_n;
  q.vocab = a.vocab, q.n_pos = a.n_pos, q.reduce = a.reduce, q.mode = a.mode;
  const void *wte = a.wte;
  if (q.vocab < 0) q.vocab = 0;            // (a caller's negative vocab keeps meaning "no token is in range")
  if (a.base) wte = a.base, q.vocab = -1;  // the dense base travels in the kernel's wte parameter, as in launch_wave_any
  const int G = 64 / SCONE_ELL_W(a.max_n);
  const unsigned long long groups = ((unsigned long long)a.BT + G - 1) / G;
  unsigned long long blocks = (groups + 3) / 4;
  const unsigned long long cap = (unsigned long long)SCONE_ROWS_BLOCKS_PER_CU * scone_lookup_cus(h);
  if (blocks > cap) blocks = cap;  // the waves stride over the groups
  if (!scone_grid_fits(blocks, 256)) return scone_fail(h, SCONE_EINVAL, "scone_embed_rows: too many tokens for one launch");
  if (a.max_n <= 3)
    hipLaunchKernelGGL((k_embed_rows<FMT, OutT, 3>), dim3((unsigned)blocks), dim3(256), 0, s, live, a.ell, a.tok, a.pos,
                       (const OutT *)wte, (const OutT *)a.wpe, (const uint8_t *)a.zero_row, (OutT *)a.out, a.status, q, a.tv.d);
  else
    hipLaunchKernelGGL((k_embed_rows<FMT, OutT, 4>), dim3((unsigned)blocks), dim3(256), 0, s, live, a.ell, a.tok, a.pos,
                       (const OutT *)wte, (const OutT *)a.wpe, (const uint8_t *)a.zero_row, (OutT *)a.out, a.status, q, a.tv.d);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

// With a CU reserve (scone_set_cu_reserve) the launch goes to the handle's masked stream, as try_launch_wave's does.
template <int FMT>
int launch_rows_fmt(scone_handle *h, const live_rows_view &live, const embed_args &a, int out_dtype, hipStream_t s) {
  hipStream_t ls = s;
  int rc = scone_lookup_enter(h, s, &ls);
  if (rc) return rc;
  switch (out_dtype) {
    case SCONE_DT_F32: rc = launch_rows_out<FMT, float>(h, live, a, ls); break;
    case SCONE_DT_F16: rc = launch_rows_out<FMT, __half>(h, live, a, ls); break;
    case SCONE_DT_BF16: rc = launch_rows_out<FMT, __hip_bfloat16>(h, live, a, ls); break;
    default: rc = scone_fail(h, SCONE_EINVAL, "scone_embed_rows: bad out_dtype"); break;
  }
  const int rc2 = scone_lookup_leave(h, s, ls);
  return rc ? rc : rc2;
}

// one translation unit per row type (scone_rows_<fmt>.hip), as the scone_gather_<fmt>.hip units
int launch_rows_f32(scone_handle *h, const live_rows_view &live, const embed_args &a, int out_dtype, hipStream_t s);
int launch_rows_f16(scone_handle *h, const live_rows_view &live, const embed_args &a, int out_dtype, hipStream_t s);
int launch_rows_bf16(scone_handle *h, const live_rows_view &live, const embed_args &a, int out_dtype, hipStream_t s);

}  // namespace scone_gather
