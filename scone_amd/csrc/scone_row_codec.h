// How a table format stores a row, as a READER sees it: the one definition per format that every lookup body calls --
// embed_token, embed_units, embed_token_long (scone_embed_wave.h) and the lane-group kernel k_embed (scone_gather_impl.h).
// A row is a run of 32-bit payload words; row_codec<FMT> says how many elements a word holds, where the scale of a run of
// elements lives and how it becomes an fp32 operand, how a word is added to the accumulators, and which division the mean
// takes.  Nothing else in those two headers names a format, except static_asserts and the measured tuning tables
// (wave_hiocc, wave_occupancy).  The write side (scone_table.hip, scone_opt_rows.h) has its own, per-element, definitions.
#pragma once
#include "scone_common.h"
#include "scone_mean_div.h"

namespace scone_gather {

// acc[e] = fma(sc, q_e, acc[e]) for the 8 offset-binary nibbles of w, in 2.5 instead of 4 VALU ops per element:
// w ^ 0x88888888 turns every nibble into two's complement; with a nibble in the HIGH half of a byte the
// sign-extending byte convert (v_cvt_f32_i32 sext(BYTE_k), one SDWA instruction) yields 16 q, and
// fma(sc / 16, 16 q, acc) equals fma(sc, q, acc) bit for bit (sc / 16 and the product are exact).
__device__ __forceinline__ void i4_accumulate(uint32_t w, float sc, float *acc) {
  const uint32_t t = w ^ 0x88888888u;
  const uint32_t ev = (t << 4) & 0xF0F0F0F0u;  // elements 0, 2, 4, 6 in bytes 0..3
  const uint32_t od = t & 0xF0F0F0F0u;         // elements 1, 3, 5, 7
  const float sc16 = sc * 0.0625f;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int qe = (int)(ev << (24 - 8 * b)) >> 24;
    const int qo = (int)(od << (24 - 8 * b)) >> 24;
    acc[2 * b] = fmaf(sc16, (float)qe, acc[2 * b]);
    acc[2 * b + 1] = fmaf(sc16, (float)qo, acc[2 * b + 1]);
  }
}

// MXFP4: acc[0..8) += the 8 E2M1 elements of payload dword w (element 2k = low nibble of byte k) times the block scale, with
// gfx950's packed convert: v_cvt_scalef32_pk_f32_fp4 turns the two nibbles of byte `byte_sel` into two fp32 and applies the
// scale operand's exponent -- two elements per VALU instruction, then one add each.  `sc` is mx_scale_operand(X): the E8M0
// byte in an fp32 exponent field.  The product is exact wherever it is finite, so acc += value is the oracle's sum of the
// dequantised table; the exhaustive (code, X) test of tests/test_gpu_mxfp4_table.py holds the convert to the definition.
// `tie`: p0, p1 are two accumulators of the word summed just before this one.  A convert has no operand but the loaded word and
// its scale, so left to itself the scheduler decodes every row as it arrives -- 8 fp32 per payload dword in flight, and the
// K >= 4 paths of k_embed_wave spill (fp32 output, d = 1024, max_n = 4: 164 B of scratch).  The empty asm emits nothing; it
// makes every convert wait for the two sums written just before it (the previous byte's; for the first byte, with `tie`, the
// previous word's), as bf16_accumulate_column does for bf16: rows stay packed until they are summed.
__device__ __forceinline__ float mx_scale_operand(uint32_t x) { return __uint_as_float(x << 23); }
__device__ __forceinline__ void mx_accumulate(uint32_t w, float sc, float *acc, bool tie = false, float p0 = 0.f, float p1 = 0.f) {
  typedef float mx_f2 __attribute__((ext_vector_type(2)));
  if (tie) asm("" : "+v"(w) : "v"(p0), "v"(p1));
  const mx_f2 v0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0);
  acc[0] += v0.x, acc[1] += v0.y;
  asm("" : "+v"(w) : "v"(acc[0]), "v"(acc[1]));
  const mx_f2 v1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1);
  acc[2] += v1.x, acc[3] += v1.y;
  asm("" : "+v"(w) : "v"(acc[2]), "v"(acc[3]));
  const mx_f2 v2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 2);
  acc[4] += v2.x, acc[5] += v2.y;
  asm("" : "+v"(w) : "v"(acc[4]), "v"(acc[5]));
  const mx_f2 v3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 3);
  acc[6] += v3.x, acc[7] += v3.y;
}

// bf16 rows (a bf16 is the upper half of its fp32: the value is bits << 16): acc[a], acc[a + 1] += the two elements of row
// word w[k], k = 0 .. K - 1 in list order.  The shift and the mask have no operand but the loaded word, so left to itself the
// scheduler unpacks every row as it arrives and the live registers of a token double (fp16 rows stay packed until their
// convert + add: at d = 768, max_n = 3 that was 72 VGPRs with 44 B of scratch against the fp16 twin's 67 without).  The empty
// asm statements emit nothing; they make the unpack of row k wait for the sum of rows 0 .. k - 1, and the first row of a
// column for the column before it (`prev`), which is the order the compiler picks for fp16 by itself: one accumulator pair
// in flight, the rows packed.  The arithmetic is the plain list-order sum.
template <int K, int STRIDE>
__device__ __forceinline__ void bf16_accumulate_column(const uint32_t *w, float &lo, float &hi, const float *prev) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    uint32_t ww = w[k * STRIDE];
    if (k > 0)
      asm("" : "+v"(ww) : "v"(lo), "v"(hi));
    else if (prev)
      asm("" : "+v"(ww) : "v"(prev[0]), "v"(prev[1]));
    lo += __uint_as_float(ww << 16);
    hi += __uint_as_float(ww & 0xFFFF0000u);
  }
}

// One of the two scales that travel in one packed word (row_pair_bits, seg_pair_bits below): the low BITS, or with `second`
// the BITS above them.  A macro, not a member of row_codec: the expression has to be compiled inside the body that holds the
// word.  As a function it is simplified on its own before it is inlined, and the scale converts of k_embed_wave,
// k_embed_fused and k_embed_csr_wave come out in another order (same instructions, up to 8 more VGPRs at INT8 d = 768).
#define SCONE_SCALE_OF_PAIR(word, second, BITS) ((second) ? ((word) >> (BITS)) : ((word) & ((1u << (BITS)) - 1u)))

template <int FMT> struct row_codec {
  static_assert(FMT >= SCONE_FMT_F32 && FMT <= SCONE_FMT_MXFP4, "unknown table format");
  // ---- geometry -------------------------------------------------------------------------------------------------------
  static constexpr int BPE4 = FMT == SCONE_FMT_F32 ? 16 : (FMT == SCONE_FMT_F16 || FMT == SCONE_FMT_BF16) ? 8 : FMT == SCONE_FMT_I8 ? 4 : 2;  // bytes per 4 elements (last arm: INT4 and MXFP4)
  static constexpr int EPW = 16 / BPE4;  // elements per 32-bit row word
  static constexpr int RW8 = BPE4 / 2;   // row words per 8 elements (the unit of embed_units)
  static constexpr int VEC = 4 * EPW;    // elements per 16-byte vector (the lane-group kernel's load; MXFP4: one block)
  static constexpr bool PLAIN_F32 = FMT == SCONE_FMT_F32;  // a row is its fp32 values: the layout of the shards' partial sums
  // ---- scales ---------------------------------------------------------------------------------------------------------
  // SCALE_SPAN consecutive elements share one scale (0: the whole row does).  INT8: one fp16 per row, [rows]; INT4: one fp16
  // per 128 elements, [rows, d / 128]; MXFP4: one E8M0 byte per 32, [rows, d / 32] -- the last two in the physical order of
  // scone_i4_scale_slot / scone_mx_scale_slot (scone_common.h).
  static constexpr bool SCALED = FMT == SCONE_FMT_I8 || FMT == SCONE_FMT_I4 || FMT == SCONE_FMT_MXFP4;
  static constexpr int SCALE_SPAN = FMT == SCONE_FMT_I4 ? SCONE_I4_GROUP : FMT == SCONE_FMT_MXFP4 ? SCONE_MX_BLOCK : 0;
  static constexpr bool ROW_SCALE = SCALED && SCALE_SPAN == 0;
  // the raw scale bits of the run of elements that starts at element e0 of local row lr of a d-wide table: one load of the
  // scale's own width, for any lane and any row.  0 for a format without scales.
  template <typename E> static __device__ __forceinline__ uint32_t scale_bits(const void *scales, long long lr, int d, E e0) {
    if constexpr (FMT == SCONE_FMT_I8)
      return reinterpret_cast<const unsigned short *>(scales)[lr];
    else if constexpr (FMT == SCONE_FMT_I4)
      return reinterpret_cast<const unsigned short *>(scales)[lr * (d / SCONE_I4_GROUP) + scone_i4_scale_slot(e0 / SCONE_I4_GROUP, d)];
    else if constexpr (FMT == SCONE_FMT_MXFP4)
      return reinterpret_cast<const uint8_t *>(scales)[lr * (d / SCONE_MX_BLOCK) + scone_mx_scale_slot(e0 / SCONE_MX_BLOCK, d)];
    else
      return 0u;
  }
  // raw bits -> the fp32 operand of add_word (MXFP4: the E8M0 byte in an exponent field, see mx_accumulate)
  static __device__ __forceinline__ float scale_operand(uint32_t bits) {
    if constexpr (FMT == SCONE_FMT_MXFP4)
      return mx_scale_operand(bits);
    else if constexpr (SCALED)
      return __half2float(__ushort_as_half((unsigned short)bits));
    else
      return 1.0f;
  }
  // The wave-per-token bodies hold a row number that is wave-uniform, and a scalar load fetches whole dwords.  A per-row
  // scale is therefore fetched as the dword that holds the scales of rows lr and lr ^ 1, and picked by lr & 1:
  // scale_operand(SCONE_SCALE_OF_PAIR(bits, lr & 1, SCALE_BITS)).
  static __device__ __forceinline__ uint32_t row_pair_bits(const void *scales, long long lr) {
    static_assert(ROW_SCALE, "a format with one scale per row");
    return reinterpret_cast<const uint32_t *>(scales)[lr >> 1];
  }
  // d = 1024 (two 512-element segments): scone_i4_scale_slot / scone_mx_scale_slot order the scales so that the two a lane
  // of embed_token needs -- INT4: group lane / 16 of segment 0 and group 4 + lane / 16 of segment 1; MXFP4: block lane / 4 and
  // block 16 + lane / 4 -- are the two halves of ONE dword / ONE 16-bit word: one load and one register per row instead of two.
  // Segment s of the row takes scale_operand(SCONE_SCALE_OF_PAIR(bits, s != 0, SCALE_BITS)).
  static constexpr bool seg_pair(int d) { return SCALED && !ROW_SCALE && d == 1024; }
  static constexpr int SCALE_BITS = FMT == SCONE_FMT_MXFP4 ? 8 : 16;  // width of one stored scale
  static __device__ __forceinline__ uint32_t seg_pair_bits(const void *scales, long long lr, uint32_t lane) {
    constexpr int PAIRS = 1024 / SCALE_SPAN / 2, LANES = SCALE_SPAN / 8;  // pairs per row; lanes that share a scale
    if constexpr (SCALE_BITS == 16)
      return reinterpret_cast<const uint32_t *>(scales)[lr * PAIRS + lane / LANES];
    else
      return reinterpret_cast<const unsigned short *>(scales)[lr * PAIRS + lane / LANES];
  }
  // ---- accumulate -----------------------------------------------------------------------------------------------------
  // acc[0 .. EPW) += dequant(w), `sc` the scale_operand of the word's elements.  The products scale * q of INT8 / INT4 are
  // exact in fp32 (11-bit x 8-bit significands), so fmaf(scale, q, acc) == acc + fp32(scale * q): the same value the oracle
  // adds when it sums the dequantised fp32 table.  `tie`: p0, p1 are two accumulators of the word summed just before this one, for
  // the format whose decode has to be held behind them (MXFP4, see mx_accumulate); ignored by every other.
  static __device__ __forceinline__ void add_word(uint32_t w, float sc, float *acc, bool tie = false, float p0 = 0.f, float p1 = 0.f) {
    if constexpr (FMT == SCONE_FMT_F32) {
      acc[0] += __uint_as_float(w);
    } else if constexpr (FMT == SCONE_FMT_F16) {
      acc[0] += __half2float(__ushort_as_half((unsigned short)(w & 0xFFFFu)));
      acc[1] += __half2float(__ushort_as_half((unsigned short)(w >> 16)));
    } else if constexpr (FMT == SCONE_FMT_BF16) {  // a bf16 is the upper half of its fp32: bits << 16
      acc[0] += __uint_as_float(w << 16);
      acc[1] += __uint_as_float(w & 0xFFFF0000u);
    } else if constexpr (FMT == SCONE_FMT_I8) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int q = (int)(w << (24 - 8 * b)) >> 24;  // sign-extended byte b
        acc[b] = fmaf(sc, (float)q, acc[b]);
      }
    } else if constexpr (FMT == SCONE_FMT_MXFP4) {
      mx_accumulate(w, sc, acc, tie, p0, p1);
    } else {
      static_assert(FMT == SCONE_FMT_I4, "every table format has its own branch");
      i4_accumulate(w, sc, acc);
    }
  }
  // The second loop shape, for a body that holds the K rows of a token at once: acc[0 .. EPW) += word w[k * STRIDE] of every
  // row k = 0 .. K - 1, in list order, BEFORE the next word of any row.  BY_COLUMN formats must be summed this way by such a
  // body (bf16_accumulate_column says why); `prev` as above, null for the first column.
  static constexpr bool BY_COLUMN = FMT == SCONE_FMT_BF16;
  template <int K, int STRIDE> static __device__ __forceinline__ void add_column(const uint32_t *w, float *acc, const float *prev) {
    static_assert(BY_COLUMN, "a format summed column by column");
    bf16_accumulate_column<K, STRIDE>(w, acc[0], acc[1], prev);
  }
  // ---- mean -----------------------------------------------------------------------------------------------------------
  // sum / K of a lane's elements.  fp32 / fp16 / bf16 tables can hold anything (a sum may overflow, be subnormal, inf or NaN;
  // a bf16 row spans fp32's whole exponent range): the full IEEE quotient -- the `else` below is theirs, and a new format
  // belongs there unless its sums are provably in range (MXFP4 spans fp32's whole range too: the full quotient, in the form that
  // lets the zero sums of that format pass, scone_mean_div_of_sum).  A sum of INT8 / INT4 rows is +0 or a multiple of 2^-24 far below
  // overflow, where the short form IS the IEEE quotient (scone_mean_div.h).
  static __device__ __forceinline__ void mean_div(float *acc, const int n, const int k) {
    if constexpr (FMT == SCONE_FMT_I8 || FMT == SCONE_FMT_I4)
      scone_mean_div_in_range(acc, n, k);
    else if constexpr (FMT == SCONE_FMT_MXFP4)
      scone_mean_div_of_sum(acc, n, k);  // the full quotient; acc is a sum started at +0, and zero sums are common in this format
    else
      scone_mean_div(acc, n, k);
  }
};

}  // namespace scone_gather
