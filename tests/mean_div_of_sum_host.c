/* Host check of scone_mean_div_of_sum (scone_amd/csrc/scone_mean_div.h): the division the MXFP4 lookups take.  It must return
 * the IEEE quotient x / k for every fp32 x EXCEPT -0 (a list-order sum that started at +0 is never -0), zeros included
 * without the true division.  Built by tests/test_mean_div_of_sum_cpu.py with
 *   gcc -O2 -ffp-contract=off -fno-fast-math mean_div_of_sum_host.c -lm
 * For k = 2..64 and a few large k: x = +0; every subnormal-range numerator +-n 2^-149, n < 2^16; 2^19 pseudo-random bit patterns
 * of the whole fp32 space; 2^18 patterns whose quotient lies within a few binades of FLT_MIN (the edge of the threshold
 * 2^-125 k); the special values.  Each x alone and again inside a block of 8 whose other elements are zeros (a zero must not
 * change the path of its neighbours, nor be changed by it).  Prints "checked N mismatches M zero_blocks_fast Z". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../scone_amd/csrc/scone_mean_div.h"

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static int same(float a, float b) { return (a != a && b != b) || bits_of(a) == bits_of(b); }
static uint32_t mix(uint64_t i) { /* splitmix64, high half */
  uint64_t z = i + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static long long n_checked, n_bad;

static void check(float x, int k) {
  if (bits_of(x) == 0x80000000u) return; /* -0: outside the function's domain */
  const float kf = (float)k;
  volatile float vx = x, vk = kf;
  const float want = vx / vk;
  float one = x;
  scone_mean_div_of_sum(&one, 1, k);
  float blk[8] = {0.f, 0.f, 0.f, x, 0.f, 0.f, 0.f, 0.f};
  scone_mean_div_of_sum(blk, 8, k);
  int ok = same(one, want) && same(blk[3], want);
  for (int e = 0; e < 8; ++e)
    if (e != 3 && bits_of(blk[e]) != 0u) ok = 0; /* +0 / k = +0 */
  n_checked += 2;
  if (!ok) {
    if (n_bad < 20) printf("MISMATCH x=%a (0x%08x) k=%d alone=%a in block=%a x/k=%a\n", x, bits_of(x), k, one, blk[3], want);
    ++n_bad;
  }
}

int main(void) {
  static const int big[] = {100, 127, 128, 1000, 4095, 65536, 1000003, 16777215, 16777216, 16777217, 100000000};
  int ks[80], nk = 0;
  for (int k = 2; k <= 64; ++k) ks[nk++] = k;
  for (unsigned i = 0; i < sizeof(big) / sizeof(big[0]); ++i) ks[nk++] = big[i];
  static const uint32_t special[] = {0x00000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00001u, 0x7F7FFFFFu, 0xFF7FFFFFu,
                                     0x00800000u, 0x80800000u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu, 0x01000000u};
  for (int j = 0; j < nk; ++j) {
    const int k = ks[j];
    for (unsigned i = 0; i < sizeof(special) / sizeof(special[0]); ++i) check(from_bits(special[i]), k);
    for (uint32_t n = 1; n < (1u << 16); ++n) {
      check(from_bits(n), k);
      check(from_bits(n | 0x80000000u), k);
    }
    for (uint32_t i = 0; i < (1u << 19); ++i) check(from_bits(mix(((uint64_t)k << 32) | i)), k);
    for (uint32_t i = 0; i < (1u << 18); ++i) { /* quotient near FLT_MIN: |x| = k * 2^-126 * 2^[-3, 3) */
      const uint32_t r = mix(((uint64_t)(k + 1000) << 32) | i);
      float x = (float)k * ldexpf(1.0f + (float)(r & 0x7FFFFF) / 8388608.0f, -126 + (int)((r >> 23) & 7) - 3 - 1);
      x += ldexpf((float)((int)((r >> 26) & 3) - 1), -149);
      check((r >> 31) ? -x : x, k);
    }
    /* the exact threshold and its neighbours */
    const float lo = (float)k * 2.3509887e-38f;
    check(lo, k); check(nextafterf(lo, 0.f), k); check(nextafterf(lo, 1.f), k); check(-lo, k); check(-nextafterf(lo, 0.f), k);
  }
  /* a block of zeros takes the three-instruction path: the result is +0 and no division is needed (the claim of the header) */
  long long zero_fast = 0;
  for (int j = 0; j < nk; ++j) {
    float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    scone_mean_div_in_range(z, 8, ks[j]);
    int ok = 1;
    for (int e = 0; e < 8; ++e) ok = ok && bits_of(z[e]) == 0u;
    zero_fast += ok;
  }
  printf("checked %lld mismatches %lld zero_blocks_fast %lld of %d\n", n_checked, n_bad, zero_fast, nk);
  return n_bad != 0 || zero_fast != nk;
}
