/* Host check of scone_amd/csrc/scone_mean_div.h: the helpers every lookup kernel divides its sum with must return
 * the IEEE quotient x / k: scone_mean_div for every fp32 x, scone_mean_div_in_range inside its stated range.  Built by tests/test_mean_div_cpu.py with
 *   gcc -O2 -ffp-contract=off -fno-fast-math -fopenmp mean_div_host.c -lm
 * Prints one line "checked N mismatches M" (plus the first few mismatches) and exits non-zero on any mismatch.
 *
 * Inputs, for k = 2..64 and a few large k (up to 2^24, the last count a float holds exactly, and some beyond it, which divide by the count rounded to a float):
 *   - every subnormal-range numerator x = +-n 2^-149, n < 2^16 (all the quotients are subnormal: the ties live here)
 *   - 2^24 pseudo-random bit patterns of the whole fp32 space (NaNs, infinities and subnormals among them)
 *   - 2^22 patterns drawn so that x / k falls within a few binades of FLT_MIN (the edge of the fast path)
 *   - the special values: +-0, +-inf, NaN, +-FLT_MAX, +-FLT_MIN, +-smallest subnormal, values next to k * FLT_MIN
 * scone_mean_div_in_range (the three instructions alone) is held to x / k on every one of those inputs that meets its
 * precondition ("in range N": about half of them).
 * Each x is divided alone (n = 1), so that it is judged by the path it takes itself; a quarter of them again inside a
 * block of 8 neighbours (the lanes' real use: one bad element sends the whole block through the true division).
 * Last, the control: the bare three-instruction quotient without the redo is counted on the subnormal numerators at
 * k = 6 and 10 and on x = inf ("bare shortcut mismatches": thousands, plus 2^32 for the NaN out of inf). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../scone_amd/csrc/scone_mean_div.h"

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static int same(float a, float b) { return (a != a && b != b) || bits_of(a) == bits_of(b); }

static uint32_t mix(uint64_t i) { /* splitmix64, high half */
  uint64_t z = i + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static long long n_checked, n_bad;
static long long n_in_range; /* per thread, summed at the end */
#pragma omp threadprivate(n_in_range)

static void report(float x, float kf, float got) {
#pragma omp critical
  {
    if (n_bad < 20)
      printf("MISMATCH x=%a (0x%08x) k=%.0f helper=%a (0x%08x) x/k=%a (0x%08x)\n", x, bits_of(x), kf, got, bits_of(got),
             x / kf, bits_of(x / kf));
    ++n_bad;
  }
}

static void check1(float x, int k) {
  const float kf = (float)k;
  volatile float vx = x, vk = kf; /* the reference quotient: one divss, nothing folded */
  const float want = vx / vk;
  float a = x;
  scone_mean_div(&a, 1, k);
  if (!same(a, want)) report(x, kf, a);
  /* the short form, wherever its precondition holds: x is +0, or finite with |x / k| >= 2^-126 */
  if (x == 0.0f ? !signbit(x) : (fabsf(x) >= kf * SCONE_MEAN_DIV_MIN_NORMAL && fabsf(x) < INFINITY)) {
    float b = x;
    scone_mean_div_in_range(&b, 1, k);
    if (!same(b, want)) report(x, kf, b);
    ++n_in_range;
  }
}

static void check8(const float *x, int k) {
  const float kf = (float)k;
  float a[8];
  memcpy(a, x, sizeof a);
  scone_mean_div(a, 8, k);
  for (int e = 0; e < 8; ++e) {
    volatile float vx = x[e], vk = kf;
    if (!same(a[e], vx / vk)) report(x[e], kf, a[e]);
  }
}

int main(void) {
  int ks[80];
  int nk = 0;
  for (int k = 2; k <= 64; ++k) ks[nk++] = k;
  const int big[] = {100, 127, 1000, 4097, 65535, 65536, 1000003, 16777215, 16777216, 16777217, 16777219, 1000000007, 2147483647};
  for (unsigned i = 0; i < sizeof big / sizeof big[0]; ++i) ks[nk++] = big[i];

  for (int ki = 0; ki < nk; ++ki) {
    const int k = ks[ki];
    const float kf = (float)k;
    /* special values */
    const uint32_t sp[] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00001u, 0x7F800001u,
                           0x7F7FFFFFu, 0xFF7FFFFFu, 0x00800000u, 0x80800000u, 0x00000001u, 0x80000001u, 0x007FFFFFu,
                           0x807FFFFFu, 0x00800001u, 0x3F800000u, 0xBF800000u, 0x7F000000u, 0x7EFFFFFFu};
    for (unsigned i = 0; i < sizeof sp / sizeof sp[0]; ++i) check1(from_bits(sp[i]), k);
    const float edge = kf * SCONE_MEAN_DIV_MIN_NORMAL; /* x / k == FLT_MIN here (exact product for these k) */
    for (int s = -64; s <= 64; ++s) {
      const uint32_t b = bits_of(edge) + (uint32_t)s;
      check1(from_bits(b), k);
      check1(from_bits(b | 0x80000000u), k);
    }
    n_checked += 20 + 2 * 129;

#pragma omp parallel for schedule(static)
    for (long long n = 0; n < 65536; ++n) { /* every numerator below 2^16 units of 2^-149, both signs */
      check1(from_bits((uint32_t)n), k);
      check1(from_bits((uint32_t)n | 0x80000000u), k);
    }
    n_checked += 2 * 65536;

#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (1ll << 24); i += 8) {
      float blk[8];
      for (int e = 0; e < 8; ++e) {
        blk[e] = from_bits(mix((uint64_t)ki << 40 | (uint64_t)(i + e)));
        check1(blk[e], k);
      }
      if ((i & 24) == 0) check8(blk, k);
    }
    n_checked += (1ll << 24) + (1ll << 22);

#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (1ll << 22); i += 8) {
      float blk[8];
      for (int e = 0; e < 8; ++e) {
        /* exponent field within 8 of the edge's own, random sign and mantissa: quotients around FLT_MIN */
        const uint32_t v = mix(((uint64_t)ki << 40 | (uint64_t)(i + e)) ^ 0x5555555555ull);
        int ex = (int)(bits_of(edge) >> 23) - 8 + (int)(v >> 27) % 16;
        if (ex < 0) ex = 0;
        blk[e] = from_bits((v & 0x807FFFFFu) | ((uint32_t)ex << 23));
        check1(blk[e], k);
      }
      check8(blk, k);
    }
    n_checked += 2ll << 22;
  }
  /* the control: the bare three-instruction quotient, without the redo, IS wrong on these inputs (so they can tell) */
  long long bare_bad = 0;
  for (int k = 6; k <= 10; k += 4)
    for (uint32_t n = 1; n < 65536; ++n) {
      const float x = from_bits(n), kf = (float)k, y = 1.0f / kf;
      const float q0 = x * y;
      const float q = fmaf(fmaf(-kf, q0, x), y, q0);
      volatile float vx = x, vk = kf;
      bare_bad += !same(q, vx / vk);
    }
  {
    const float inf = from_bits(0x7F800000u), y = 1.0f / 3.0f, q0 = inf * y;
    bare_bad += !same(fmaf(fmaf(-3.0f, q0, inf), y, q0), inf) ? (1ll << 32) : 0;
  }
  printf("bare shortcut mismatches %lld\n", bare_bad);
  long long in_range = 0;
#pragma omp parallel reduction(+ : in_range)
  in_range += n_in_range;
  printf("in range %lld\n", in_range);
  printf("checked %lld mismatches %lld\n", n_checked, n_bad);
  return n_bad ? 1 : 0;
}
