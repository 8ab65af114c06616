// acc[e] <- acc[e] / k, the one division of the mean (engine.py:250: embeddings.mean(dim=0)), for every lookup kernel.
//
// scone_mean_div: the IEEE-754 round-to-nearest-even quotient x / (float)k for EVERY fp32 x -- zeros of both signs,
// subnormals, infinities and NaN included -- and every list length k >= 2 an int holds: k = 2 .. max_n (max_n + 1) / 2
// for the hit-list kernels, any length for the CSR kernel.  k <= 2^24 is exact in a float; a longer list divides by k
// rounded to the nearest float, which is what dividing a float by an integer count does anywhere (torch.mean included).
//
// How: the three-instruction sequence  y = RN(1 / kf); q0 = RN(x y); r = x - q0 kf (exact inside the fma);
// q = RN(q0 + r y)  (Markstein) is the correctly rounded quotient whenever x is finite and the quotient is a normal
// number.  It is NOT outside that range: an infinite x (a sum that overflowed) gives inf - inf = NaN, a subnormal
// quotient can sit exactly half way between two fp32 values (it does for even k that are not a power of two) where
// r y instead of r / kf rounds to the wrong neighbour, and x = -0 comes out as +0.  In every one of those cases, and
// in no other, the first product q0 is not a normal number (zero, subnormal, infinite or NaN), so one class test per
// element on q0 finds them, and the lane then divides its elements with the true division instead.  Ordinary data
// never takes that branch.
//
// scone_mean_div_in_range: the three instructions alone, for sums that cannot leave their range: x is +0, or finite with
// |x / k| >= 2^-126.  That holds for every sum of INT8 / INT4 table rows: a dequantised value is an integer times an
// fp16 scale, i.e. a multiple of 2^-24 of magnitude <= 127 * 65504, so a sum of k <= 2^31 of them is +0 or a multiple
// of 2^-24 below 2^55.  (The test costs the INT8 headline 0.6 % of its time; the quantised kernels do
// not need it.)
//
// scone_mean_div_of_sum: scone_mean_div for an x that is a list-order sum started at +0.  Such a sum is never -0 (+0 + -0 = +0,
// and nothing added to a non-zero sum gives -0), and for x = +0 the three instructions give +0, the quotient; so a zero
// element need not send its lane through the true division.  For a table whose rows hold many zeros -- MXFP4: code 0 is one
// of 8 magnitudes, so with K = 2 rows a lane of 16 elements holds a zero sum in every fifth token -- that is the difference
// between the division being rare and being the rule.  Every other x is judged exactly as scone_mean_div judges it.
//
// Plain C: tests/mean_div_of_sum_host.c holds it to x / k for every x but -0.  tests/mean_div_host.c includes this file and holds both functions to x / k on the CPU (tests/test_mean_div_cpu.py).
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCONE_MEAN_DIV_FN __host__ __device__ __forceinline__
#else
#define SCONE_MEAN_DIV_FN static inline
#endif

#define SCONE_MEAN_DIV_MIN_NORMAL 1.17549435e-38f  // 2^-126

SCONE_MEAN_DIV_FN void scone_mean_div_in_range(float *acc, const int n, const int k) {
  const float kf = (float)k;
  const float y = 1.0f / kf;
#pragma unroll
  for (int e = 0; e < n; ++e) {
    const float x = acc[e];
    const float q0 = x * y;
    const float r = fmaf(-kf, q0, x);
    acc[e] = fmaf(r, y, q0);
  }
}

SCONE_MEAN_DIV_FN void scone_mean_div(float *acc, const int n, const int k) {
  const float kf = (float)k;
  const float y = 1.0f / kf;
  int fast = 1;
#pragma unroll
  for (int e = 0; e < n; ++e) {
    const float a0 = fabsf(acc[e] * y);
    // "q0 is a normal number" (one class test on the device); NaN fails the first comparison
    if (!(a0 >= SCONE_MEAN_DIV_MIN_NORMAL && a0 < INFINITY)) fast = 0;
  }
  if (fast) {
    scone_mean_div_in_range(acc, n, k);
  } else {
#pragma unroll
    for (int e = 0; e < n; ++e) acc[e] = acc[e] / kf;
  }
}

SCONE_MEAN_DIV_FN void scone_mean_div_of_sum(float *acc, const int n, const int k) {
  const float kf = (float)k;
  // the quotient is a normal number for certain, and x y with it, when 2^-125 kf <= |x| < inf (y = RN(1 / kf) >= (1 - 2^-24) / kf):
  // one threshold for all of the lane's elements instead of a product per element (x / k in [2^-126, 2^-125) takes the true
  // division too, which is always right)
  const float lo = kf * 2.3509887e-38f;  // 2^-125 kf
  int fast = 1;
#pragma unroll
  for (int e = 0; e < n; ++e) {
    const float a = fabsf(acc[e]);
    if (!((a >= lo && a < INFINITY) || a == 0.0f)) fast = 0;  // (a sum is never -0)
  }
  if (fast) {
    scone_mean_div_in_range(acc, n, k);
  } else {
#pragma unroll
    for (int e = 0; e < n; ++e) acc[e] = acc[e] / kf;
  }
}
