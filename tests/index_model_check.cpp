// TEST INFRASTRUCTURE -- prints what the product's own __host__ __device__ index functions (scone_amd/csrc/scone_common.h) make
// of a list of keys, so that tests/test_index_model_host.py can hold the Python restatement in tests/index_model.py to them.
// Host only (hipcc -x hip --cuda-host-only); nothing here touches a GPU.
//
// Input (the file named by argv[1], or stdin), one key per line, decimal:
//   max_n n t0 t1 t2 t3 slot_mask bloom_mask
// Output, one line per key, decimal:
//   ok lo ext hash home_bucket step bloom_bit
#include <cinttypes>
#include <cstdio>

#include "../scone_amd/csrc/scone_common.h"

int main(int argc, char **argv) {
  FILE *in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!in) {
    std::fprintf(stderr, "index_model_check: cannot open %s\n", argv[1]);
    return 2;
  }
  int max_n, n;
  uint32_t t[4];
  unsigned long long slot_mask, bloom_mask;
  unsigned long long lines = 0;
  for (;;) {
    const int got = std::fscanf(in, "%d %d %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %llu %llu", &max_n, &n, &t[0], &t[1], &t[2],
                                &t[3], &slot_mask, &bloom_mask);
    if (got == EOF) break;
    if (got != 8 || max_n < 1 || max_n > SCONE_MAX_N || n < 1 || n > max_n) {
      std::fprintf(stderr, "index_model_check: bad line %llu\n", lines + 1);
      return 2;
    }
    const scone_key k = scone_pack_key(t, n, max_n);
    const unsigned long long h = scone_hash_key(k.lo, k.ext);
    std::printf("%d %llu %" PRIu32 " %llu %llu %llu %llu\n", k.ok ? 1 : 0, k.lo, k.ext, h, scone_bucket_home(h, slot_mask),
                scone_bucket_step(h), scone_bloom_bit(h, bloom_mask));
    ++lines;
  }
  if (in != stdin) std::fclose(in);
  return 0;
}
