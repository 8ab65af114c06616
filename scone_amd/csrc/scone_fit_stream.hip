// Streaming f-gram vocabulary construction: scone_fit (scone_fit.hip) as a counter that can be fed in chunks of whole
// texts, grows with the DISTINCT n-grams seen, can be finalised any number of times, exported and merged -- what
// collections.Counter gives the reference's fit for free (scone/tokenization/n_gram_extractor.py:72-104, :59-70).
//
// State: the exact-key open-addressing table of scone_fit and of the lookup index (scone_pack_key / scone_hash_key /
// scone_slot, slot claim by CAS, never a wait) with two side arrays per slot: a 64-bit count (atomicAdd) and the 64-bit
// first sequence number (atomicMin): 32 B per slot.  A device counter holds the number of distinct keys; it is bumped by
// the one thread whose CAS wrote a slot's tag word.
//
// Order of every mutating call: validate (a pass of its own; a refused call changes nothing) -> grow if the table could
// not hold 2 x (distinct + new entries) slots -> count.  Growth is never taken inside a chunk, so a count's probe loop
// always ends and no key is ever dropped; the result is a function of the multiset of (key, sequence number) pairs fed
// and not of chunking, growth history or order (count: a sum; first: a minimum).
//
// Key-hash partitions (scone_fit_update_part): the same call counting only the keys whose hash falls into one of n_parts parts.
// A key lives in exactly one part, so its count and first number are complete there, and each part is finalised on its own
// (scone_fit_finalize_seq gives rows that scone_fit_merge takes): device memory follows the distinct keys of ONE part.
//
// Half-written slots: a slot whose lo word is claimed and whose tag word is still 0 exists only INSIDE a count / merge /
// rehash launch, where every reader goes through the CAS on the tag word.  Every launch that reads the table otherwise
// (rehash source, export, finalise) runs after the writer's launch has completed on the stream, and tests the tag word.
#include "scone_common.h"

#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

struct scone_fit_state {
  int device;
  int max_n;
  scone_slot *slots;
  unsigned long long *cnt;    // [cap] occurrences of the slot's key
  unsigned long long *first;  // [cap] smallest sequence number of the slot's key (all ones while unseen)
  unsigned long long cap;     // power of two >= 1024
  unsigned long long *d_counters;  // [0] distinct keys (persistent), [1] scratch of finalise / export
  uint32_t *d_status;
  void *scratch;  // per-chunk text tables and the scan's workspace; grows, never shrinks
  size_t scratch_bytes;
  unsigned long long n_distinct, n_occ, n_grows, next_seq;  // host mirrors, exact after every call (each one synchronises)
};

namespace {

#define FIT_ST_BAD_OFFSETS 0x100u  // this file's own status bit, beside SCONE_ST_BAD_TOKEN
#define FIT_ST_BAD_LEN 0x200u
#define FIT_MIN_SLOTS 1024ull

// number of n-gram occurrences of a text of length L: sum_{n=1..min(max_n,L)} (L - n + 1)   (scone_fit.hip's occ_of)
__host__ __device__ inline unsigned long long occ_of(long long L, int max_n) {
  unsigned long long s = 0;
  for (int n = 1; n <= max_n; ++n)
    if (L - n + 1 > 0) s += (unsigned long long)(L - n + 1);
  return s;
}

__device__ inline unsigned long long grid_tid() { return (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ inline unsigned long long grid_size() { return (unsigned long long)gridDim.x * blockDim.x; }

// The validating pre-pass of scone_fit_update: every token non-negative and representable by scone_pack_key, the
// offsets start at 0, never decrease and end at n_tokens; and the occurrence count of every text for the scan.
// Reads tok[0, n_tokens) and offsets[0, n_texts] only, whatever they hold.
__global__ __launch_bounds__(256) void k_fits_validate(const int32_t *__restrict__ tok, long long n_tokens,
                                                       const long long *__restrict__ offsets, long long n_texts, int max_n,
                                                       unsigned long long *__restrict__ occ, uint32_t *__restrict__ status) {
  const long long work = n_tokens > n_texts ? n_tokens : n_texts;
  for (long long i = (long long)grid_tid(); i < work; i += (long long)grid_size()) {
    if (i < n_tokens) {
      const int32_t v = tok[i];
      if (v < 0 || (max_n > 3 && (uint32_t)v >= 0xFFFFFFu)) atomicOr(status, SCONE_ST_BAD_TOKEN);
    }
    if (i < n_texts) {
      const long long a = offsets[i], b = offsets[i + 1];
      if (b < a || (i == 0 && a != 0) || (i == n_texts - 1 && b != n_tokens)) atomicOr(status, FIT_ST_BAD_OFFSETS);
      occ[i] = b >= a ? occ_of(b - a, max_n) : 0ull;
    }
  }
}

// The key-hash partition of scone_fit_partition / scone_fit_update_part (the formula is a contract, include/scone_hip.h): the
// UPPER 32 bits of the hash scaled to [0, n_parts).  The home slot is hash & mask, the LOWER bits, so the keys of one part
// still spread over the whole table; a partition taken from the lower bits would leave a part 1 / n_parts of the home slots.
__host__ __device__ inline uint32_t fits_part_of(unsigned long long hash, uint32_t n_parts) {
  return (uint32_t)(((hash >> 32) * (unsigned long long)n_parts) >> 32);
}

// Find-or-claim the slot of (lo, tag), probing from the home slot s.  Returns the slot; *claimed = this thread wrote the tag
// word.  The table always has room (growth rule), so the loop ends; cap + 1 probes without success returns ~0 and the caller
// raises INDEX_FULL.
__device__ inline unsigned long long fits_slot_from(scone_slot *slots, unsigned long long mask, unsigned long long s,
                                                    unsigned long long lo, unsigned long long tag, bool *claimed) {
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    const unsigned long long old = atomicCAS(&slots[s].lo, 0ull, lo);
    if (old == 0ull || old == lo) {
      const unsigned long long prev = atomicCAS(&slots[s].hi, 0ull, tag);
      if (prev == 0ull || prev == tag) {
        *claimed = prev == 0ull;
        return s;
      }
    }
    s = (s + 1ull) & mask;
  }
  return ~0ull;
}

__device__ inline unsigned long long fits_slot_of(scone_slot *slots, unsigned long long mask, unsigned long long lo,
                                                  unsigned long long tag, uint32_t ext, bool *claimed) {
  return fits_slot_from(slots, mask, scone_hash_key(lo, ext) & mask, lo, tag, claimed);
}

// One item per (flat token position g, n): count the n-gram starting at g if it fits in its text (k_fit_count with 64-bit
// counts, a caller-given sequence base and the distinct counter).  The chunk has passed k_fits_validate.
// PART: count only the keys of partition `part` of `n_parts` (scone_fit_update_part).  The key is hashed once; an
// out-of-partition key leaves before the first CAS, so it never claims a slot or touches n_distinct, and the hash is reused for
// the home slot.  Its occurrence still has its sequence number: numbering is by position, not by what is counted.  With PART
// false the two trailing arguments are unused and the kernel is scone_fit_update's as it always was.
template <bool PART>
__global__ __launch_bounds__(256) void k_fits_count(scone_slot *__restrict__ slots, unsigned long long mask,
                                                    unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ first,
                                                    const int32_t *__restrict__ tok, long long n_tokens,
                                                    const long long *__restrict__ offsets, long long n_texts,
                                                    const unsigned long long *__restrict__ base_seq, unsigned long long seq_base,
                                                    int max_n, unsigned long long *__restrict__ n_distinct,
                                                    uint32_t *__restrict__ status, uint32_t part, uint32_t n_parts) {
  const unsigned long long work = (unsigned long long)n_tokens * (unsigned long long)max_n;
  for (unsigned long long gid = grid_tid(); gid < work; gid += grid_size()) {
    const int n = (int)(gid / (unsigned long long)n_tokens) + 1;
    const long long g = (long long)(gid - (unsigned long long)(n - 1) * (unsigned long long)n_tokens);
    // text of g: largest t with offsets[t] <= g
    long long lo = 0, hi = n_texts;
    while (hi - lo > 1) {
      const long long mid = (lo + hi) >> 1;
      if (offsets[mid] <= g) lo = mid;
      else hi = mid;
    }
    const long long t0 = offsets[lo], L = offsets[lo + 1] - t0, i = g - t0;
    if (i + n > L) continue;
    uint32_t k[SCONE_MAX_N] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < SCONE_MAX_N; ++j)
      if (j < n) k[j] = (uint32_t)tok[g + j];
    const scone_key key = scone_pack_key(k, n, max_n);
    unsigned long long hash = 0ull;
    if constexpr (PART) {
      hash = scone_hash_key(key.lo, key.ext);
      if (fits_part_of(hash, n_parts) != part) continue;
    }
    // insertion order inside the text: all 1-grams, then all 2-grams, ...
    unsigned long long seq = seq_base + base_seq[lo] + (unsigned long long)i;
    for (int m = 1; m < n; ++m) seq += (unsigned long long)(L - m + 1);
    const unsigned long long tag = ((unsigned long long)key.ext << 32) | 1ull;
    bool claimed = false;
    unsigned long long s;
    if constexpr (PART) s = fits_slot_from(slots, mask, hash & mask, key.lo, tag, &claimed);
    else s = fits_slot_of(slots, mask, key.lo, tag, key.ext, &claimed);
    if (s == ~0ull) {
      atomicOr(status, SCONE_ST_INDEX_FULL);
      continue;
    }
    if (claimed) atomicAdd(n_distinct, 1ull);
    atomicAdd(&cnt[s], 1ull);
    atomicMin(&first[s], seq);
  }
}

// Growth: every complete slot of the old table moves to the new one with its count and first number.  Keys are distinct,
// so each new slot has one writer; the claim still goes through the two CAS steps because two keys may share the lo word.
__global__ __launch_bounds__(256) void k_fits_rehash(const scone_slot *__restrict__ old_slots,
                                                     const unsigned long long *__restrict__ old_cnt,
                                                     const unsigned long long *__restrict__ old_first, unsigned long long old_cap,
                                                     scone_slot *__restrict__ slots, unsigned long long mask,
                                                     unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ first,
                                                     uint32_t *__restrict__ status) {
  for (unsigned long long o = grid_tid(); o < old_cap; o += grid_size()) {
    const scone_slot sl = old_slots[o];
    if (sl.hi == 0ull) continue;
    bool claimed = false;
    const unsigned long long s = fits_slot_of(slots, mask, sl.lo, sl.hi, (uint32_t)(sl.hi >> 32), &claimed);
    if (s == ~0ull) {
      atomicOr(status, SCONE_ST_INDEX_FULL);
      continue;
    }
    cnt[s] = old_cnt[o];
    first[s] = old_first[o];
  }
}

// packed slot -> token ids (+1 removed) and length (k_fit_emit's decoding)
__device__ inline int fits_unpack(const scone_slot sl, int max_n, uint32_t *out) {
  const uint32_t ext = (uint32_t)(sl.hi >> 32);
  uint32_t v[4];
  if (max_n <= 3) {
    v[0] = (uint32_t)sl.lo, v[1] = (uint32_t)(sl.lo >> 32), v[2] = ext, v[3] = 0;
  } else {
    v[0] = (uint32_t)(sl.lo & 0xFFFFFFu), v[1] = (uint32_t)((sl.lo >> 24) & 0xFFFFFFu);
    v[2] = (uint32_t)((sl.lo >> 48) & 0xFFFFu) | ((ext & 0xFFu) << 16), v[3] = ext >> 8;
  }
  int len = 0;
  for (int j = 0; j < max_n; ++j) {
    out[j] = v[j] ? v[j] - 1u : 0u;
    if (v[j]) len = j + 1;
  }
  return len;
}

__global__ __launch_bounds__(256) void k_fits_export(const scone_slot *__restrict__ slots,
                                                     const unsigned long long *__restrict__ cnt,
                                                     const unsigned long long *__restrict__ first, unsigned long long cap,
                                                     int max_n, unsigned long long out_cap, unsigned long long *__restrict__ n_out,
                                                     uint32_t *__restrict__ keys, uint8_t *__restrict__ lens,
                                                     unsigned long long *__restrict__ counts,
                                                     unsigned long long *__restrict__ firsts) {
  for (unsigned long long s = grid_tid(); s < cap; s += grid_size()) {
    const scone_slot sl = slots[s];
    if (sl.hi == 0ull) continue;
    const unsigned long long j = atomicAdd(n_out, 1ull);
    if (j >= out_cap) continue;
    uint32_t v[SCONE_MAX_N];
    const int len = fits_unpack(sl, max_n, v);
    for (int i = 0; i < max_n; ++i) keys[j * max_n + i] = v[i];
    lens[j] = (uint8_t)len;
    counts[j] = cnt[s];
    firsts[j] = first[s];
  }
}

// The validating pre-pass of scone_fit_merge: lengths in 1..max_n, keys representable.
__global__ __launch_bounds__(256) void k_fits_merge_validate(const uint32_t *__restrict__ keys, const uint8_t *__restrict__ lens,
                                                             unsigned long long n, int max_n, uint32_t *__restrict__ status) {
  for (unsigned long long i = grid_tid(); i < n; i += grid_size()) {
    const int len = lens[i];
    if (len < 1 || len > max_n) {
      atomicOr(status, FIT_ST_BAD_LEN);
      continue;
    }
    uint32_t k[SCONE_MAX_N] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < SCONE_MAX_N; ++j)
      if (j < len) k[j] = keys[i * max_n + j];
    if (!scone_pack_key(k, len, max_n).ok) atomicOr(status, SCONE_ST_BAD_TOKEN);
  }
}

// count += counts[i], first = min(first, first[i]); the entries have passed k_fits_merge_validate
__global__ __launch_bounds__(256) void k_fits_merge(scone_slot *__restrict__ slots, unsigned long long mask,
                                                    unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ first,
                                                    const uint32_t *__restrict__ keys, const uint8_t *__restrict__ lens,
                                                    const unsigned long long *__restrict__ counts,
                                                    const unsigned long long *__restrict__ firsts, unsigned long long n, int max_n,
                                                    unsigned long long *__restrict__ n_distinct, uint32_t *__restrict__ status) {
  for (unsigned long long i = grid_tid(); i < n; i += grid_size()) {
    const int len = lens[i];
    uint32_t k[SCONE_MAX_N] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < SCONE_MAX_N; ++j)
      if (j < len) k[j] = keys[i * max_n + j];
    const scone_key key = scone_pack_key(k, len, max_n);
    const unsigned long long tag = ((unsigned long long)key.ext << 32) | 1ull;
    bool claimed = false;
    const unsigned long long s = fits_slot_of(slots, mask, key.lo, tag, key.ext, &claimed);
    if (s == ~0ull) {
      atomicOr(status, SCONE_ST_INDEX_FULL);
      continue;
    }
    if (claimed) atomicAdd(n_distinct, 1ull);
    atomicAdd(&cnt[s], counts[i]);
    atomicMin(&first[s], firsts[i]);
  }
}

// finalise, pass 1: how many entries are eligible (sizes every buffer of pass 2 and of the sorts)
__global__ __launch_bounds__(256) void k_fits_eligible(const unsigned long long *__restrict__ cnt, unsigned long long cap,
                                                       unsigned long long min_freq, unsigned long long *__restrict__ n_sel) {
  for (unsigned long long s = grid_tid(); s < cap; s += grid_size()) {
    const unsigned long long c = cnt[s];
    if (c != 0ull && c >= min_freq) atomicAdd(n_sel, 1ull);
  }
}

// finalise, pass 2: (first number, slot) of every eligible entry, in any order (the sort by first number follows);
// sel_cap is pass 1's count, which this pass reproduces exactly because nothing wrote to the table in between
__global__ __launch_bounds__(256) void k_fits_compact(const unsigned long long *__restrict__ cnt,
                                                      const unsigned long long *__restrict__ first, unsigned long long cap,
                                                      unsigned long long min_freq, unsigned long long sel_cap,
                                                      unsigned long long *__restrict__ n_sel,
                                                      unsigned long long *__restrict__ sel_first,
                                                      unsigned long long *__restrict__ sel_slot) {
  for (unsigned long long s = grid_tid(); s < cap; s += grid_size()) {
    const unsigned long long c = cnt[s];
    if (c == 0ull || c < min_freq) continue;
    const unsigned long long j = atomicAdd(n_sel, 1ull);
    if (j >= sel_cap) continue;
    sel_first[j] = first[s];
    sel_slot[j] = s;
  }
}

__global__ __launch_bounds__(256) void k_fits_gather_counts(const unsigned long long *__restrict__ cnt,
                                                            const unsigned long long *__restrict__ slot, unsigned long long m,
                                                            unsigned long long *__restrict__ out) {
  for (unsigned long long j = grid_tid(); j < m; j += grid_size()) out[j] = cnt[slot[j]];
}

// counts and firsts are optional outputs (firsts: scone_fit_finalize_seq; first[] is the state's per-slot array)
__global__ __launch_bounds__(256) void k_fits_emit(const scone_slot *__restrict__ slots,
                                                   const unsigned long long *__restrict__ first,
                                                   const unsigned long long *__restrict__ slot,
                                                   const unsigned long long *__restrict__ cnt_sorted, unsigned long long n_out,
                                                   int max_n, uint32_t *__restrict__ keys, uint8_t *__restrict__ lens,
                                                   unsigned long long *__restrict__ counts,
                                                   unsigned long long *__restrict__ firsts) {
  for (unsigned long long r = grid_tid(); r < n_out; r += grid_size()) {
    const unsigned long long s = slot[r];
    uint32_t v[SCONE_MAX_N];
    const int len = fits_unpack(slots[s], max_n, v);
    for (int j = 0; j < max_n; ++j) keys[r * max_n + j] = v[j];
    lens[r] = (uint8_t)len;
    if (counts) counts[r] = cnt_sorted[r];
    if (firsts) firsts[r] = first[s];
  }
}

struct dev_buf {
  void *p = nullptr;
  ~dev_buf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
  template <typename T> T *as() { return reinterpret_cast<T *>(p); }
  void *release() {
    void *q = p;
    p = nullptr;
    return q;
  }
};

inline unsigned blocks_for(unsigned long long items) { return scone_capped_blocks((items + 255) / 256); }

}  // namespace

#define FIT_HIP(call)                                                \
  do {                                                               \
    hipError_t e__ = (call);                                         \
    if (e__ != hipSuccess) {                                         \
      (void)hipGetLastError();                                       \
      return e__ == hipErrorOutOfMemory ? SCONE_ENOMEM : SCONE_EHIP; \
    }                                                                \
  } while (0)

// The table must hold 2 * need slots; if it does not, move it to the smallest power of two that does.  The old arrays are
// freed only after the new ones are complete, so every failure leaves the state as it was.
static int fits_grow(scone_fit_state *st, unsigned long long need, hipStream_t s) {
  if (need > (1ull << 61)) return SCONE_ENOMEM;
  if (st->cap >= 2 * need) return SCONE_OK;
  unsigned long long cap = FIT_MIN_SLOTS;
  while (cap < 2 * need) cap <<= 1;
  dev_buf slots, cnt, first;
  FIT_HIP(slots.alloc(cap * sizeof(scone_slot)));
  FIT_HIP(cnt.alloc(cap * 8));
  FIT_HIP(first.alloc(cap * 8));
  FIT_HIP(hipMemsetAsync(slots.p, 0, cap * sizeof(scone_slot), s));
  FIT_HIP(hipMemsetAsync(cnt.p, 0, cap * 8, s));
  FIT_HIP(hipMemsetAsync(first.p, 0xFF, cap * 8, s));
  FIT_HIP(hipMemsetAsync(st->d_status, 0, 4, s));
  hipLaunchKernelGGL(k_fits_rehash, dim3(blocks_for(st->cap)), dim3(256), 0, s, st->slots, st->cnt, st->first, st->cap,
                     slots.as<scone_slot>(), cap - 1, cnt.as<unsigned long long>(), first.as<unsigned long long>(), st->d_status);
  FIT_HIP(hipGetLastError());
  uint32_t h_status = 0;
  FIT_HIP(hipMemcpyAsync(&h_status, st->d_status, 4, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipStreamSynchronize(s));
  if (h_status) return SCONE_ENOMEM;  // cannot happen: the new table is at most half full
  (void)hipFree(st->slots);
  (void)hipFree(st->cnt);
  (void)hipFree(st->first);
  st->slots = (scone_slot *)slots.release();
  st->cnt = (unsigned long long *)cnt.release();
  st->first = (unsigned long long *)first.release();
  st->cap = cap;
  ++st->n_grows;
  return SCONE_OK;
}

static int fits_scratch(scone_fit_state *st, size_t bytes) {
  if (bytes <= st->scratch_bytes) return SCONE_OK;
  void *p = nullptr;
  FIT_HIP(hipMalloc(&p, bytes));
  if (st->scratch) (void)hipFree(st->scratch);
  st->scratch = p;
  st->scratch_bytes = bytes;
  return SCONE_OK;
}

extern "C" void scone_fit_destroy(scone_fit_state *st) {
  if (!st) return;
  {
    scone_device_guard dev_guard__(st->device);
    if (st->slots) (void)hipFree(st->slots);
    if (st->cnt) (void)hipFree(st->cnt);
    if (st->first) (void)hipFree(st->first);
    if (st->d_counters) (void)hipFree(st->d_counters);
    if (st->d_status) (void)hipFree(st->d_status);
    if (st->scratch) (void)hipFree(st->scratch);
  }
  delete st;
}

static int fits_init(scone_fit_state *st) {
  FIT_HIP(hipMalloc((void **)&st->slots, st->cap * sizeof(scone_slot)));
  FIT_HIP(hipMalloc((void **)&st->cnt, st->cap * 8));
  FIT_HIP(hipMalloc((void **)&st->first, st->cap * 8));
  FIT_HIP(hipMalloc((void **)&st->d_counters, 16));
  FIT_HIP(hipMalloc((void **)&st->d_status, 4));
  FIT_HIP(hipMemset(st->slots, 0, st->cap * sizeof(scone_slot)));
  FIT_HIP(hipMemset(st->cnt, 0, st->cap * 8));
  FIT_HIP(hipMemset(st->first, 0xFF, st->cap * 8));
  FIT_HIP(hipMemset(st->d_counters, 0, 16));
  FIT_HIP(hipMemset(st->d_status, 0, 4));
  FIT_HIP(hipDeviceSynchronize());
  return SCONE_OK;
}

extern "C" int scone_fit_create(int32_t device, int32_t max_n, uint64_t initial_slots, scone_fit_state **out) {
  if (!out) return SCONE_EINVAL;
  *out = nullptr;
  if (max_n < 1 || max_n > SCONE_MAX_N || device < 0 || initial_slots > (1ull << 40)) return SCONE_EINVAL;
  scone_device_guard dev_guard__(device);  // the caller's current device is restored on return
  FIT_HIP(dev_guard__.err);
  scone_fit_state *st = new (std::nothrow) scone_fit_state();
  if (!st) return SCONE_ENOMEM;
  st->device = device;
  st->max_n = max_n;
  st->cap = FIT_MIN_SLOTS;
  while (st->cap < initial_slots) st->cap <<= 1;
  const int rc = fits_init(st);
  if (rc != SCONE_OK) {
    scone_fit_destroy(st);
    return rc;
  }
  *out = st;
  return SCONE_OK;
}

extern "C" int scone_fit_stats(scone_fit_state *st, uint64_t *n_distinct, uint64_t *n_occurrences, uint64_t *slots,
                               uint64_t *n_grows, uint64_t *next_seq) {
  if (!st) return SCONE_EINVAL;
  if (n_distinct) *n_distinct = st->n_distinct;
  if (n_occurrences) *n_occurrences = st->n_occ;
  if (slots) *slots = st->cap;
  if (n_grows) *n_grows = st->n_grows;
  if (next_seq) *next_seq = st->next_seq;
  return SCONE_OK;
}

// scone_fit_update (n_parts = 1: the unfiltered kernel) and scone_fit_update_part (n_parts > 1: the filtering one).  Everything
// but the count launch is shared: validation, numbering and growth look at ALL occurrences of the chunk.
static int fits_update(scone_fit_state *st, const int32_t *d_tokens, int64_t n_tokens, const int64_t *d_text_offsets,
                       int64_t n_texts, uint64_t seq_base, uint32_t part, uint32_t n_parts, scone_stream_t stream) {
  if (!st || n_tokens < 0 || n_texts < 0) return SCONE_EINVAL;
  if (n_tokens == 0 || n_texts == 0) return SCONE_OK;
  if (!d_tokens || !d_text_offsets) return SCONE_EINVAL;
  scone_device_guard dev_guard__(st->device);
  FIT_HIP(dev_guard__.err);
  hipStream_t s = (hipStream_t)stream;
  const int max_n = st->max_n;

  // scratch: occ[n_texts] | base[n_texts] | the scan's workspace
  size_t tmp_bytes = 0;
  FIT_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull,
                                  (size_t)n_texts, rocprim::plus<unsigned long long>(), s));
  const size_t tab = ((size_t)n_texts * 8 + 255) & ~(size_t)255;
  const int rc_s = fits_scratch(st, 2 * tab + tmp_bytes + 256);
  if (rc_s != SCONE_OK) return rc_s;
  unsigned long long *occ = (unsigned long long *)st->scratch;
  unsigned long long *base = (unsigned long long *)((char *)st->scratch + tab);
  void *tmp = (char *)st->scratch + 2 * tab;

  // 1. validate; occurrences per text; base sequence number of every text (exclusive scan)
  FIT_HIP(hipMemsetAsync(st->d_status, 0, 4, s));
  const unsigned long long vwork = (unsigned long long)(n_tokens > n_texts ? n_tokens : n_texts);
  hipLaunchKernelGGL(k_fits_validate, dim3(blocks_for(vwork)), dim3(256), 0, s, d_tokens, (long long)n_tokens,
                     (const long long *)d_text_offsets, (long long)n_texts, max_n, occ, st->d_status);
  FIT_HIP(hipGetLastError());
  FIT_HIP(rocprim::exclusive_scan(tmp, tmp_bytes, occ, base, 0ull, (size_t)n_texts, rocprim::plus<unsigned long long>(), s));
  uint32_t h_status = 0;
  unsigned long long h_last[2] = {0, 0};
  FIT_HIP(hipMemcpyAsync(&h_status, st->d_status, 4, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipMemcpyAsync(&h_last[0], base + (n_texts - 1), 8, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipMemcpyAsync(&h_last[1], occ + (n_texts - 1), 8, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipStreamSynchronize(s));
  if (h_status & FIT_ST_BAD_OFFSETS) return SCONE_EINVAL;
  if (h_status & SCONE_ST_BAD_TOKEN) return SCONE_ERANGE;
  const unsigned long long chunk_occ = h_last[0] + h_last[1];
  if (chunk_occ == 0) return SCONE_OK;  // only empty texts

  // 2. grow before the count, never inside it
  const int rc_g = fits_grow(st, st->n_distinct + chunk_occ, s);
  if (rc_g != SCONE_OK) return rc_g;

  // 3. count
  const unsigned long long seq0 = seq_base == UINT64_MAX ? st->next_seq : seq_base;
  const unsigned long long work = (unsigned long long)n_tokens * (unsigned long long)max_n;
  if (n_parts > 1)
    hipLaunchKernelGGL(k_fits_count<true>, dim3(blocks_for(work)), dim3(256), 0, s, st->slots, st->cap - 1, st->cnt, st->first,
                       d_tokens, (long long)n_tokens, (const long long *)d_text_offsets, (long long)n_texts, base, seq0, max_n,
                       st->d_counters, st->d_status, part, n_parts);
  else
    hipLaunchKernelGGL(k_fits_count<false>, dim3(blocks_for(work)), dim3(256), 0, s, st->slots, st->cap - 1, st->cnt, st->first,
                       d_tokens, (long long)n_tokens, (const long long *)d_text_offsets, (long long)n_texts, base, seq0, max_n,
                       st->d_counters, st->d_status, 0u, 1u);
  FIT_HIP(hipGetLastError());
  unsigned long long h_distinct = 0;
  FIT_HIP(hipMemcpyAsync(&h_distinct, st->d_counters, 8, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipMemcpyAsync(&h_status, st->d_status, 4, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipStreamSynchronize(s));
  st->n_distinct = h_distinct;
  st->n_occ += chunk_occ;
  if (seq0 + chunk_occ > st->next_seq) st->next_seq = seq0 + chunk_occ;
  if (h_status & SCONE_ST_INDEX_FULL) return SCONE_ENOMEM;  // cannot happen: the table is at most half full
  return SCONE_OK;
}

extern "C" int scone_fit_update(scone_fit_state *st, const int32_t *d_tokens, int64_t n_tokens, const int64_t *d_text_offsets,
                                int64_t n_texts, uint64_t seq_base, scone_stream_t stream) {
  return fits_update(st, d_tokens, n_tokens, d_text_offsets, n_texts, seq_base, 0u, 1u, stream);
}

extern "C" int scone_fit_update_part(scone_fit_state *st, const int32_t *d_tokens, int64_t n_tokens,
                                     const int64_t *d_text_offsets, int64_t n_texts, uint64_t seq_base, uint32_t part,
                                     uint32_t n_parts, scone_stream_t stream) {
  if (!st || n_parts == 0 || part >= n_parts) return SCONE_EINVAL;  // before any device work
  return fits_update(st, d_tokens, n_tokens, d_text_offsets, n_texts, seq_base, part, n_parts, stream);
}

extern "C" int scone_fit_partition(const uint32_t *h_keys, const uint8_t *h_lens, uint64_t n, int32_t max_n, uint32_t n_parts,
                                   uint32_t *h_part_out) {
  if (max_n < 1 || max_n > SCONE_MAX_N || n_parts == 0) return SCONE_EINVAL;
  if (n == 0) return SCONE_OK;
  if (!h_keys || !h_lens || !h_part_out) return SCONE_EINVAL;
  // two passes: a refusal writes nothing
  for (int pass = 0; pass < 2; ++pass)
    for (uint64_t i = 0; i < n; ++i) {
      const int len = h_lens[i];
      if (len < 1 || len > max_n) return SCONE_EINVAL;
      uint32_t k[SCONE_MAX_N] = {0u, 0u, 0u, 0u};
      for (int j = 0; j < len; ++j) k[j] = h_keys[i * (uint64_t)max_n + j];
      const scone_key key = scone_pack_key(k, len, max_n);
      if (!key.ok) return SCONE_ERANGE;
      if (pass) h_part_out[i] = fits_part_of(scone_hash_key(key.lo, key.ext), n_parts);
    }
  return SCONE_OK;
}

static int fits_finalize(scone_fit_state *st, uint32_t min_freq, uint64_t max_f_grams, uint32_t *d_keys_out, uint8_t *d_lens_out,
                         uint64_t *d_counts_out, uint64_t *d_first_out, uint64_t out_cap, uint64_t *h_n_out,
                         scone_stream_t stream) {
  if (!st || !h_n_out) return SCONE_EINVAL;
  *h_n_out = 0;
  scone_device_guard dev_guard__(st->device);
  FIT_HIP(dev_guard__.err);
  hipStream_t s = (hipStream_t)stream;
  if (st->n_distinct == 0 || max_f_grams == 0 || out_cap == 0) return SCONE_OK;
  if (!d_keys_out || !d_lens_out) return SCONE_EINVAL;
  const unsigned long long cap = st->cap;
  unsigned long long *n_sel = st->d_counters + 1;

  // eligible entries (count >= min_freq); their number sizes every buffer below, so count first
  FIT_HIP(hipMemsetAsync(n_sel, 0, 8, s));
  hipLaunchKernelGGL(k_fits_eligible, dim3(blocks_for(cap)), dim3(256), 0, s, st->cnt, cap, (unsigned long long)min_freq, n_sel);
  FIT_HIP(hipGetLastError());
  unsigned long long m = 0;
  FIT_HIP(hipMemcpyAsync(&m, n_sel, 8, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipStreamSynchronize(s));
  if (m == 0) return SCONE_OK;

  dev_buf sel_first, sel_slot, k2, v2, c1, c2, tmp1, tmp2;
  FIT_HIP(sel_first.alloc(m * 8));
  FIT_HIP(sel_slot.alloc(m * 8));
  FIT_HIP(k2.alloc(m * 8));
  FIT_HIP(v2.alloc(m * 8));
  FIT_HIP(c1.alloc(m * 8));
  FIT_HIP(c2.alloc(m * 8));
  FIT_HIP(hipMemsetAsync(n_sel, 0, 8, s));
  hipLaunchKernelGGL(k_fits_compact, dim3(blocks_for(cap)), dim3(256), 0, s, st->cnt, st->first, cap, (unsigned long long)min_freq,
                     m, n_sel, sel_first.as<unsigned long long>(), sel_slot.as<unsigned long long>());
  FIT_HIP(hipGetLastError());

  // (1) stable sort by first sequence number ascending, (2) stable sort by the 64-bit count descending
  size_t need = 0;
  FIT_HIP(rocprim::radix_sort_pairs(nullptr, need, sel_first.as<unsigned long long>(), k2.as<unsigned long long>(),
                                    sel_slot.as<unsigned long long>(), v2.as<unsigned long long>(), (size_t)m, 0, 64, s));
  FIT_HIP(tmp1.alloc(need));
  FIT_HIP(rocprim::radix_sort_pairs(tmp1.p, need, sel_first.as<unsigned long long>(), k2.as<unsigned long long>(),
                                    sel_slot.as<unsigned long long>(), v2.as<unsigned long long>(), (size_t)m, 0, 64, s));
  hipLaunchKernelGGL(k_fits_gather_counts, dim3(blocks_for(m)), dim3(256), 0, s, st->cnt, v2.as<unsigned long long>(), m,
                     c1.as<unsigned long long>());
  FIT_HIP(hipGetLastError());
  size_t need2 = 0;
  FIT_HIP(rocprim::radix_sort_pairs_desc(nullptr, need2, c1.as<unsigned long long>(), c2.as<unsigned long long>(),
                                         v2.as<unsigned long long>(), sel_slot.as<unsigned long long>(), (size_t)m, 0, 64, s));
  FIT_HIP(tmp2.alloc(need2));
  FIT_HIP(rocprim::radix_sort_pairs_desc(tmp2.p, need2, c1.as<unsigned long long>(), c2.as<unsigned long long>(),
                                         v2.as<unsigned long long>(), sel_slot.as<unsigned long long>(), (size_t)m, 0, 64, s));

  unsigned long long n_out = m < max_f_grams ? m : max_f_grams;
  if (n_out > out_cap) n_out = out_cap;
  hipLaunchKernelGGL(k_fits_emit, dim3(blocks_for(n_out)), dim3(256), 0, s, st->slots, st->first, sel_slot.as<unsigned long long>(),
                     c2.as<unsigned long long>(), n_out, st->max_n, d_keys_out, d_lens_out, (unsigned long long *)d_counts_out,
                     (unsigned long long *)d_first_out);
  FIT_HIP(hipGetLastError());
  FIT_HIP(hipStreamSynchronize(s));
  *h_n_out = n_out;
  return SCONE_OK;
}

extern "C" int scone_fit_finalize(scone_fit_state *st, uint32_t min_freq, uint64_t max_f_grams, uint32_t *d_keys_out,
                                  uint8_t *d_lens_out, uint64_t *d_counts_out, uint64_t out_cap, uint64_t *h_n_out,
                                  scone_stream_t stream) {
  return fits_finalize(st, min_freq, max_f_grams, d_keys_out, d_lens_out, d_counts_out, nullptr, out_cap, h_n_out, stream);
}

extern "C" int scone_fit_finalize_seq(scone_fit_state *st, uint32_t min_freq, uint64_t max_f_grams, uint32_t *d_keys_out,
                                      uint8_t *d_lens_out, uint64_t *d_counts_out, uint64_t *d_first_out, uint64_t out_cap,
                                      uint64_t *h_n_out, scone_stream_t stream) {
  return fits_finalize(st, min_freq, max_f_grams, d_keys_out, d_lens_out, d_counts_out, d_first_out, out_cap, h_n_out, stream);
}

extern "C" int scone_fit_export(scone_fit_state *st, uint32_t *d_keys_out, uint8_t *d_lens_out, uint64_t *d_counts_out,
                                uint64_t *d_first_out, uint64_t out_cap, uint64_t *h_n_out, scone_stream_t stream) {
  if (!st || !h_n_out) return SCONE_EINVAL;
  *h_n_out = st->n_distinct;
  if (out_cap < st->n_distinct) return SCONE_ERANGE;
  if (st->n_distinct == 0) return SCONE_OK;
  if (!d_keys_out || !d_lens_out || !d_counts_out || !d_first_out) return SCONE_EINVAL;
  scone_device_guard dev_guard__(st->device);
  FIT_HIP(dev_guard__.err);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *n_out = st->d_counters + 1;
  FIT_HIP(hipMemsetAsync(n_out, 0, 8, s));
  hipLaunchKernelGGL(k_fits_export, dim3(blocks_for(st->cap)), dim3(256), 0, s, st->slots, st->cnt, st->first, st->cap, st->max_n,
                     (unsigned long long)out_cap, n_out, d_keys_out, d_lens_out, (unsigned long long *)d_counts_out,
                     (unsigned long long *)d_first_out);
  FIT_HIP(hipGetLastError());
  FIT_HIP(hipStreamSynchronize(s));
  return SCONE_OK;
}

extern "C" int scone_fit_merge(scone_fit_state *st, const uint32_t *d_keys, const uint8_t *d_lens, const uint64_t *d_counts,
                               const uint64_t *d_first, uint64_t n, scone_stream_t stream) {
  if (!st) return SCONE_EINVAL;
  if (n == 0) return SCONE_OK;
  if (!d_keys || !d_lens || !d_counts || !d_first) return SCONE_EINVAL;
  scone_device_guard dev_guard__(st->device);
  FIT_HIP(dev_guard__.err);
  hipStream_t s = (hipStream_t)stream;

  FIT_HIP(hipMemsetAsync(st->d_status, 0, 4, s));
  hipLaunchKernelGGL(k_fits_merge_validate, dim3(blocks_for(n)), dim3(256), 0, s, d_keys, d_lens, (unsigned long long)n, st->max_n,
                     st->d_status);
  FIT_HIP(hipGetLastError());
  uint32_t h_status = 0;
  FIT_HIP(hipMemcpyAsync(&h_status, st->d_status, 4, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipStreamSynchronize(s));
  if (h_status & FIT_ST_BAD_LEN) return SCONE_EINVAL;
  if (h_status & SCONE_ST_BAD_TOKEN) return SCONE_ERANGE;

  const int rc_g = fits_grow(st, st->n_distinct + n, s);
  if (rc_g != SCONE_OK) return rc_g;

  hipLaunchKernelGGL(k_fits_merge, dim3(blocks_for(n)), dim3(256), 0, s, st->slots, st->cap - 1, st->cnt, st->first, d_keys, d_lens,
                     (const unsigned long long *)d_counts, (const unsigned long long *)d_first, (unsigned long long)n, st->max_n,
                     st->d_counters, st->d_status);
  FIT_HIP(hipGetLastError());
  unsigned long long h_distinct = 0;
  FIT_HIP(hipMemcpyAsync(&h_distinct, st->d_counters, 8, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipMemcpyAsync(&h_status, st->d_status, 4, hipMemcpyDeviceToHost, s));
  FIT_HIP(hipStreamSynchronize(s));
  st->n_distinct = h_distinct;
  if (h_status & SCONE_ST_INDEX_FULL) return SCONE_ENOMEM;  // cannot happen: the table is at most half full
  return SCONE_OK;
}
