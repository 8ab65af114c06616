/*
 * scone_hip.h -- C ABI of libscone_hip.so: the MI355X (gfx950) f-gram embedding
 * lookup / aggregation path.
 *
 * The reference (llmsresearch/scone) is pure Python and has no FFI of its own.
 * Each entry point below names the reference code it replaces (file:line under
 * the reference checkout); INTEGRATION.md shows the ctypes stub a maintainer
 * would add on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross this boundary
 *   - every function returns 0 (SCONE_OK) or a negative errno-style code and
 *     never throws; scone_last_error(h) holds a human-readable message
 *   - the caller owns every buffer it passes; the library owns the index, the
 *     table and its workspaces
 *   - "d_" pointers are device pointers on the handle's device, "h_" pointers
 *     are host pointers; all device work is enqueued on the given stream
 *     (hipStream_t passed as void*; NULL = the default stream) and the call
 *     returns without synchronising unless documented otherwise
 *   - index and table are immutable on the lookup path, and lookups are thread-safe and stream-ordered: scone_embed
 *     (any batch size), scone_match, scone_match_csr, scone_gather_reduce, scone_embed_partial, scone_finalize and
 *     scone_table_gather_rows may be called concurrently from several host threads on one handle, on the same or on
 *     different streams.  Batches of up to 32768 tokens at d = 768 / 1024 / 1280 take one launch and no workspace; larger
 *     ones use a workspace that belongs to the STREAM of the call (created on first use, grown on demand or by
 *     scone_reserve) and is locked while the call enqueues its kernels.  Lookups and scone_embed_prefetch on a table
 *     created with stage_tokens > 0 share ONE staging pipeline per handle: they may be called from several threads, and are
 *     serialised on a lock of the handle for the length of the call (host side; their device work follows each other through
 *     the pipeline's events).  Not concurrent on one handle: index / table mutation against lookups, the scone_shard_*
 *     exchange calls, and scone_destroy against anything
 *   - every entry point selects the handle's device and restores the caller's current device before it returns
 */
#ifndef SCONE_HIP_H
#define SCONE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCONE_ABI_VERSION 2

typedef struct scone_handle scone_handle;
typedef void *scone_stream_t; /* hipStream_t */

/* table row formats (defined by this library; the reference's cache is always
 * fp32, scone/inference/embedding_cache.py:86,134,139) */
enum {
  SCONE_FMT_F32 = 0, /* [N,d] float                                     row_bytes 4d      */
  SCONE_FMT_F16 = 1, /* [N,d] IEEE half                                 row_bytes 2d      */
  SCONE_FMT_I8 = 2,  /* [N,d] int8 + scales[N] half (per row)           row_bytes d+2     */
  SCONE_FMT_I4 = 3,  /* [N,d/2] offset-binary nibbles (elem 2k = low)   row_bytes d/2+2*d/128
                        + scales[N,d/128] half (per 128-group)                            */
  SCONE_FMT_BF16 = 4,/* [N,d] bfloat16 (the upper half of the fp32), no scales, d % 8 == 0   row_bytes 2d
                        fp32 rows are stored with IEEE round-to-nearest-even (NaN stays a quiet NaN); a row reads
                        back as bits << 16, so every lookup equals the fp32 lookup of the dequantised table
                        bit for bit.  Appended: the values above and SCONE_ABI_VERSION are unchanged.   */
  SCONE_FMT_MXFP4 = 5 /* OCP microscaling MXFP4, d % 128 == 0                              row_bytes d/2+d/32
                        [N,d/2] E2M1 nibbles (elem 2k = low nibble of byte k, the order of INT4 here and of torch's
                        float4_e2m1fn_x2): s m2 m1 m0, magnitude codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6, bit 3 the sign, no
                        inf / NaN code, 0x8 is -0
                        + scales[N,d/32] uint8 E8M0, one per 32 consecutive elements, logical order in upload / download:
                        X in 0..254 means 2^(X-127) (X = 0: the fp32 subnormal 2^-127), X = 255 makes the block NaN.
                        value = fp32(elem) * fp32(2^(X-127)), ONE IEEE fp32 product: exact for every (code, X) but the
                        large codes at X >= 253, which overflow to +-inf.  Rows are summed as acc += value, so every
                        lookup equals the fp32 lookup of the dequantised table bit for bit.
                        fp32 rows are stored block by block by the OCP MX v1.0 rule: a block with a NaN or +-inf gets
                        X = 255 (nibbles: the sign bits); else amax = max|v|, amax == 0 -> X = 127 and signed zeros, else
                        X = clamp(floor(log2(amax)) - 2 + 127, 0, 254), and each v / 2^(X-127) goes to the nearest E2M1
                        magnitude, ties to the even code, above 6 to 6, sign kept (|v - dq(v)| <= amax / 4).
                        Appended: the values above and SCONE_ABI_VERSION are unchanged.   */
};
enum {
  SCONE_PLACE_HBM = 0,        /* rows in device memory                                              */
  SCONE_PLACE_PINNED_HOST = 1 /* rows >= cfg.hot_rows in pinned host DRAM mapped into the GPU, read over PCIe */
};
enum { SCONE_REDUCE_MEAN = 0, SCONE_REDUCE_SUM = 1 };
enum {
  SCONE_MODE_COVER = 0,         /* the reference CODE: every f-gram covering the token, aggregated and ADDED to
                                   the token embedding (n_gram_extractor.py:106-126, engine.py:250,
                                   language_model.py:242-243)                                             */
  SCONE_MODE_LONGEST_SUFFIX = 1 /* the PAPER (Algorithm 2, assets/algorithm.png): the longest f-gram of length
                                   >= 2 ENDING at the token REPLACES the token embedding; causal           */
};
enum { SCONE_DT_F32 = 0, SCONE_DT_F16 = 1, SCONE_DT_BF16 = 2 };

enum {
  SCONE_OK = 0,
  SCONE_ESTATE = -1,  /* call order / missing index or table            */
  SCONE_EHIP = -5,    /* a HIP runtime call failed                      */
  SCONE_ENOMEM = -12, /* allocation failed / index full                 */
  SCONE_ENODEV = -19, /* no usable GPU                                  */
  SCONE_EINVAL = -22, /* bad argument                                   */
  SCONE_ERANGE = -34  /* id / token / row outside the configured range  */
};

typedef struct scone_cfg {
  uint32_t struct_size;    /* = sizeof(scone_cfg)                                          */
  int32_t device;          /* HIP device ordinal                                           */
  int32_t max_n;           /* longest f-gram, 1..4 (NGramExtractor.max_n,
                              scone/tokenization/n_gram_extractor.py:39)                    */
  int32_t dim;             /* embedding_dim d (EmbeddingCache.embedding_dim, :45);
                              multiple of 4 (F32), 8 (F16), 16 (I8), 128 (I4); 0 = index only.
                              There is no upper bound: rows of ANY width that the format's rule allows are
                              supported on every road (quantiser, lookups, lists, row shards and their
                              exchanges, pinned host memory read in place and through the cache of cold
                              rows).  The widest the suite checks is d = 16384 (F32 and I4; I8, F16 and
                              MXFP4 at 8192: tests/test_gpu_wide_rows.py).  Whatever the format,
                              SCONE_MODE_LONGEST_SUFFIX, scone_embed_varlen, scone_embed_base_varlen and
                              scone_embed_select need d % 8 == 0 (stated again at those calls)          */
  int32_t table_fmt;       /* SCONE_FMT_*                                                  */
  int32_t placement;       /* SCONE_PLACE_*                                                */
  uint64_t n_rows;         /* N = number of f-grams (global)                               */
  uint64_t row_begin;      /* rows owned by this handle: [row_begin, row_end); the whole   */
  uint64_t row_end;        /* table is 0..N (row_end = 0 means N)                          */
  uint64_t index_capacity; /* hash slots (power of two >= 4); 0 = smallest power of two >= 2*N */
  uint64_t hot_rows;       /* SCONE_PLACE_PINNED_HOST only: global rows [0, hot_rows) stay in HBM, the
                              rest in pinned host DRAM.  f-gram ids are frequency-ordered
                              (Counter.most_common, n_gram_extractor.py:91-99), so the head of
                              the table takes most of the hits.                              */
  uint32_t lookup_mode;    /* SCONE_MODE_* for scone_embed / scone_embed_partial / scone_finalize           */
  uint32_t stage_tokens;   /* SCONE_PLACE_PINNED_HOST only.  0: the lookup kernel reads host rows in place over
                              PCIe.  > 0: prefetch through an HBM cache of cold rows -- the batch is processed in
                              chunks of about this many tokens; on side streams each chunk is matched, the cold rows
                              it references that are not cached take a cache slot (clock eviction) and are copied
                              host -> HBM once, while the previous chunk is reduced on the caller's stream out of
                              [hot head | cache].  The cache lives as long as the table: a row stays resident across
                              chunks, batches and calls until it is evicted (the reference's analogue: the page cache
                              under its memory-mapped table, embedding_cache.py:76-91,132-135)                  */
  uint64_t cache_rows;     /* stage_tokens > 0: row slots of that cache (payload + scale bytes of HBM each).  At least
                              what the pipeline needs -- 7 chunks' worst case (5 record sets in the ring + the chunk being
                              placed + one of slack), 42 x stage_tokens rows for max_n = 3: 11.0M rows = 5.8 GB of INT4
                              d = 1024 rows at stage_tokens = 262144 -- is always provisioned (0 = exactly that); never
                              more than the cold rows                                                              */
} scone_cfg;

/* ---- lifecycle ----------------------------------------------------------- */
int scone_abi_version(void);
const char *scone_strerror(int code);
/* Allocates the (empty) index and, when cfg->dim > 0, the table storage. */
int scone_create(const scone_cfg *cfg, scone_handle **out);
void scone_destroy(scone_handle *h);
const char *scone_last_error(const scone_handle *h);
/* Sticky device-side status bits raised by kernels (bit 0, SCONE_ST_BAD_TOKEN: a token id outside [0, vocab) of a given d_wte
 * or a position id -- the caller's or the default one -- outside [0, n_pos) of a given d_wpe, see "Ids out of range" at
 * scone_embed; also a scone_embed_select position outside the batch, bit 1: f-gram id outside the table, bit 2: index
 * full, bit 3: the cache of cold rows of a pinned-host lookup had no evictable slot for a row -- sized so that it cannot
 * happen; the affected tokens read a wrong row, bit 4: scone_backward_rows_dn found more rows in its plan than rows_cap and
 * wrote none, *d_n_out = 0); synchronises the stream, returns the bits in *bits and clears them. */
int scone_status(scone_handle *h, uint32_t *bits, scone_stream_t stream);
/* The cache of cold rows of a pinned-host table (cfg.stage_tokens > 0): its row slots, the rows copied host -> HBM since the
 * cache was created (every miss crosses PCIe once), the chunks prepared and the tokens per chunk actually used (smaller than
 * cfg.stage_tokens when the cache is small).  All zero before the first lookup.  Synchronises the device. */
int scone_stage_counters(scone_handle *h, uint64_t *cache_rows, uint64_t *rows_copied, uint64_t *chunks, uint64_t *chunk_tokens);

/* ---- index: f-gram -> id (replaces NGramExtractor.f_grams / f_gram_to_id,
 *      n_gram_extractor.py:42-44, and the id map of embedding_cache.py:173) --- */
/* keys[n, max_n] uint32 token ids (first lens[i] used), lens[n] in 1..max_n;
 * key i gets id = id0 + i.  May be called repeatedly.  On a duplicate key the
 * smallest id wins.  Host-pointer variant copies through a staging buffer and
 * synchronises; the device variant is stream-ordered. */
int scone_index_build(scone_handle *h, const uint32_t *h_keys, const uint8_t *h_lens,
                      uint64_t n, uint64_t id0);
int scone_index_build_device(scone_handle *h, const uint32_t *d_keys, const uint8_t *d_lens,
                             uint64_t n, uint64_t id0, scone_stream_t stream);
/* Synchronises.  n_keys = distinct keys stored, n_dups = duplicate insertions seen. */
int scone_index_stats(scone_handle *h, uint64_t *n_keys, uint64_t *capacity, uint64_t *n_dups);

/* The built index as three host blobs -- hash slots, direct unigram table, presence bitmap -- so that a table file can
 * carry it (scone_amd's native file: EmbeddingCache.save_native(with_index=True)) and a shard of a 1e9-key table loads
 * without rebuilding it from the keys.  Import needs a handle created with the same max_n and index_capacity (compare
 * scone_index_blob_sizes) and replaces the index; both synchronise the device. */
int scone_index_blob_sizes(scone_handle *h, uint64_t *slot_bytes, uint64_t *uni_bytes, uint64_t *bloom_bytes);
int scone_index_export(scone_handle *h, void *h_slots, void *h_uni, void *h_bloom, uint64_t *n_keys);
int scone_index_import(scone_handle *h, const void *h_slots, const void *h_uni, const void *h_bloom, uint64_t n_keys);

/* ---- vocabulary construction on the GPU (NGramExtractor.fit, n_gram_extractor.py:72-104) -----
 * d_tokens[n_tokens] int32: the corpus, texts back to back; d_text_offsets[n_texts+1] int64.
 * Counts every n-gram (n = 1..max_n, windows inside one text), keeps those with
 * count >= min_freq, orders them by count descending with ties in first-insertion order
 * (Counter.most_common: texts in order; per text all 1-grams, then all 2-grams, ...;
 * extract_all_n_grams :59-70) and writes the first min(max_f_grams, out_cap) as
 * d_keys_out[*, max_n] / d_lens_out[*] (/ d_counts_out[*], optional): row r is f-gram id r.
 * *h_n_out = rows written, *h_n_distinct = distinct n-grams seen (optional).  Synchronises. */
int scone_fit(int32_t device, const int32_t *d_tokens, int64_t n_tokens, const int64_t *d_text_offsets,
              int64_t n_texts, int32_t max_n, uint32_t min_freq, uint64_t max_f_grams,
              uint32_t *d_keys_out, uint8_t *d_lens_out, uint32_t *d_counts_out, uint64_t out_cap,
              uint64_t *h_n_out, uint64_t *h_n_distinct, scone_stream_t stream);

/* The same fit as a counter that is fed in chunks (what Counter.update gives the reference's fit loop, n_gram_extractor.py:72-104,
 * with extract_all_n_grams :59-70 fixing the insertion order): a persistent state on the device that grows with the DISTINCT
 * n-grams seen, can be finalised any number of times, exported and merged.  For every chunking, growth history, shard order and
 * merge order the f-gram list equals scone_fit's on the whole corpus: same keys, same ids, same counts.  The state is an
 * exact-key table (the packing and hash of the lookup index) with a 64-bit count and a 64-bit first sequence number per slot,
 * 32 B per slot; counts never wrap.  No handle and no error string: return codes only, as scone_fit.  Every call selects the
 * state's device and restores the caller's.  One state is used by one host thread at a time; states are independent.
 * scone_fit_create: max_n in 1..4; initial_slots = 0 means 1024, any other value is rounded up to a power of two >= 1024.
 * SCONE_EINVAL for a bad max_n / device or a null out, before any device work.  scone_fit_destroy(NULL) is a no-op. */
typedef struct scone_fit_state scone_fit_state;
int scone_fit_create(int32_t device, int32_t max_n, uint64_t initial_slots, scone_fit_state **out);
void scone_fit_destroy(scone_fit_state *st);
/* Counts one chunk of WHOLE texts (a text never spans two calls); layout as scone_fit: d_tokens[n_tokens] int32 back to back,
 * d_text_offsets[n_texts + 1] int64 starting at 0.  Occurrences are numbered as scone_fit numbers them (texts in order; inside a
 * text all 1-grams left to right, then all 2-grams, ...; extract_all_n_grams :59-70), starting at seq_base for the chunk's first
 * text.  seq_base = UINT64_MAX continues where the previous chunk ended (next_seq); any other value is the caller's global number
 * of this chunk's first occurrence, so that shards may be counted out of order or on other devices.  Afterwards
 * next_seq = max(next_seq, seq_base + occurrences of the chunk).  n_texts = 0 or n_tokens = 0 is a no-op.
 * The chunk is validated by a pass of its own BEFORE anything is counted, and a refused call leaves the state exactly as it
 * was: SCONE_ERANGE for a negative token or one the key packing cannot hold (max_n = 4: >= 2^24 - 1); SCONE_EINVAL for offsets
 * that do not start at 0, decrease, or do not end at n_tokens, for a null state, and for null arrays with non-zero sizes.
 * Growth comes before the count, never inside it: with need = n_distinct + occurrences of the chunk, a table of fewer than
 * 2 * need slots is moved to the smallest power of two >= 2 * need (old and new arrays coexist during the move; a failed
 * allocation returns SCONE_ENOMEM with the old table intact), so slots < 4 * max(512, need) at every moment.
 * Synchronises the stream (twice: it reads the validation status and the chunk's occurrence count, then the distinct counter). */
int scone_fit_update(scone_fit_state *st, const int32_t *d_tokens, int64_t n_tokens, const int64_t *d_text_offsets,
                     int64_t n_texts, uint64_t seq_base, scone_stream_t stream);
/* Host mirrors, exact after every call (none is left in flight): distinct n-grams held, occurrences FED to scone_fit_update /
 * scone_fit_update_part (every occurrence of every accepted chunk, whether its key was in the call's partition or not; merged
 * counts are not added), slots of the table (x 32 B = its device memory), growth events, next_seq.  Any output may be
 * NULL.  No device work. */
int scone_fit_stats(scone_fit_state *st, uint64_t *n_distinct, uint64_t *n_occurrences, uint64_t *slots, uint64_t *n_grows,
                    uint64_t *next_seq);
/* The f-gram list of everything counted so far, in scone_fit's order (count descending, ties by first sequence number ascending =
 * Counter.most_common, n_gram_extractor.py:91-99): entries with count >= min_freq (and >= 1), two stable radix sorts, the count key
 * 64 bits wide.  Row r of d_keys_out[*, max_n] / d_lens_out[*] / d_counts_out[*] (uint64, optional) is f-gram id r;
 * *h_n_out = min(eligible, max_f_grams, out_cap) rows are written.  Does NOT consume the state: call it again with other
 * min_freq / max_f_grams, or go on updating.  Scratch is sized by the eligible entries (48 B each + the sorts' workspace).
 * Synchronises the stream. */
int scone_fit_finalize(scone_fit_state *st, uint32_t min_freq, uint64_t max_f_grams, uint32_t *d_keys_out, uint8_t *d_lens_out,
                       uint64_t *d_counts_out, uint64_t out_cap, uint64_t *h_n_out, scone_stream_t stream);
/* Export: every distinct entry as d_keys_out[*, max_n] / d_lens_out / d_counts_out (64-bit) / d_first_out (first sequence number),
 * in no particular order; *h_n_out = n_distinct.  out_cap < n_distinct returns SCONE_ERANGE with the needed number in *h_n_out
 * and writes nothing.  Merge: adds n such entries to a state, count += d_counts[i], first = min(first, d_first[i]); the same key
 * may occur more than once.  All entries are validated before any is applied: a length outside 1..max_n returns SCONE_EINVAL, a
 * token the key packing cannot hold SCONE_ERANGE, and the state is unchanged.  Merge grows like an update, with
 * need = n_distinct + n, and leaves next_seq alone (the caller passes an explicit seq_base to later updates).  Shards counted
 * separately with explicit seq_base and merged in any order give the state that counting the corpus in order gives; export +
 * merge is also checkpoint and resume.  Both synchronise the stream. */
int scone_fit_export(scone_fit_state *st, uint32_t *d_keys_out, uint8_t *d_lens_out, uint64_t *d_counts_out,
                     uint64_t *d_first_out, uint64_t out_cap, uint64_t *h_n_out, scone_stream_t stream);
int scone_fit_merge(scone_fit_state *st, const uint32_t *d_keys, const uint8_t *d_lens, const uint64_t *d_counts,
                    const uint64_t *d_first, uint64_t n, scone_stream_t stream);

/* Exact fit beyond one device's memory: key-hash partitions.  The key space is cut into n_parts parts by a hash of the key, and
 * a pass over the corpus counts the keys of ONE part; the state then holds about 1 / n_parts of the distinct n-grams, at the
 * price of n_parts passes (or n_parts devices, one part each, nothing exchanged).
 *
 * The partition function is a contract -- selections written by one process are routed by another.  With
 * (lo, ext) = scone_pack_key(tokens, len, max_n), the packed key of the index (tokens stored + 1; max_n <= 3: 32 bits per
 * token, lo = t0 | t1 << 32, ext = t2; max_n = 4: 24 bits per token, lo = t0 | t1 << 24 | (t2 & 0xFFFF) << 48,
 * ext = t2 >> 16 | t3 << 8), and scone_hash_key(lo, ext) the index's 64-bit hash (x = lo ^ ext * 0x9E3779B97F4A7C15;
 * x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31):
 *
 *     part = (uint32_t)(((scone_hash_key(lo, ext) >> 32) * (uint64_t)n_parts) >> 32)
 *
 * It is taken from the UPPER 32 bits of the hash on purpose: the table picks a key's home slot from the LOWER bits,
 * hash & (slots - 1).  A partition taken from the lower bits would put a part's keys on 1 / n_parts of the home slots and
 * turn probing into long clusters.
 *
 * Why it is exact: every key lives in exactly one part, so its count and its first sequence number are complete inside that
 * part.  A key among the global top max_f_grams (count descending, first number ascending) has fewer than max_f_grams keys in
 * front of it globally, hence fewer in its own part: it is in its part's top max_f_grams.  So each part is finalised on its
 * own (scone_fit_finalize_seq), and merging the selections of all parts into a fresh state (scone_fit_merge) and finalising
 * that gives scone_fit's list: same keys, same ids, same counts.
 *
 * scone_fit_partition: pure host, no device work.  h_keys[n, max_n] / h_lens[n] as scone_index_build takes them;
 * h_part_out[n] receives each key's part.  SCONE_EINVAL: max_n outside 1..4, n_parts == 0, a length outside 1..max_n, null
 * arrays with n > 0.  SCONE_ERANGE: a token the key packing cannot hold (max_n = 4: >= 2^24 - 1).  On a refusal nothing is
 * written. */
int scone_fit_partition(const uint32_t *h_keys, const uint8_t *h_lens, uint64_t n, int32_t max_n, uint32_t n_parts,
                        uint32_t *h_part_out);
/* scone_fit_update in every respect but one: only occurrences whose key has partition `part` of `n_parts` are counted; a key
 * of another part never takes a slot.  Unchanged: the validation pass comes first and a refused call leaves the state as it
 * was; growth comes before the count with need = n_distinct + ALL occurrences of the chunk (an upper bound, so no growth
 * inside a count and every probe loop ends); EVERY occurrence of the chunk is numbered whether it is counted or not, and
 * next_seq and n_occurrences advance by all of them, so every part of one corpus ends at the same next_seq.
 * part >= n_parts or n_parts == 0 returns SCONE_EINVAL before any device work.  (part = 0, n_parts = 1) is scone_fit_update.
 * The state does not remember partitions: it stays a function of the multiset of (key, sequence number) pairs it was fed, and
 * feeding several parts to one state is legal (all n_parts parts of a chunk, each with the chunk's seq_base = scone_fit_update).
 * Memory per part: slots < 4 * max(512, distinct keys of the part + occurrences of one chunk). */
int scone_fit_update_part(scone_fit_state *st, const int32_t *d_tokens, int64_t n_tokens, const int64_t *d_text_offsets,
                          int64_t n_texts, uint64_t seq_base, uint32_t part, uint32_t n_parts, scone_stream_t stream);
/* scone_fit_finalize's list, row for row, plus the first sequence number of every row in d_first_out[*] (uint64): what
 * scone_fit_merge takes, so a part's selection is directly mergeable (scone_fit_export carries first numbers too, but of every
 * distinct entry).  d_counts_out and d_first_out may each be NULL.  Does not consume the state.  Synchronises the stream. */
int scone_fit_finalize_seq(scone_fit_state *st, uint32_t min_freq, uint64_t max_f_grams, uint32_t *d_keys_out, uint8_t *d_lens_out,
                           uint64_t *d_counts_out, uint64_t *d_first_out, uint64_t out_cap, uint64_t *h_n_out,
                           scone_stream_t stream);

/* ---- table: rows (replaces EmbeddingCache.cache_embeddings storage,
 *      embedding_cache.py:56-111) ------------------------------------------- */
/* Raw rows already in the handle's format.  rows: nrows * payload bytes
 * (4d / 2d / d / d/2); scales: NULL (F32,F16), half[nrows] (I8), half[nrows, d/128] (I4).
 * src_is_device selects host or device source pointers.  Rows are global ids and must
 * lie inside [row_begin,row_end). */
int scone_table_upload(scone_handle *h, const void *rows, const void *scales, uint64_t row0,
                       uint64_t nrows, int src_is_device, scone_stream_t stream);
/* Inverse of scone_table_upload: raw payload rows (+ scales) of global rows [row0, row0+nrows)
 * in the handle's format, to host or device buffers; synchronises for host destinations.
 * With it a quantised table can be saved and reloaded without re-quantising. */
int scone_table_download(scone_handle *h, void *rows, void *scales, uint64_t row0, uint64_t nrows,
                         int dst_is_device, scone_stream_t stream);
/* fp32 rows on the device -> the handle's format (quantised on the GPU). */
int scone_table_store_f32(scone_handle *h, const float *d_rows_f32, uint64_t row0, uint64_t nrows,
                          scone_stream_t stream);
/* Scattered variant: row i of d_rows_f32 goes to global row d_ids[i]
 * (cache_embeddings(f_gram_ids, embeddings), embedding_cache.py:98-99,110-111). */
int scone_table_store_f32_ids(scone_handle *h, const float *d_rows_f32, const int64_t *d_ids,
                              uint64_t nrows, scone_stream_t stream);
/* Counter-based synthetic rows (bench / full-size tests); any row can be
 * recomputed on the host (oracle/ref_port.py synth_*).
 * SCONE_FMT_MXFP4 (restated in tests/mxfp4_fixture.py): with hash32 the lowbias32 finaliser and
 * base(c) = hash32((uint32)c + 0x9E3779B9 * (uint32)(c >> 32)) ^ seed, payload dword w of row g is
 * hash32(base(g) + w) -- the words INT4 gets -- and the scale byte of block b of row g is
 * E - 1 + (hash32(base(g * (d/32) + b) + 0x51ED27) >> 8) % 3, E = the exponent field of base_scale clamped to
 * [1, 253]: within +-1 of floor(log2(base_scale)) + 127. */
int scone_table_fill_synthetic(scone_handle *h, uint32_t seed, float base_scale,
                               scone_stream_t stream);
/* Row gather: out[i,:] = dequantised row d_ids[i] as fp32
 * (EmbeddingCache.get_embeddings, embedding_cache.py:113-147). */
int scone_table_gather_rows(scone_handle *h, const int64_t *d_ids, uint64_t n, float *d_out,
                            scone_stream_t stream);

/* ---- hot path ------------------------------------------------------------ */
/* Per-window membership + id (NGramExtractor.get_token_f_grams,
 * n_gram_extractor.py:106-126, one entry per (n, start)):
 * d_hits[(n-1)*B*T + b*T + i] = id of tok[b, i:i+n] or -1. */
int scone_match(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t *d_hits,
                scone_stream_t stream);
/* Per-position id lists in the reference's order (n ascending, start ascending,
 * duplicates kept) as CSR over the B*T positions: d_offsets[B*T+1] (int32),
 * d_ids[ids_cap] (int32).  Writes the total to *h_total after synchronising the
 * stream; returns SCONE_ERANGE (and a valid *h_total) if ids_cap is too small. */
int scone_match_csr(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T,
                    int32_t *d_offsets, int32_t *d_ids, int64_t ids_cap, int64_t *h_total,
                    scone_stream_t stream);
/* Aggregate precomputed id lists: out[t,:] = reduce_k dequant(row ids[offsets[t]+k])
 * (+ base[t,:] when d_base != NULL, same dtype as out); zeros where the list is
 * empty (engine.py:247-259). */
int scone_gather_reduce(scone_handle *h, const int32_t *d_offsets, const int32_t *d_ids,
                        int64_t ntok, const void *d_base, int32_t reduce, void *d_out,
                        int32_t out_dtype, scone_stream_t stream);
/* Fused match + gather + dequantise + reduce + combine
 * (n_gram_extractor.py:106-126 -> embedding_cache.py:113-181 -> engine.py:234-266 ->
 *  language_model.py:239-254 with the projection folded into the table):
 *   out[b,i,:] = cast( (wte[tok[b,i]] + reduce_k row_k) + wpe[pos[b,i]] )
 * d_wte / d_wpe: [vocab,d] / [n_pos,d] in out_dtype, or NULL (term omitted);
 * d_pos: int32 [B,T] or NULL (= arange(T), language_model.py:248-251).
 * Batches of up to 32768 tokens (environment SCONE_FUSED_MAX_TOKENS, read by scone_create) at d = 768 / 1024 / 1280
 * run as ONE launch without any workspace; larger ones use the id-record workspace of the call's stream (grown on first
 * use / by scone_reserve).
 * Stream-ordered, no hidden synchronisation -- with ONE exception: the FIRST lookup (or scone_embed_prefetch) of a pinned-host
 * table with cfg.stage_tokens > 0 on a given caller stream synchronises that stream once, for ~1 ms: the staging pipeline
 * chooses its two side streams among six candidates by MEASURED overlap with the caller's stream (HIP multiplexes streams onto a
 * few hardware queues; side streams that share the caller's queue would serialise the prefetch behind the lookups).
 * Ids out of range (a padded batch: -1, -100, == vocab) are defined, never read out of bounds.  For every position p:
 *   token term     wte[tok[p]] if 0 <= tok[p] < vocab, else a row of +0.0 (also when d_wte == NULL);
 *   position term  wpe[pos] if 0 <= pos < n_pos, else a row of +0.0 (also when d_wpe == NULL); pos is d_pos[p] or the default
 *                  (i, or p - cu[s] in a packed batch) -- default positions with T > n_pos are out of range from i = n_pos on;
 *   f-gram term    unchanged by either: the id list of the raw tokens.  A negative token matches nothing; a token >= vocab
 *                  still matches every f-gram that contains it (the index knows nothing of wte);
 *   out[p,:]       cast((token term + f-gram term) + position term) in fp32, rounded once, like every other row.  On a
 *                  SCONE_MODE_LONGEST_SUFFIX handle a matched f-gram replaces the token term, in or out of range;
 *   status         bit 0 (SCONE_ST_BAD_TOKEN) is raised if and only if some position OF THE CALL has an id out of range for a
 *                  table that was given (d_wte / d_wpe != NULL) -- in longest_suffix mode too, matched or not.  No other bit.
 * Every other row of the output is what it is without the bad id, and nothing outside the output rows is written.  The rule
 * holds for every lookup entry point below (scone_embed_varlen, scone_embed_base*, scone_embed_select, scone_finalize,
 * scone_shard_gather_embed*, scone_shard_cols_embed) and for every launch on a part of a batch (staged chunks, the packed
 * traversal, a sequence or token range): only the ids of the positions a call covers can raise the bit. */
int scone_embed(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, const void *d_wte,
                int64_t vocab, const void *d_wpe, int64_t n_pos, const int32_t *d_pos,
                int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream);
/* Packed variable-length batch (new here; the reference pads: batch_tokenize matches over the padded ids, so a pad id that
 * occurs in an f-gram changes the lists of the last max_n - 1 real tokens of every sequence -- f_gram_tokenizer.py calls
 * get_token_f_grams one sequence at a time, and that per-sequence result is what this call stands for).
 * d_tok[total_tokens] holds the sequences back to back; d_cu_seqlens[n_seqs + 1] (int32, on the device) is non-decreasing with
 * cu[0] = 0 and cu[n_seqs] = total_tokens; sequence s is [cu[s], cu[s+1]), empty sequences (repeated values) are allowed.
 * Token p of sequence s gets exactly what scone_embed gives it when sequence s is passed alone as B = 1, T = cu[s+1] - cu[s]:
 * the same id list in the reference's order, the same sequential fp32 sum, IEEE mean and (wte + fg) + wpe, in both lookup
 * modes and with the handle's row_begin / row_end ownership rule.  d_out: [total_tokens, d].  d_pos: int32 [total_tokens] or
 * NULL (= p - cu[s]).  The one-launch rule of scone_embed applies with total_tokens in place of B*T; larger batches use the
 * id-record and position workspaces of the call's stream (scone_reserve).  Stream-ordered, no hidden synchronisation:
 * total_tokens comes from the host.  total_tokens == 0 or n_seqs == 0: a no-op.
 * SCONE_EINVAL (scone_last_error names the reason): negative n_seqs / total_tokens, a null d_tok / d_cu_seqlens / d_out,
 * total_tokens > 2^31 - 1, a bad reduce / out_dtype, d % 8 != 0, a pinned-host table created with stage_tokens > 0 (its
 * staging pipeline chunks whole rectangular sequences; tables read in place from pinned host memory work).  The CONTENTS of d_cu_seqlens are the caller's contract and are not validated on the device;
 * whatever they are, no token outside d_tok[0, total_tokens) is read and nothing outside the total_tokens output rows written.
 * Token / position ids out of range: as scone_embed ("Ids out of range"), the default position being p - cu[s]. */
int scone_embed_varlen(scone_handle *h, const int32_t *d_tok, const int32_t *d_cu_seqlens, int32_t n_seqs,
                       int64_t total_tokens, const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos,
                       const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream);
/* Fused lookup onto a DENSE base (new here: the caller already holds its token embeddings -- the inputs_embeds of
 * language_model.py:239-243, a tensor-parallel or scaled wte, an adapter's output; replaces match_csr + gather_reduce(base),
 * five launches and a host synchronise, by the one or two launches of scone_embed):
 *   out[p,:] = cast( (base[p,:] + reduce_k row_k) + wpe[pos[p]] )
 * scone_embed / scone_embed_varlen with the per-position row d_base[p,:] where those use wte[tok[p]].  d_base: [B*T, d]
 * ([total_tokens, d]) in out_dtype, required.  The id lists, the sequential fp32 sum, the IEEE mean, zero-fill for K = 0, d_wpe
 * == NULL (term omitted), d_pos == NULL (default positions) and the row_begin / row_end ownership rule (owned rows only,
 * divisor = full K) are scone_embed's; on a SCONE_MODE_LONGEST_SUFFIX handle a matched f-gram REPLACES the base row, as it
 * replaces the wte row there.  Token ids serve the match only: there is no vocabulary bound, a negative token matches nothing,
 * and SCONE_ST_BAD_TOKEN is raised only for a position id outside [0, n_pos) (its term is a row of +0.0: "Ids out of
 * range" at scone_embed, without the token rule).  Same launches, workspaces and stream ordering
 * as scone_embed / scone_embed_varlen (no hidden synchronisation but the staged first-bind exception above); every road of
 * scone_embed takes a dense base (one launch, two kernels, any d % 8 == 0, the lane-group fallback for other dims, staged and
 * in-place pinned-host tables, the CU reserve).
 * In place: d_out == d_base is allowed and defined (a wavefront reads the words of row p in the lanes that store them, and no
 * other wavefront touches that row).  Any OTHER overlap of the two [n, d] ranges returns SCONE_EINVAL.
 * SCONE_EINVAL (scone_last_error names the reason): a null d_tok / d_base / d_out (/ d_cu_seqlens), negative sizes, a bad
 * reduce / out_dtype, d_wpe with n_pos <= 0, a partial overlap, and for the packed call what scone_embed_varlen refuses
 * (d % 8 != 0, stage_tokens > 0, total_tokens > 2^31 - 1).  B*T == 0 / total_tokens == 0: a no-op. */
int scone_embed_base(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, const void *d_base,
                     const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce,
                     void *d_out, int32_t out_dtype, scone_stream_t stream);
int scone_embed_base_varlen(scone_handle *h, const int32_t *d_tok, const int32_t *d_cu_seqlens, int32_t n_seqs,
                            int64_t total_tokens, const void *d_base, const void *d_wpe, int64_t n_pos,
                            const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype,
                            scone_stream_t stream);

/* ---- the fused lookup over a batch's LIVE rows (new here: the reference trains its f-gram embeddings with a separate model,
 * README.md:21-23, and only bakes them into a table for inference).  The forward dual of scone_backward_rows: the same fused
 * lookup, with the rows taken from the caller's compact array d_rows [n, dim] keyed by d_row_ids [n] -- the ascending distinct
 * ids scone_backward_row_ids / scone_backward_rows return for the batch -- and NOT from the handle's table, which is never read
 * (pinned-host and staged handles are accepted like any other).  An f-gram model's outputs for the f-grams a batch matches go
 * in; scone_backward_rows of the same plan gives the gradient of exactly this array.
 * Output bits: with every hit of the batch listed, bit for bit what scone_embed (d_wte / vocab), scone_embed_base (d_base) or
 * their _varlen forms give on a handle with the same index, max_n and lookup_mode whose F32 / F16 / BF16 table (the type
 * `dtype` names) holds d_rows[u] in row d_row_ids[u]: that entry's arithmetic, in every rule -- exact widening, the sequential
 * fp32 sum from +0.0f in the reference's list order, the IEEE mean for K >= 2, (base + fg) + wpe, one rounding to out_dtype, the
 * replaced base row of lookup_mode longest_suffix, "Ids out of range" for token and position ids.
 * Base rows: at most one of d_wte and d_base (both: SCONE_EINVAL; neither: the term is omitted).  d_base follows
 * scone_embed_base: [B * T, dim] (packed: [total_tokens, dim]) in out_dtype, d_out == d_base is the defined in-place call, any
 * other overlap of the two ranges returns SCONE_EINVAL.
 * An id that is not listed: a hit whose id is not among the live ids contributes a row of +0.0, K stays the full hit count and
 * SCONE_ST_BAD_ID is raised.  No address outside d_rows[0, n_live) is ever formed, whatever the list holds; a list that is not
 * ascending is outside the contract (which listed row a hit then reads is unspecified, but the read stays inside the array).
 * n_live = n, or min(*d_n, n) when d_n is given -- the count on the device (scone_backward_rows_dn's), read on the stream;
 * with n_live == 0 every hit is unlisted.
 * Stream contract: ordered on `stream`, no synchronisation; allocates only the stream's match workspace, as scone_embed does
 * above its one-launch limit; two launches at every batch size (the match, then the gather over the live rows: a wave
 * resolves the ids of a group of 8 or 4 consecutive tokens to slots with a lane-parallel lower-bound search, then walks the
 * group as the unit-walking lookup kernel does); there is no one-launch form.  The packed form adds a launch for the
 * remainder where scone_embed_varlen does.
 * B * T == 0 (packed: total_tokens == 0 or n_seqs == 0) returns SCONE_OK before `live` and the pointers are looked at.
 * SCONE_EINVAL (scone_last_error names the reason): a null live, d_tok or d_out, a null d_row_ids or d_rows with n > 0, a
 * d_rows that is not 16-byte aligned, a bad struct_size / dtype / out_dtype / reduce, n > 2^31 - 1, dim == 0 or dim % 8 != 0,
 * a handle that owns only part of the rows (row_begin != 0 or row_end != n_rows: the match records of a shard leave out the
 * other shards' hits), and the shape, wte / wpe and packed-batch refusals of scone_embed / scone_embed_varlen (negative sizes,
 * total_tokens > 2^31 - 1, a null d_cu_seqlens, d_wte with vocab <= 0, d_wpe with n_pos <= 0). */
typedef struct scone_live_rows {
  uint32_t struct_size;      /* sizeof(scone_live_rows) */
  int32_t dtype;             /* SCONE_DT_F32 / F16 / BF16: element type of d_rows */
  const int64_t *d_row_ids;  /* [n] ascending, distinct: what scone_backward_row_ids / scone_backward_rows return */
  const void *d_rows;        /* [n, dim] contiguous, 16-byte aligned; dim = the handle's */
  uint64_t n;                /* rows (capacity when d_n is given), <= 2^31 - 1 */
  const uint64_t *d_n;       /* NULL, or the count on the device: min(*d_n, n) rows are live, read on the stream */
} scone_live_rows;
int scone_embed_rows(scone_handle *h, const scone_live_rows *live, const int32_t *d_tok, int32_t B, int32_t T,
                     const void *d_wte, int64_t vocab, const void *d_base, const void *d_wpe, int64_t n_pos,
                     const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype, void *stream);
int scone_embed_rows_varlen(scone_handle *h, const scone_live_rows *live, const int32_t *d_tok, const int32_t *d_cu_seqlens,
                            int32_t n_seqs, int64_t total_tokens, const void *d_wte, int64_t vocab, const void *d_base,
                            const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce, void *d_out,
                            int32_t out_dtype, void *stream);

/* Pinned-host tables with a prefetch pipeline (cfg.stage_tokens > 0): start fetching for the NEXT batch now.  The first chunks
 * of (d_tok, B, T) are matched, their missing cold rows placed in the HBM cache and copied host -> HBM on the handle's side
 * streams, ordered behind `stream` (the stream on which the tokens are produced) -- or, tokens_ready != 0, behind nothing: the
 * tokens are complete (uploaded and synchronised earlier), and the prefetch may run BESIDE a lookup queued on `stream` just
 * before, which is the point of calling it early -- and the call returns.  The scone_embed of exactly that batch (same pointer
 * and shape; the tokens must not change in between; any stream) takes the prepared chunks over instead of starting its pipeline
 * cold: a loop that calls scone_embed_prefetch(next) right after scone_embed(current) never pays the pipeline fill.  One
 * announcement may be pending; one that is never used is dropped by the next call (the rows it cached stay cached).  Results are
 * bit-identical with and without the call.  Thread-safe like scone_embed (serialised on the handle's staging lock).
 * Any other handle (rows in HBM, or read in place): a no-op.  There the match of the next batch could run ahead; built and
 * measured in round 5 -- k_match_ell on a side stream beside the previous gather is 1-19 % SLOWER than match-then-gather on
 * one stream at every batch size (the gather holds every wave slot; profiles/r05b, r05c) -- and removed.
 * (The north-star's "async prefetch"; the reference's memory-mapped table has no counterpart -- embedding_cache.py:132-135
 * faults rows in on first use.) */
int scone_embed_prefetch(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t tokens_ready, scone_stream_t stream);
/* Every per-stream workspace of the handle (those that exist, the default stream's -- created here -- and any created
 * later) holds at least max_tokens tokens: nothing is allocated inside a timed region afterwards. */
int scone_reserve(scone_handle *h, int64_t max_tokens);
/* CU reserve (new here; the reference is a single-stream Python loop).  A large-batch lookup fills every wave slot of the
 * chip for the length of the kernel, so a kernel another stream launches meanwhile -- the send / recv channels of an RCCL
 * collective in the sharded step, a copy kernel -- only gets in where lookup workgroups retire.  With n_reserved > 0 (a
 * multiple of 8: one CU per XCD; 0 switches it off) the lookup kernels of scone_embed (batches above the one-launch limit),
 * scone_embed_partial and the scone_shard_*_embed* calls run on a stream of the handle whose CU mask leaves n_reserved
 * compute units free, ordered into the caller's stream by two events (everything queued on the caller's stream before the
 * call precedes the lookup, everything queued after follows it); their grids are sized for the remaining CUs.  The two
 * cross-stream events cost ~75 us per lookup on MI355X / ROCm 7.2 (measured, profiles/r04c): a caller that owns its loop
 * queues it on the masked stream itself -- scone_lookup_stream returns it (NULL without a reserve; it lives until the next
 * scone_set_cu_reserve / scone_destroy) -- and a lookup called on THAT stream is launched there directly, no events.  Not
 * concurrent with lookups on the same handle (like every table mutation); synchronises the previous masked stream. */
int scone_set_cu_reserve(scone_handle *h, int32_t n_reserved);
int scone_get_cu_reserve(scone_handle *h, int32_t *n_reserved, int32_t *n_cus);
int scone_lookup_stream(scone_handle *h, void **stream);
/* Do kernels queued on stream_b START while a kernel queued before them on stream_a is still running?  HIP multiplexes a
 * process's streams onto a few hardware queues (four by default); two streams that share a queue run one after the other, and
 * which streams share depends on how many streams the process created before (profiles/r06i).  A caller that builds its own
 * overlap around the lookup -- the split-phase exchange of a row-sharded table plans and packs on a side stream -- picks that
 * side stream among a few candidates with this probe (scone_amd.hip_backend.SconeTable.pick_side_stream); the staging
 * pipeline of a pinned-host table does the same internally.  An 80-us spinning kernel on stream_a, a time stamp on stream_b;
 * synchronises both streams; *overlap = 1 or 0.  (No counterpart in the reference: it has no streams.) */
int scone_streams_overlap(scone_handle *h, scone_stream_t stream_a, scone_stream_t stream_b, int32_t *overlap);
/* Optional timing of the gather/reduce kernel launched by scone_embed: while enabled, every
 * call brackets that kernel with HIP events on the launch stream (a ring of 1024 pairs).
 * scone_profile_read synchronises the device, returns the number of timed launches and
 * their summed duration in milliseconds since the last reset, and optionally resets. */
int scone_profile_enable(scone_handle *h, int enable);
int scone_profile_read(scone_handle *h, uint64_t *n_launches, double *total_ms, int reset);
/* The individual launch times (milliseconds, launch order) behind scone_profile_read's sum since the last reset:
 * writes min(*n, cap) of them to h_ms and the number available to *n (at most 65536 are kept).  Synchronises.
 * bench.py reports their min / median / max: the same binary runs this kernel 5-10 % apart from process to
 * process (placement of the big buffers), so a mean alone says little. */
int scone_profile_samples(scone_handle *h, float *h_ms, uint64_t cap, uint64_t *n);

/* ---- row-sharded tables (one handle per GPU; RCCL exchange is done by the
 *      caller between the two calls) ---------------------------------------- */
/* fp32 partial sums over the rows this handle owns + the full per-position hit
 * count (the index is replicated, so every rank knows K). */
int scone_embed_partial(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T,
                        float *d_partial, int32_t *d_counts, scone_stream_t stream);
/* out[t,:] = cast( (wte[tok[t]] + sum[t,:] / K_t) + wpe[pos[t]] ) for t in
 * [tok_begin, tok_end) of the flattened B*T positions; d_sum / d_counts / d_out
 * are indexed from tok_begin (slice-local), d_tok / d_pos are the full [B,T].
 * Token / position ids out of range: as scone_embed ("Ids out of range"); only the ids of [tok_begin, tok_end) are looked at. */
int scone_finalize(scone_handle *h, const float *d_sum, const int32_t *d_counts,
                   const int32_t *d_tok, int32_t B, int32_t T, int64_t tok_begin, int64_t tok_end,
                   const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos,
                   const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype,
                   scone_stream_t stream);

/* ---- row-sharded tables, row exchanges (preferred over the partial-sum pair above: the wire carries quantised rows -- 528 B
 *      for an INT4 d=1024 row instead of a 4096-B fp32 partial sum per token and rank -- each DISTINCT row once per
 *      destination, and the receiving rank reduces them in the reference's order, so results are bit-identical to the
 *      unsharded table).  Tokens and index are replicated, so both ends of a transfer derive what is sent; the caller only
 *      moves the buffers.  Two forms, built from the same plan / pack / embed primitives below: the all-gather form (every
 *      rank reduces the whole batch out of [replicated head | the distinct rows of all ranks]) and the slice exchange (rank r
 *      reduces slice r: sequences [r*ceil(B/world), (r+1)*ceil(B/world)); scone_shard_gather_plan_chunks with n_chunks = world
 *      and dedup_across_chunks = 0 lists, per destination, the distinct rows of mine its slice references; ONE
 *      all_to_all_single of records).  (The first form of the slice exchange -- one record per reference, scone_shard_plan /
 *      _pack / _embed -- was superseded in round 2 and removed in round 4 together with ABI version 1.) ------------------ */
int scone_shard_record_bytes(scone_handle *h, uint64_t *bytes);
/* Replicated head (optional; call once after scone_create, before rows are stored).  Global rows [0, n_head) are
 * kept on EVERY shard in addition to the rows it owns and never cross xGMI.  f-gram ids are frequency-ordered
 * (Counter.most_common, n_gram_extractor.py:91-99): the head holds every unigram and the most frequent f-grams,
 * i.e. about half of all row references (every token has its unigram), and without it the rank that owns the head
 * sends ten times what the others send.  scone_table_fill_synthetic fills the head as well;
 * scone_shard_head_store_f32 quantises fp32 rows into it exactly as scone_table_store_f32 does (rows must lie in
 * [0, n_head); every rank stores the same rows). */
int scone_shard_set_head(scone_handle *h, uint64_t n_head);
int scone_shard_head_store_f32(scone_handle *h, const float *d_rows_f32, uint64_t row0, uint64_t nrows,
                               scone_stream_t stream);

/* ---- row-sharded tables, all-gather form: EVERY rank ends up with the whole [B, T, d] output.  Gathering the rows the
 *      batch references costs a quarter of the bytes of gathering the finished 2 KB vectors, and here every DISTINCT row
 *      crosses once however many tokens reference it: scone_shard_gather_plan claims the distinct rows this shard owns
 *      (outside the replicated head) that the batch references and returns their number (synchronises);
 *      scone_shard_gather_pack writes one record [row payload | scales | row id] per claimed row; the caller all-gathers
 *      the record buffers of all ranks (any order); scone_shard_gather_embed indexes the records by row id and reduces
 *      the whole batch out of [replicated head | records] -- bit-identical to the unsharded table. -------------------- */
int scone_shard_gather_plan(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, uint64_t *h_n_records,
                            scone_stream_t stream);
int scone_shard_gather_pack(scone_handle *h, void *d_send_buf, scone_stream_t stream);
int scone_shard_gather_embed(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, const void *d_records,
                             uint64_t n_records, const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos,
                             const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream);
/* The same exchange cut into n_chunks (<= 64) runs of sequences (chunk c = sequences [c * ceil(B / n_chunks), ...)) so that
 * the all-gather of chunk c + 1 overlaps the reduction of chunk c:
 *   scone_shard_gather_plan_chunks   one match of the batch, one claim pass per chunk in chunk order.
 *                                    dedup_across_chunks = 1 (all-gather form): a row claimed by an earlier chunk is not
 *                                    claimed again.  dedup_across_chunks = 0 with n_chunks = world (slice exchange: chunk q =
 *                                    the sequences rank q finalises): every chunk lists each DISTINCT row of mine it
 *                                    references -- what I send to rank q, one record per row however many of its tokens
 *                                    reference it; the records go out with ONE all_to_all_single and the receiver uses
 *                                    _add_records + _embed_range for its own slice.  h_chunk_end[c] = records claimed by
 *                                    chunks 0..c (chunk c's are [h_chunk_end[c-1], h_chunk_end[c])); synchronises
 *   scone_shard_gather_pack_range    records [first, first + count) of the plan into d_send_buf, followed by `pad` padding
 *                                    records (row id 0xFFFFFFFF: an all-gather wants equal contributions; receivers skip them)
 *   scone_shard_gather_add_records   receiver: records [record0, record0 + n_records) of the gathered buffer
 *                                    (d_records_base = record 0; the buffer will hold n_total records in all, padding
 *                                    included) join the row map; record0 == 0 starts a new exchange
 *   scone_shard_gather_embed_range   sequences [seq_begin, seq_end) of the planned batch out of [replicated head | records
 *                                    added so far]; every row they reference must have been added.  d_out's first row
 *                                    is token out_tok0 of the flattened batch (0: d_out is the whole [B, T, d];
 *                                    seq_begin * T: d_out holds just this run).  B, T must be the planned batch's.  The
 *                                    id lists of a run are rewritten to record numbers in place, ONCE per plan: the slot
 *                                    remembers which sequences already hold record numbers, so a second call over the
 *                                    same or an overlapping range (a retry, other chunk bounds) reduces them as they are;
 *                                    a new exchange (_add_records with record0 == 0) on lists that were already rewritten
 *                                    is refused (SCONE_ESTATE): plan the batch again first.
 * The receiver's row map (row id -> record number) is an open-addressing hash map sized by the exchange (cache-resident). */
/* Plan slots (0 .. 3; 0 is active at first): the receiver-side state of a planned batch (its id lists, the scales of
 * [head | records], the row map) exists once per slot, so that a serving loop can plan, pack and exchange batch b + 1 (and
 * b + 2: the chain plan -> transfers must then fit TWO reductions, not one) on side streams while batch b is still being
 * reduced on the main stream.  A host-side switch, no device work; the
 * scone_shard_gather_plan* / _add_records / _embed_range / _embed calls that follow work on the selected slot.  The
 * sender-side scratch is shared: plan and pack of one batch must be enqueued before the next plan.  New here (the reference is one process). */
int scone_shard_select_slot(scone_handle *h, int32_t slot);
int scone_shard_gather_plan_chunks(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t n_chunks,
                                   int32_t dedup_across_chunks, uint64_t *h_chunk_end, scone_stream_t stream);
/* The match of a plan, sharded over the ranks.  In the all-gather form every rank needs the id lists of the WHOLE batch
 * (it reduces all of it), which makes the match against a 1e9-key index the largest helper kernel of the step.  Index and
 * tokens are replicated and matching is per sequence, so rank r matches only ITS run of sequences, the runs are
 * all-gathered by the caller (32 B per token for max_n <= 3: scone_ell_width ints per token) and the claim passes run over
 * the gathered lists:
 *   scone_shard_gather_match      sequences [seq_begin, seq_end) of the batch d_tok [B, T] against ALL rows -> their list
 *                                 records, (seq_end - seq_begin) * T * width int32 at d_ell_out; stream-ordered, no state
 *   scone_shard_gather_plan_ell   the claim passes of scone_shard_gather_plan_chunks over lists the caller supplies:
 *                                 d_ell [B * T, width] int32, records of the whole batch in token order.  The buffer is
 *                                 BORROWED by the selected plan slot until the batch has been reduced (_embed_range
 *                                 rewrites it in place); same chunk semantics, synchronises
 * New here (the reference matches one sequence at a time in one process: n_gram_extractor.py:106-126). */
int scone_ell_width(scone_handle *h, uint32_t *ints_per_token);
int scone_shard_gather_match(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t seq_begin,
                             int32_t seq_end, int32_t *d_ell_out, scone_stream_t stream);
int scone_shard_gather_plan_ell(scone_handle *h, int32_t *d_ell, int32_t B, int32_t T, int32_t n_chunks,
                                int32_t dedup_across_chunks, uint64_t *h_chunk_end, scone_stream_t stream);
int scone_shard_gather_pack_range(scone_handle *h, uint64_t first, uint64_t count, uint64_t pad, void *d_send_buf,
                                  scone_stream_t stream);
int scone_shard_gather_add_records(scone_handle *h, const void *d_records_base, uint64_t record0, uint64_t n_records,
                                   uint64_t n_total, scone_stream_t stream);
/* Rewrite the id lists of sequences [seq_begin, seq_end) of the planned batch to record numbers now, on `stream` (every row
 * they reference must have been added): a loop that receives on one stream and reduces on another does this where the
 * records arrive, so that scone_shard_gather_embed_range finds the lists done and only launches the lookup. */
int scone_shard_gather_remap_range(scone_handle *h, int32_t seq_begin, int32_t seq_end, scone_stream_t stream);
/* (Token / position ids out of range: as scone_embed, "Ids out of range"; only the ids of sequences [seq_begin, seq_end) are
 * looked at -- here and in scone_shard_gather_embed / scone_shard_cols_embed.) */
int scone_shard_gather_embed_range(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t seq_begin,
                                   int32_t seq_end, const void *d_records_base, uint64_t n_total, const void *d_wte,
                                   int64_t vocab, const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce,
                                   void *d_out, int64_t out_tok0, int32_t out_dtype, scone_stream_t stream);

/* ---- all-gather form with COLUMNS on the wire (one plan = one exchange).  A rank's contribution travels as three arrays
 *      instead of [payload | scales | row id] records: the payload rows at the table's own stride (the lookup reads them in
 *      place, cache-line aligned), the scales (received straight into the caller's [head scales | scales of all ranks]
 *      buffer: nothing to unpack), and the SENDER's hash fragment row id -> position in its contribution (u64 slots; built
 *      while it packs: its own ~65k inserts instead of 0.45M 64-bit CAS on every receiver, ~36 us per step at C5's scale).
 *      The receiver has no indexing pass: a list entry is resolved in its owner's fragment (the owner follows from the id:
 *      contiguous ranges [r N / W, (r + 1) N / W)) and becomes rec_base[owner] + position.
 *   scone_shard_cols_frag_slots   slots of the fragment for `count` rows (a power of two >= 4 count, >= 64): both ends
 *                                 derive it from the exchanged counts
 *   scone_shard_cols_pack         records [first, first + count) of the plan (scone_shard_gather_plan*) as columns;
 *                                 d_frag_out [frag_slots] u64 is cleared and filled; stream-ordered
 *   scone_shard_cols_build_frag   the fragment of an arbitrary id list (position = index in the list): tools and tests
 *                                 stand in for the other ranks with it
 *   scone_shard_head_scales       the replicated head's scales [n_head, scale bytes] into d_out: the front of the scales
 *                                 buffer (once per buffer, not per step)
 *   scone_shard_head_version      a counter bumped by every change of the replicated head (scone_shard_set_head /
 *                                 _head_store_f32 / scone_table_fill_synthetic): a caller's scales buffer whose front was
 *                                 filled at another version takes scone_shard_head_scales again
 *   scone_shard_cols_embed        sequences [seq_begin, seq_end) of the planned batch out of [replicated head | d_rows
 *                                 [n_total, payload bytes]] with scales d_scales_full [n_head + n_total, scale bytes];
 *                                 d_frags holds frag_slots_total u64 slots; h_frag_off[r] (slots into d_frags),
 *                                 h_frag_slots[r], h_rec_base[r] (row number of rank r's first row in d_rows) for r < world
 *                                 (every fragment must lie inside d_frags: SCONE_EINVAL otherwise); h_row_lo[world + 1]:
 *                                 the owners' row ranges -- rank r owns [h_row_lo[r], h_row_lo[r + 1]), ascending from 0 to
 *                                 n_rows (tables of at most 2^32 rows) -- or NULL for the floor partition r * n_rows / world
 *                                 of scone_amd.distributed.shard_range.  Lists are rewritten once per plan, as in
 *                                 scone_shard_gather_embed_range; bit-identical to the unsharded table.
 * New here (the reference keeps its table in one process: embedding_cache.py:49-50). */
/* Sync-free plan (round 4; one chunk): scone_shard_gather_plan_async / _plan_ell_async enqueue match and claim passes and
 * return -- no count comes back to the host; scone_shard_cols_pack_cap packs up to cap_rows of the claimed rows (the capacity
 * both ends sized the transfer for, e.g. the previous batches' counts + 12.5 %), reading the count on the device, and writes
 * d_header_out [2] u64 = {rows claimed, 1 if that exceeded cap_rows}.  The caller ships the header with the columns, reads
 * it when the batch is reduced, and repeats a batch that overflowed with the exact-size calls above (the receivers' lookups
 * of an overflowed exchange raise SCONE_ST_BAD_ID: rows are missing, never read out of bounds). */
int scone_shard_gather_plan_async(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, scone_stream_t stream);
int scone_shard_gather_plan_ell_async(scone_handle *h, int32_t *d_ell, int32_t B, int32_t T, scone_stream_t stream);
int scone_shard_cols_pack_cap(scone_handle *h, uint64_t cap_rows, void *d_rows_out, void *d_scales_out, void *d_frag_out,
                              uint64_t frag_slots, void *d_header_out, scone_stream_t stream);
int scone_shard_cols_frag_slots(uint64_t count, uint64_t *slots);
int scone_shard_cols_pack(scone_handle *h, uint64_t first, uint64_t count, void *d_rows_out, void *d_scales_out,
                          void *d_frag_out, uint64_t frag_slots, scone_stream_t stream);
int scone_shard_cols_build_frag(scone_handle *h, const int32_t *d_ids, uint64_t count, void *d_frag_out, uint64_t frag_slots,
                                scone_stream_t stream);
int scone_shard_head_scales(scone_handle *h, void *d_out, scone_stream_t stream);
int scone_shard_head_version(scone_handle *h, uint64_t *version);
int scone_shard_cols_embed(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t seq_begin, int32_t seq_end,
                           const void *d_rows, uint64_t n_total, const void *d_scales_full, const void *d_frags,
                           uint64_t frag_slots_total, const uint64_t *h_frag_off, const uint64_t *h_frag_slots,
                           const uint64_t *h_rec_base, const uint64_t *h_row_lo, int32_t world, const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos, const int32_t *d_pos,
                           int32_t reduce, void *d_out, int64_t out_tok0, int32_t out_dtype, scone_stream_t stream);

/* ---- transport without kernels for the all-gather form (distributed.py: gather_transport="sdma").  The exchange sends exact
 *      contiguous ranges, so a rank can PUSH its columns into its peers' receive buffers with the copy engines (SDMA over
 *      xGMI) while every wave slot belongs to the lookup kernel -- RCCL's send / recv are kernels that must find room
 *      beside it.  One process per GPU: buffers and events are shared through HIP's interprocess handles (64 opaque
 *      bytes each, moved between the ranks by the caller, e.g. dist.all_gather).
 *   scone_ipc_alloc / _free           device memory on the handle's device + its interprocess handle (a rank's receive buffer)
 *   scone_ipc_open / _close           a peer's buffer mapped into this process (peer access is enabled on demand)
 *   scone_ipc_event_create / _open    an interprocess event (record in the owner, wait anywhere); _destroy frees either kind
 *   scone_ipc_event_record / _wait    stream-ordered.  NB a wait sees the most recent record AT THE TIME OF THE CALL: the
 *                                     caller orders "peer has called record" before "I call wait" itself (a host-side
 *                                     collective between the two, see distributed.py)
 *   scone_ipc_push                    bytes to a (peer-mapped) device pointer on `stream`; copy_engine != 0 forbids the
 *                                     blit-kernel fallback (hipMemcpyDeviceToDeviceNoCU)
 * New here (the reference's only multi-process set-up is training-side DDP, hydra_train.py:32-48). */
int scone_ipc_alloc(scone_handle *h, uint64_t bytes, void **d_ptr, void *handle64);
int scone_ipc_free(scone_handle *h, void *d_ptr);
int scone_ipc_open(scone_handle *h, const void *handle64, void **d_ptr);
int scone_ipc_close(scone_handle *h, void *d_ptr);
int scone_ipc_event_create(scone_handle *h, void **event, void *handle64);
int scone_ipc_event_open(scone_handle *h, const void *handle64, void **event);
int scone_ipc_event_destroy(scone_handle *h, void *event);
int scone_ipc_event_record(scone_handle *h, void *event, scone_stream_t stream);
int scone_ipc_event_wait(scone_handle *h, void *event, scone_stream_t stream);
int scone_ipc_push(scone_handle *h, void *d_dst, const void *d_src, uint64_t bytes, int32_t copy_engine, scone_stream_t stream);

/* ---- backward: deterministic sparse row gradients of the f-gram table (new here; in the reference the table is a trained
 * nn.Embedding, f_gram_model.py:120,172, whose gradient autograd scatters with float atomics).  Appended: SCONE_ABI_VERSION
 * is unchanged.  The gradient needs the id lists and grad_out only and never reads a table row: it works on every row format,
 * placement and shard.
 * Definition.  Position p of a batch of ntok positions has the id list L_p, exactly the list scone_embed / scone_embed_varlen /
 * scone_embed_base* aggregate on this handle: the reference's order (n ascending, start ascending, duplicates kept), every
 * covering f-gram in cover mode and zero or one id in SCONE_MODE_LONGEST_SUFFIX, only the rows in [row_begin, row_end); K_p is
 * the FULL hit count.  A reference is a triple (row r, position p, place k in L_p).  Its contribution, all in IEEE fp32 with
 * g = grad_out: mean  c = fp32(g[p, :]) * w_p, w_p = 1.0f / (float)K_p (one rounded reciprocal per position, one rounded
 * product per element); sum  c = fp32(g[p, :]).  The references of a row are taken in (p, k) ascending order -- a stable sort by
 * row of the reference stream -- and cut into chunks of C = scone_backward_chunk() consecutive references.  A chunk's partial
 * is a = +0.0; a = a + c over its references in order (multiply and add are separate roundings, no fused multiply-add); a row
 * with one chunk gets that partial, a row with several gets acc = +0.0; acc = acc + partial_j in chunk order.  Output: the U
 * distinct rows with at least one reference, d_row_ids_out[U] int64 ascending, each row once, and d_grad_rows_out[U, d] fp32 --
 * the payload of a coalesced torch.sparse_coo_tensor.  No atomics on floating-point data anywhere: the result is a pure function
 * of the inputs, bit for bit, from run to run.  C is part of that contract: a compile-time power of two in [64, 512].
 *   scone_backward_chunk         C; no device work
 *   scone_backward_plan          the lists of scone_embed's batch d_tok [B, T] (matched by the lookup's own matcher; the call
 *                                stream's workspace is held only while that match and the kernels that read its records are
 *                                enqueued), expanded to (row, p) pairs, sorted stably by row, cut into chunks.  The plan owns all
 *                                its buffers -- a later lookup on the same stream does not disturb it -- including the partials
 *                                buffer of the rows with several chunks: nothing is allocated later.  Synchronises the stream
 *                                ONCE, to return U in *h_n_rows and the reference count in *h_n_refs (either may be NULL).
 *                                Token ids out of range: as scone_embed ("Ids out of range": a negative token matches nothing, a
 *                                token >= vocab matches normally; there is no wte here and no status bit).  B * T == 0 and
 *                                U == 0 are valid empty plans.  On a pinned-host table with stage_tokens > 0 the call works as
 *                                on any other (it matches and never touches the staging pipeline)
 *   scone_backward_plan_varlen   the same for scone_embed_varlen's packed batch; scone_embed_varlen's refusals apply (among
 *                                them stage_tokens > 0: SCONE_EINVAL)
 *   scone_backward_plan_csr      the caller's lists, the counterpart of scone_gather_reduce: d_offsets [ntok + 1] / d_ids int32.
 *                                K_p is the list length; ids outside the owned range are skipped; ids outside the table are
 *                                skipped and raise SCONE_ST_BAD_ID (scone_gather_reduce's rule); no such id is ever used as an
 *                                address, and offsets are clamped into [0, d_offsets[ntok]]: with total = d_offsets[ntok], list p
 *                                is d_ids[lo, hi), lo = d_offsets[p] clamped into [0, total], hi = d_offsets[p + 1] clamped into
 *                                [lo, total].  Offsets that decrease give lists that overlap; each is taken as it stands, so
 *                                the references may outnumber total.  Synchronises twice more than the token forms: it reads
 *                                d_offsets[ntok], then the number of owned references, which sizes its buffers
 *   scone_backward_rows          d_grad_out [ntok, d] in grad_dtype (SCONE_DT_*) -> d_row_ids_out / d_grad_rows_out.  Stream-
 *                                ordered: no synchronisation, no allocation.  A plan may be used any number of times, with
 *                                either reduce and any grad_dtype.  rows_cap < U: SCONE_ERANGE, nothing written.  U == 0: a no-op
 *   scone_backward_counts        K_p per position, int32 [ntok]; stream-ordered
 *   scone_backward_plan_destroy  NULL: a no-op
 * SCONE_EINVAL (scone_last_error names the reason): null pointers, a bad grad_dtype / reduce, d % 8 != 0, a handle with
 * dim == 0, a plan of another handle, a batch whose lists could hold 2^32 references or more.  One plan is used by one host
 * thread at a time; plans are independent of each other, and a plan must be destroyed before its handle. */
typedef struct scone_bwd_plan scone_bwd_plan;
int scone_backward_chunk(void);
int scone_backward_plan(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, scone_bwd_plan **out, uint64_t *h_n_rows,
                        uint64_t *h_n_refs, scone_stream_t stream);
int scone_backward_plan_varlen(scone_handle *h, const int32_t *d_tok, const int32_t *d_cu_seqlens, int32_t n_seqs,
                               int64_t total_tokens, scone_bwd_plan **out, uint64_t *h_n_rows, uint64_t *h_n_refs,
                               scone_stream_t stream);
int scone_backward_plan_csr(scone_handle *h, const int32_t *d_offsets, const int32_t *d_ids, int64_t ntok, scone_bwd_plan **out,
                            uint64_t *h_n_rows, uint64_t *h_n_refs, scone_stream_t stream);
int scone_backward_rows(scone_handle *h, scone_bwd_plan *plan, const void *d_grad_out, int32_t grad_dtype, int32_t reduce,
                        int64_t *d_row_ids_out, float *d_grad_rows_out, uint64_t rows_cap, scone_stream_t stream);
int scone_backward_counts(scone_handle *h, scone_bwd_plan *plan, int32_t *d_k_out, scone_stream_t stream);
void scone_backward_plan_destroy(scone_bwd_plan *plan);

/* ---- optimizer step: the fused sparse update of the fp32 master rows, their optimizer state and the served table (new here;
 * the reference trains the table with a stock torch optimizer).  Appended: SCONE_ABI_VERSION is unchanged.  It consumes what
 * scone_backward_rows returns: d_row_ids [n] int64 ascending and distinct, d_grad_rows [n, d] fp32.
 * Arrays.  d_master, d_state1, d_state2: fp32 [row_end - row_begin, d] on the handle's device, indexed by id - row_begin (the
 * handle's owned rows).  d_state1 is Adam's m; d_state2 is Adam's v or Adagrad's sum of squares; an array the kind does not use
 * may be NULL.  All three are updated in place.
 * Scalars.  scone_opt_scalars_of computes them on the host in double and rounds each to fp32 ONCE (no GPU, no handle):
 *   alpha = lr (SGD, Adagrad);  alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t) (Adam, t = step >= 1)
 *   b1 = beta1, b2 = beta2, c1 = 1 - beta1, c2 = 1 - beta2, eps = eps, decay = lr * weight_decay, gscale = grad_scale
 * scone_opt_step uses exactly these values; a test that wants the bits reads them here (as C from scone_backward_chunk).
 * Per element (g of d_grad_rows, w of d_master, m / v / s of the state), every operation IEEE fp32 and rounded once, NO fused
 * multiply-add, sqrt and / correctly rounded, subnormals kept -- the translation unit is built with the Makefile's flags
 * (-ffp-contract=off, nothing else: correctly rounded sqrt and division and IEEE subnormals are hipcc's defaults for gfx950):
 *   g1 = gscale == 1 ? g : g * gscale
 *   w1 = decay  == 0 ? w : w - decay * w                   (decoupled and lazy: only the listed rows decay)
 *   SGD      w' = w1 - alpha * g1
 *   ADAGRAD  s' = s + g1 * g1 ;                             w' = w1 - (alpha * g1) / (sqrt(s') + eps)
 *   ADAM     m' = b1 * m + c1 * g1 ; v' = b2 * v + c2 * (g1 * g1) ; w' = w1 - (alpha * m') / (sqrt(v') + eps)
 * gscale == 1 and decay == 0 skip their step exactly (no multiply by 1, no subtraction of 0 * w).
 * Served table.  Global row id of the handle's table becomes exactly what scone_table_store_f32_ids of the w' row would have
 * stored: every format and its scales (the d == 1024 scale-slot orders of INT4 / MXFP4 included), HBM or a pinned-host table
 * with a hot head, a row-sharded handle.  As with that call, a staged-prefetch cache (stage_tokens > 0), if one exists, is
 * dropped first.  A row that is not listed keeps every bit: master, state and table.
 * Ids.  An id outside [row_begin, row_end) is skipped and raises SCONE_ST_BAD_ID; an id <= its predecessor in the list is
 * skipped and raises SCONE_ST_BAD_ID; no such id is ever used as an address.  Every other row is applied, by one wavefront,
 * independent of every other.  (A list that repeats a row at a distance is outside the contract: both copies are applied, in
 * no order; nothing outside that row is touched.)
 * The call is stream-ordered: it does not synchronise, allocates nothing and does all its device work in ONE kernel launch
 * (grid capped as every row-parallel kernel here; environment SCONE_OPT_MAX_BLOCKS, read by scone_create, lowers the cap).
 * n == 0: a no-op.  Plain vector stores only; no atomics but the integer OR on the status word: a pure function of its inputs.
 * SCONE_EINVAL (scone_last_error names the reason): null cfg / d_row_ids / d_grad_rows / d_master, a state array the kind
 * needs is NULL, a bad kind or struct_size, step < 1 for Adam, a non-finite lr / beta1 / beta2 / eps / weight_decay /
 * grad_scale, a handle with dim == 0. */
enum { SCONE_OPT_SGD = 0, SCONE_OPT_ADAGRAD = 1, SCONE_OPT_ADAM = 2 };
typedef struct scone_opt_cfg {
  uint32_t struct_size; /* sizeof(scone_opt_cfg) */
  int32_t kind;         /* SCONE_OPT_* */
  double lr, beta1, beta2, eps, weight_decay, grad_scale; /* grad_scale 1.0 and weight_decay 0.0: that step is skipped exactly */
  int64_t step;         /* t >= 1: Adam's bias correction; ignored by the others */
} scone_opt_cfg;
typedef struct scone_opt_scalars {
  float alpha, b1, b2, c1, c2, eps, decay, gscale;
} scone_opt_scalars;
int scone_opt_scalars_of(const scone_opt_cfg *cfg, scone_opt_scalars *out);
int scone_opt_step(scone_handle *h, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows, uint64_t n,
                   float *d_master, float *d_state1, float *d_state2, scone_stream_t stream);

/* ---- lean optimizer step: training a table that is too large for scone_opt_step's fp32 [N, d] master and state arrays (new
 * here).  Appended: SCONE_ABI_VERSION is unchanged; scone_opt_step and scone_opt_cfg are as they were.  Two changes make the
 * memory small: ROW-WISE Adagrad keeps ONE fp32 accumulator per row (d_row_state, fp32 [row_end - row_begin], indexed by
 * id - row_begin) instead of one per element, and IN-PLACE mode has no master copy at all: the served fp32 / bf16 rows are
 * the weights.  A 100M x 1024 bf16 table is 205 GB of rows + 0.4 GB of state; scone_opt_step's Adam needs 1.2 TB beside it.
 * d_row_ids [n] int64 and d_grad_rows [n, d] fp32 are what scone_backward_rows returns, as for scone_opt_step.
 * Modes.
 *   master mode (d_master != NULL): d_master is fp32 [row_end - row_begin, d] as in scone_opt_step; the master row is updated
 *     in place and the served row becomes exactly what scone_table_store_f32_ids of the new master row stores -- every format
 *     and every placement scone_opt_step supports.  SCONE_LEAN_SGD here equals scone_opt_step's SGD bit for bit.
 *   in-place mode (d_master == NULL): w is the stored element widened to fp32 (fp32: the value; bf16: bits << 16), read and
 *     written through the handle's own row store (HBM, pinned host with a hot head, an owned shard range).  SCONE_FMT_F32 and
 *     SCONE_FMT_BF16 tables only: every other format returns SCONE_EINVAL naming it (a quantised row cannot hold a small
 *     update; fp16 is left out on purpose).
 * Scalars.  scone_lean_scalars_of (no GPU, no handle) fills alpha = lr, eps = eps, decay = lr * weight_decay, gscale =
 * grad_scale, each computed in double and rounded to fp32 ONCE; the other fields of scone_opt_scalars are 0.
 * Per element, every operation IEEE fp32 and rounded once, NO fused multiply-add, sqrt and / correctly rounded, subnormals kept
 * (the unit is built with the Makefile's flags, as scone_opt_step's is):
 *   g1 = gscale == 1 ? g : g * gscale
 *   w1 = decay  == 0 ? w : w - decay * w
 *   SGD              w' = w1 - alpha * g1
 *   ROWWISE_ADAGRAD  q  = row sum of g1 * g1 (order below);  g2 = q / (float)d;  s' = s + g2   (one s per row)
 *                    den = sqrtf(s') + eps;                   w'_j = w1_j - (alpha * g1_j) / den
 * Row sum order (part of the contract).  Element j belongs to lane l = (j / 4) % 64.  Each lane starts at q_l = +0.0f and adds
 * its elements in ascending j as q_l = q_l + (g1_j * g1_j): the product is rounded first, then the sum.  A lane with no element
 * holds +0.0f.  Then, for s = 32, 16, 8, 4, 2, 1:  q_l = q_l + q_(l ^ s), all lanes at once.  Every lane ends with the same bits
 * (fp32 addition is commutative and each stage pairs l with l ^ s); that value is q.
 * Rounding of the stored row (in-place bf16 only; cfg.rounding).
 *   SCONE_ROUND_NEAREST     round-to-nearest-even, the table's own fp32 -> bf16 conversion.
 *   SCONE_ROUND_STOCHASTIC  u = the fp32 bits of w'.  Exponent field all ones (inf / NaN): as nearest.  Otherwise the stored
 *     bits are (u + r) >> 16 in 32-bit arithmetic, r = scone_lean_rand16(seed, step, GLOBAL row id, j) in [0, 65536).  A value
 *     bf16 holds exactly never changes; both signs round away from zero with probability frac / 65536, so the rounding is
 *     unbiased; a carry out of the largest finite value gives infinity, as round-to-nearest's does.
 *   SCONE_ROUND_STOCHASTIC with a master, or on an fp32 table: SCONE_EINVAL (there is nothing to round).
 * Random bits.  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (32-bit).  h = 0x9E3779B9;
 * h = mix(h ^ v) for v = seed low, seed high, step low, step high, row low, row high, col in turn; r = h >> 16.  Keyed by the
 * GLOBAL row id and the column, never by list position, wave, grid or shard: the bits of a row do not depend on the batch,
 * the grid cap or how the table is sharded.  cfg.seed and cfg.step feed these bits and nothing else.  scone_lean_rand16 is
 * the host copy of the device function (no GPU, no handle).
 * Ids: scone_opt_step's rules.  An id outside [row_begin, row_end) is skipped and raises SCONE_ST_BAD_ID; an id <= its
 * predecessor in the list is skipped and raises SCONE_ST_BAD_ID; no such id is ever used as an address.  A row that is not
 * listed keeps every bit: table row, master and row state.
 * The call is stream-ordered: no synchronisation, no allocation, all device work in ONE kernel launch (grid capped as
 * scone_opt_step's; SCONE_OPT_MAX_BLOCKS applies).  A staged-prefetch cache is dropped first.  n == 0: a no-op.  Plain vector
 * stores only; no atomics but the integer OR on the status word.
 * SCONE_EINVAL (scone_last_error names the reason): a null cfg / d_row_ids / d_grad_rows, a null d_row_state for row-wise
 * Adagrad, a bad kind, rounding or struct_size, reserved != 0, a non-finite lr / eps / weight_decay / grad_scale, a handle
 * with dim == 0, the mode and format refusals above. */
enum { SCONE_LEAN_SGD = 0, SCONE_LEAN_ROWWISE_ADAGRAD = 1 };
enum { SCONE_ROUND_NEAREST = 0, SCONE_ROUND_STOCHASTIC = 1 };
typedef struct scone_lean_cfg {
  uint32_t struct_size; /* sizeof(scone_lean_cfg) */
  int32_t kind;         /* SCONE_LEAN_* */
  int32_t rounding;     /* SCONE_ROUND_* */
  int32_t reserved;     /* 0 */
  double lr, eps, weight_decay, grad_scale;
  uint64_t seed;        /* feed the random bits only */
  int64_t step;
} scone_lean_cfg;
int scone_lean_scalars_of(const scone_lean_cfg *cfg, scone_opt_scalars *out);
uint32_t scone_lean_rand16(uint64_t seed, int64_t step, uint64_t row_id, uint32_t col);
int scone_opt_step_lean(scone_handle *h, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                        uint64_t n, float *d_master /* NULL: in place */, float *d_row_state /* fp32 [row_end - row_begin] */,
                        scone_stream_t stream);

/* ---- backward applied in place: scone_backward_rows and the in-place scone_opt_step_lean in ONE pass (new here; FBGEMM /
 * TorchRec fuse an embedding table's backward with its optimizer the same way).  Appended: SCONE_ABI_VERSION is unchanged, and
 * every entry point above is as it was.  The table gradient -- fp32 [U, d], the one table-sized-per-batch array of in-place
 * training -- is never stored: there is no grad_rows and no row_ids output, and no device buffer is sized by U * d.
 * Contract.  After the call the table rows and d_row_state hold exactly the bits that
 *   scone_backward_rows(h, plan, d_grad_out, grad_dtype, reduce, ids, rows, U), then
 *   scone_opt_step_lean(h, cfg, ids, rows, U, NULL, d_row_state)
 * leave with the same arguments; a row the plan does not list keeps every bit.  So the gradient's order (reference order,
 * chunks of scone_backward_chunk(), partials in chunk order), the update's per-element arithmetic, the order of the row-wise
 * sum (lane (j / 4) % 64, ascending j, the butterfly) and the stochastic bits (keyed by the GLOBAL row id and the column) are
 * the ones stated under "backward" and "lean optimizer step".
 * In-place mode only: SCONE_FMT_F32 and SCONE_FMT_BF16 tables; master mode stays with the two calls.  HBM, a pinned-host table
 * with a hot head and a row-sharded handle all work (the rows go through the handle's own row store); the plan may come from
 * any of the three plan calls, in both lookup modes.  Every d % 8 == 0 up to 4096 is fused: a wave keeps the finished gradient
 * row in its share of LDS.  d > 4096 returns SCONE_EINVAL naming the two calls above, which have no such limit.
 * The call is stream-ordered: it does not synchronise and allocates nothing.  A staged-prefetch cache is dropped first, as
 * scone_opt_step_lean does.  An empty plan (U == 0) is a no-op.  At most two kernel launches: the first, only when the plan
 * has rows with several chunks, fills the plan's partials of those rows, a wavefront per chunk; the second is the fused
 * kernel, a wavefront per touched row, its grid capped as scone_opt_step's (SCONE_OPT_MAX_BLOCKS applies).  Plain vector
 * stores only and no atomics: plan rows are owned, distinct and ascending, so no id is checked and no status bit can rise.
 * The plan's partials are scratch of the call: as with scone_backward_rows, one plan is used by one host thread at a time.
 * SCONE_EINVAL (scone_last_error names the reason, prefixed "scone_backward_apply_lean: "): what scone_opt_step_lean says of
 * a cfg, a handle with dim == 0, a null plan / d_grad_out, a plan of another handle, a bad grad_dtype / reduce, a table that is
 * not fp32 / bf16 (the format is named), stochastic rounding on an fp32 table, row-wise Adagrad without d_row_state, d > 4096. */
int scone_backward_apply_lean(scone_handle *h, scone_bwd_plan *plan, const void *d_grad_out, int32_t grad_dtype, int32_t reduce,
                              const scone_lean_cfg *cfg, float *d_row_state, scone_stream_t stream);

/* ---- gradient norm, clipping and skipped steps: what a training loop puts around the optimizer step, kept on the device (new
 * here; torch.nn.utils.clip_grad_norm_ cannot take a sparse gradient, and a GradScaler's found-inf check is a host read).
 * Appended: SCONE_ABI_VERSION is unchanged and every entry point above keeps its bits and its behaviour.  Three parts:
 * scone_grad_sqnorm reduces d_grad_rows to its squared norm in a fixed order; scone_grad_ctl_set turns such terms into a clip
 * coefficient and a skip flag in a 24-byte block on the device; scone_opt_step_ctl / scone_opt_step_lean_ctl are the two
 * optimizer steps reading their scale and the flag from that block.  No call synchronises or allocates; all are stream-ordered.
 *
 * 1. scone_grad_sqnorm.  d_grad_rows is fp32 [n, d], d = cfg.dim (a multiple of 4), what scone_backward_rows returns.
 *   d_scratch holds scone_grad_sqnorm_scratch(n) = n + ceil(n / 1024) doubles (that call does no device work); d_sq_out is ONE
 *   double.  All sums are IEEE double, every addition rounded once.  Element g enters as (double)g * (double)g: that product is
 *   exact (48 significant bits), so fusing it with the addition cannot change a bit.  Every fp32 value, its square and any sum
 *   of them fit a double: the total is finite if and only if every element is finite, and it is exactly +0.0 only if every
 *   element is +-0 (subnormal elements count).
 *   Row r (the lane order of the lean step's row sum).  Element j of the row belongs to lane l = (j / 4) % 64.  a_l = +0.0; then
 *     a_l = a_l + g_j * g_j in ascending j (a lane with no element keeps +0.0).  Then, for s = 32, 16, 8, 4, 2, 1:
 *     a_l = a_l + a_(l ^ s), all 64 lanes at once.  Q_r = a_0 is stored to d_scratch[r]: the per-row squared norms are an output.
 *   Tile k covers rows [1024k, 1024k + 1024).  Thread t of 256 starts at b_t = +0.0 and adds Q_(1024k + t + 256i) for i = 0, 1,
 *     2, 3 in that order, skipping rows >= n.  Then a tree, for s = 128, 64, .. 1: b_t = b_t + b_(t + s) for every t < s.
 *     P_k = b_0 is stored to d_scratch[n + k]; there are ceil(n / 1024) tiles.
 *   Total.  One workgroup of 256 threads: thread t starts at +0.0 and adds P_(t + 256i) in ascending i; the same tree follows;
 *     b_0 is stored to *d_sq_out.  n == 0 stores +0.0 (no tile, nothing else is written or read).
 *   The result is a pure function of the n * d input values: it does not depend on the grid, on SCONE_OPT_MAX_BLOCKS (which caps
 *   the row kernel's grid as it caps scone_opt_step's) or on the run.  No atomics.  At most three kernel launches.
 *   SCONE_EINVAL (scone_last_error names the reason, prefixed "scone_grad_sqnorm: "): a null d_grad_rows or d_scratch with
 *   n > 0, a null d_sq_out, a handle with dim == 0.
 *
 * 2. scone_grad_ctl_set.  d_terms: n_terms (1 .. 64) doubles on the device -- the table's squared norm is one, the squared norm
 *   of the dense parameters' gradients (the caller's, from torch) another, other shards one each.  ONE device thread computes,
 *   every operation in IEEE double and rounded once, sqrt and / correctly rounded:
 *     total  = +0.0; total = total + d_terms[i] in ascending i
 *     norm64 = sqrt(total) * fabs(grad_scale)                  (the norm of the UN-scaled gradient)
 *     c      = max_norm / (norm64 + 1e-6)                      (torch.nn.utils.clip_grad_norm_)
 *     coef   = c < 1.0 ? (float)c : 1.0f                       (a NaN compares false: 1.0f)
 *     skip   = skip_nonfinite != 0 && total is inf or NaN ? 1 : 0
 *     sqnorm = total, norm = (float)norm64, reserved = 0
 *   and stores the block to d_ctl.  max_norm = +inf: no clipping (coef = 1.0f).  One kernel launch.
 *   SCONE_EINVAL (prefixed "scone_grad_ctl_set: "): a null d_terms / d_ctl, n_terms outside 1 .. 64, a grad_scale that is not
 *   finite, a max_norm that is <= 0 or NaN.
 *
 * 3. scone_opt_step_ctl / scone_opt_step_lean_ctl: scone_opt_step / scone_opt_step_lean with d_ctl before the stream.  Every
 *   wavefront reads skip and coef before it touches anything else.  skip != 0: the launch changes NOTHING -- no master or table
 *   row, no state, no scale, no status bit (ids are not looked at).  Otherwise gscale_eff = gscale * coef, ONE fp32 product of
 *   the cfg's gscale (scone_opt_scalars_of / scone_lean_scalars_of) and the block's coef, and the call is bit for bit the plain
 *   call whose gscale is that value -- the exact skip of the multiply when gscale_eff == 1 included.  Still one launch, no
 *   synchronisation, no allocation; ids, modes, formats and refusals are the plain call's (the host side cannot know the flag:
 *   a staged-prefetch cache is dropped either way).  A null d_ctl: SCONE_EINVAL.  Messages are prefixed with the call's name.
 *   scone_backward_apply_lean has no such form: a clipped update needs the norm before the first row is written. */
typedef struct scone_grad_ctl {
  double sqnorm;     /* the sum of the terms */
  float norm;        /* sqrt(sqnorm) * |grad_scale| */
  float coef;        /* min(1, max_norm / (norm + 1e-6)): multiply every gradient by it */
  uint32_t skip;     /* 1: the _ctl steps change nothing */
  uint32_t reserved; /* 0 */
} scone_grad_ctl;    /* 24 bytes */
int scone_grad_sqnorm_scratch(uint64_t n, uint64_t *n_doubles);
int scone_grad_sqnorm(scone_handle *h, const float *d_grad_rows, uint64_t n, double *d_scratch, double *d_sq_out,
                      scone_stream_t stream);
int scone_grad_ctl_set(scone_handle *h, const double *d_terms, int32_t n_terms, double grad_scale, double max_norm,
                       int32_t skip_nonfinite, scone_grad_ctl *d_ctl, scone_stream_t stream);
int scone_opt_step_ctl(scone_handle *h, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows, uint64_t n,
                       float *d_master, float *d_state1, float *d_state2, const scone_grad_ctl *d_ctl, scone_stream_t stream);
int scone_opt_step_lean_ctl(scone_handle *h, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                            uint64_t n, float *d_master, float *d_row_state, const scone_grad_ctl *d_ctl, scone_stream_t stream);

/* ---- gradient accumulation: the sum of two sparse row gradients over micro-batches, kept on the device (new here; torch's
 * coalesce() is the stock way, a sort with a host read of the output size).  Appended: SCONE_ABI_VERSION is unchanged and every
 * entry point above keeps its bits and its behaviour.  A sparse row gradient is what scone_backward_rows returns: n int64 row
 * ids, ascending and distinct, and fp32 rows [n, d], d = cfg.dim.  Two parts: scone_grad_merge_map + scone_grad_merge_rows add
 * two such gradients that exist; scone_backward_row_ids + scone_backward_rows_acc add the gradient of a plan to an old one
 * without ever storing it.  0xFFFFFFFF in a src array means "absent".
 *
 * 1. scone_grad_merge_map.  d_ids_a [n_a] and d_ids_b [n_b] are the two id lists.  d_ids_out, d_src_a and d_src_b have room for
 *   n_a + n_b entries, d_pos_a for n_a, d_pos_b for n_b; d_scratch holds scone_grad_merge_scratch(n_a, n_b) bytes (that call does
 *   no device work; its result does not decrease when an argument grows); d_n_out is ONE uint64 on the device.
 *     d_ids_out[0, n_out)  the ascending union of the two lists
 *     d_src_a[i]           the index in a of output row i, or absent; d_src_b[i] the same for b
 *     d_pos_a[k]           the output row of a's row k; d_pos_b[k] the same for b
 *     *d_n_out             n_out
 *   Entries [n_out, n_a + n_b) of d_src_a / d_src_b are absent; those of d_ids_out are not written.  Ids are compared as signed
 *   int64 and are never an address: every id finds its place by a binary search in the other list.  h_n_out != NULL: the stream
 *   is synchronised ONCE and n_out returned, as the backward plan returns U; h_n_out == NULL: no synchronisation.  The call
 *   allocates nothing.  n_a == 0, n_b == 0 and both are valid (the arrays of an empty list may be NULL).
 *   A list that is not ascending and distinct is outside the contract: SCONE_ST_BAD_ID is raised (every entry is compared with
 *   its predecessor) and the output is unspecified but bounded -- every d_src entry is absent or an index inside its list,
 *   every d_pos entry is < n_a + n_b, n_out <= n_a + n_b, and nothing is written outside the capacities stated above.
 *   SCONE_EINVAL, before any device work (scone_last_error names the reason, prefixed "scone_grad_merge_map: "):
 *   n_a + n_b >= 2^32 - 1, a null pointer (d_scratch and d_n_out always; the others when their list is not empty), a handle
 *   with dim == 0.
 *
 * 2. scone_grad_merge_rows.  d_src_a / d_src_b [n_out] are the map's; d_rows_a / d_rows_b the two gradients' rows, d_rows_out
 *   fp32 [n_out, d], d % 4 == 0.  Output row i:
 *     in a only   that row of a, bit for bit (-0.0 stays -0.0: a copy, not an add to zero)
 *     in b only   that row of b, bit for bit
 *     in both     a + b per element: ONE IEEE fp32 add, a the first operand, subnormals kept
 *   (a row neither has -- possible only with a map of lists outside the contract -- is stored as +0.0).  Stream-ordered, ONE
 *   launch, a wavefront per output row, its grid capped as scone_opt_step's (SCONE_OPT_MAX_BLOCKS applies); no allocation, no
 *   atomics, plain vector stores.  n_out == 0: a no-op.  The output must not overlap an input.
 *   SCONE_EINVAL (prefixed "scone_grad_merge_rows: "): d_rows_out equal to d_rows_a or d_rows_b, a null d_src_a / d_src_b /
 *   d_rows_out with n_out > 0, n_out >= 2^32 - 1, a handle with dim == 0 or dim % 4 != 0.
 *
 * 3. scone_backward_row_ids: the U row ids of a plan, ascending, what scone_backward_rows writes to d_row_ids_out, without
 *   computing a row.  One launch; U == 0: a no-op.  SCONE_ERANGE: rows_cap < U.  SCONE_EINVAL: a null plan / pointer, a plan of
 *   another handle.
 *
 * 4. scone_backward_rows_acc.  d_src_old, d_src_new and d_pos_new are d_src_a, d_src_b and d_pos_b of
 *   scone_grad_merge_map(a = the old gradient's ids, b = scone_backward_row_ids of the plan), n_out its count; d_rows_old the
 *   old gradient's rows.  After the call d_rows_out [n_out, d] holds exactly the bits that
 *     scone_backward_rows(h, plan, d_grad_out, grad_dtype, reduce, ids, rows, U), then
 *     scone_grad_merge_rows(h, d_src_old, d_src_new, n_out, d_rows_old, rows, d_rows_out)
 *   leave, and the fp32 [U, d] array `rows` never exists.  A row of one chunk is summed as stated under "backward", then
 *   old + sum is stored (the sum itself where the old gradient has no such row); a row of several chunks goes through the
 *   plan's partial slots, which are added in chunk order, and old is added last; a row only the old gradient has is copied.
 *   Stream-ordered, at most three launches (SCONE_OPT_MAX_BLOCKS caps their grids), no allocation, no synchronisation, no
 *   atomics.  U == 0: d_rows_out is a copy of d_rows_old.  n_out == 0: a no-op.  The plan's partials are scratch of the call, as
 *   with scone_backward_rows.  d_pos_new is trusted to be the map's: an entry >= n_out is skipped, never an address.
 *   SCONE_EINVAL (prefixed "scone_backward_rows_acc: "): what scone_backward_rows refuses (a null plan / pointer, a plan of
 *   another handle, a bad grad_dtype / reduce, d % 8 != 0), d_rows_out equal to d_rows_old, n_out >= 2^32 - 1.  SCONE_ERANGE:
 *   n_out < U. */
int scone_grad_merge_scratch(uint64_t n_a, uint64_t n_b, uint64_t *bytes);
int scone_grad_merge_map(scone_handle *h, const int64_t *d_ids_a, uint64_t n_a, const int64_t *d_ids_b, uint64_t n_b,
                         int64_t *d_ids_out, uint32_t *d_src_a, uint32_t *d_src_b, uint32_t *d_pos_a, uint32_t *d_pos_b,
                         void *d_scratch, uint64_t *d_n_out, uint64_t *h_n_out, scone_stream_t stream);
int scone_grad_merge_rows(scone_handle *h, const uint32_t *d_src_a, const uint32_t *d_src_b, uint64_t n_out,
                          const float *d_rows_a, const float *d_rows_b, float *d_rows_out, scone_stream_t stream);
int scone_backward_row_ids(scone_handle *h, scone_bwd_plan *plan, int64_t *d_row_ids_out, uint64_t rows_cap, scone_stream_t stream);
int scone_backward_rows_acc(scone_handle *h, scone_bwd_plan *plan, const void *d_grad_out, int32_t grad_dtype, int32_t reduce,
                            const uint32_t *d_src_old, const uint32_t *d_src_new, const uint32_t *d_pos_new, uint64_t n_out,
                            const float *d_rows_old, float *d_rows_out, scone_stream_t stream);

/* ---- backward of the dense side: deterministic gradients of wte and wpe (new here; the reference leaves them to autograd,
 * language_model.py:239-254, whose embedding backward scatters with float atomics).  New entry points only: SCONE_ABI_VERSION is
 * unchanged, and every other entry point keeps its bits, its refusals and its stream contract.  The section stands here, behind
 * "gradient accumulation", whose scone_backward_row_ids / scone_backward_rows_acc it uses: the header ends with
 * scone_embed_select, and the prototypes of the sections in between are counted.  The prototypes spell their stream
 * `void *stream` (the same type as scone_stream_t), as the section "backward and optimizer step without a host synchronisation".
 * What it is for: out = (wte[tok] + reduce_k row_k) + wpe[pos].  The sections above give the gradient of the middle term; the
 * gradient of row i of wte (of wpe) is the sum of grad_out[p, :] over the positions p whose token (position id) is i -- the
 * table's backward in a second id space, with lists of one element.
 * Definition.  An INDEX PLAN over d_idx [ntok] int32 and an id space of n_ids ids is the backward plan ("backward", above) of
 * a batch whose position p has the list [d_idx[p]].  A position has NO reference if d_idx[p] is outside [0, n_ids), or if
 * d_skip != NULL and d_skip[p] != 0.  K_p is the list length (0 or 1) and the weight is 1.0f.  Everything else is the
 * contract of "backward", word for word: the references of an id are taken in ascending p and cut into chunks of
 * C = scone_backward_chunk() consecutive references; a chunk's partial is a = +0.0; a = a + c over its references in order;
 * an id with one chunk gets that partial, an id with several gets acc = +0.0; acc = acc + partial_j in chunk order; multiply
 * and add are separate roundings; no atomics on floating-point data anywhere.  The weight being 1.0f, either `reduce` gives
 * the sum's bits.  Ids out of range are skipped silently: the forward already raises SCONE_ST_BAD_TOKEN for them, and this
 * backward raises no status bit, as scone_backward_plan raises none.
 *   scone_backward_plan_index        builds that plan: the (id, p) pairs, sorted stably by id, cut into chunks -- the passes of
 *                                    scone_backward_plan without its match and without a workspace.  n_ids is INDEPENDENT of the
 *                                    handle's table (a 50,257-row wte on a table of 40 rows): the plan carries its own id-space
 *                                    size.  Synchronises the stream ONCE, to return U (the distinct ids with a reference) in
 *                                    *h_n_rows and the reference count in *h_n_refs (either may be NULL), as scone_backward_plan
 *                                    does.  ntok == 0 and U == 0 are valid empty plans.  The result is a scone_bwd_plan:
 *                                    scone_backward_rows (d_row_ids_out: the ids, int64 ascending; d_grad_rows_out [U, d] fp32:
 *                                    the rows of the dense gradient that are not zero), scone_backward_row_ids,
 *                                    scone_backward_counts (K_p: 0 or 1), scone_backward_rows_acc and
 *                                    scone_backward_plan_destroy take it as they take any other.  scone_backward_apply_lean
 *                                    returns SCONE_EINVAL for it: its ids are not table rows.  SCONE_EINVAL: a null out, a null
 *                                    d_idx with ntok > 0, ntok < 0 or ntok >= 2^32, n_ids <= 0 or n_ids >= 2^32 - 1, a handle
 *                                    with dim == 0 or d % 8 != 0
 *   scone_backward_default_positions writes to d_pos_out [total_tokens] int32 the position the lookup uses for every p when it is
 *                                    given d_pos == NULL: p % T for the rectangle (d_cu_seqlens == NULL; n_seqs is ignored), the
 *                                    matcher's p - cu[s] for scone_embed_varlen's packed batch (d_cu_seqlens [n_seqs + 1]; T is
 *                                    ignored; n_seqs == 0: a no-op).  With it the wpe gradient of a packed batch, or of any batch
 *                                    with default positions, is an index plan with n_ids = n_pos.  Stream-ordered, one launch:
 *                                    it does not synchronise and does not allocate.  SCONE_EINVAL: negative sizes, total_tokens
 *                                    above 2^31 - 1, a rectangle with T <= 0 or total_tokens % T != 0, a null d_pos_out
 *   scone_backward_wpe_scratch       the bytes of scratch scone_backward_wpe needs for a rectangle [B, T] at dim d: the
 *                                    partials of ceil(B / C) chunks per row when B > C, else 0.  No handle, no device work
 *   scone_backward_wpe               grad_wpe of the rectangle [B, T] with DEFAULT positions: row t of d_grad_wpe_out
 *                                    [min(T, n_pos), d] fp32 is the sum of g[b * T + t, :] for b ascending, g = d_grad_out
 *                                    [B * T, d] in grad_dtype.  The references of row t are known by arithmetic, so there is no
 *                                    plan, no sort, no synchronisation and no allocation: a wave owns (row t, chunk j of C batch
 *                                    rows), computes its positions, and adds in b order; when B > C the partials go to d_scratch
 *                                    and a second launch adds them in chunk order.  Its bits are those of
 *                                    scone_backward_plan_index(n_ids = n_pos) on scone_backward_default_positions followed by
 *                                    scone_backward_rows, for every row t < n_pos (every such row has B >= 1 references); rows
 *                                    t >= n_pos do not exist -- their position is out of range in the lookup.  B * T == 0: a
 *                                    no-op.  The call is stream-ordered: it does not synchronise and allocates nothing; at most
 *                                    two launches.  d_scratch is scratch of the call (may be NULL when the size is 0).
 *                                    SCONE_EINVAL: null pointers, a bad grad_dtype, negative B or T, B * T above 2^31 - 1,
 *                                    n_pos <= 0, a handle with dim == 0 or d % 8 != 0
 * Left out, and meant to be: the index plan in the form whose counts stay on the device (a scone_bwd_ctx).  A captured step
 * trains the table only. */
int scone_backward_plan_index(scone_handle *h, const int32_t *d_idx, int64_t ntok, int64_t n_ids, const int32_t *d_skip,
                              scone_bwd_plan **out, uint64_t *h_n_rows, uint64_t *h_n_refs, void *stream);
int scone_backward_default_positions(scone_handle *h, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t T, int64_t total_tokens,
                                     int32_t *d_pos_out, void *stream);
int scone_backward_wpe_scratch(int32_t B, int32_t T, int32_t d, uint64_t *bytes);
int scone_backward_wpe(scone_handle *h, const void *d_grad_out, int32_t grad_dtype, int32_t B, int32_t T, int64_t n_pos,
                       float *d_grad_wpe_out, void *d_scratch, void *stream);

/* ---- optimizer hyper-parameters on the device: a captured step with Adam, stochastic rounding, a learning-rate schedule and a
 * dynamic loss scale (new here; torch.optim.Adam(capturable=True) keeps its step count on the device for the same reason).
 * SCONE_ABI_VERSION is unchanged; every other entry point keeps its bits, its refusals and its stream contract.  The section
 * stands IN FRONT of the one it builds on ("backward and optimizer step without a host synchronisation", next): the header ends
 * with scone_embed_select, and that section's prototypes are counted; a declaration's place changes nothing for a compiler.
 * What it is for: the by-value steps take lr, grad_scale, Adam's t and the stochastic rounding's step BY VALUE, so a replayed graph
 * repeats them as captured, and the host counts a step that the device skipped.  Here they live in a block of 104 bytes on the
 * device (8-byte aligned): scone_opt_hyper_init writes it, scone_opt_hyper_advance counts the step and derives the fp32 scalars
 * ON THE DEVICE, and scone_opt_step_dh / scone_opt_step_lean_dh / scone_grad_ctl_set_dh read them there.  Between steps the
 * caller may overwrite any input field with stream-ordered device work of its own (a copy, a fill, a scheduler kernel).
 * No call of this section synchronises or allocates; all are stream-ordered.
 *
 * 1. Scalars.  scone_opt_hyper_scalars_of(cfg, out) is the host copy of what the advance derives at t = cfg->step (no GPU, no
 *   handle, as scone_lean_rand16): a PURE FUNCTION of (cfg, t).  It equals scone_opt_scalars_of in every field but Adam's
 *   alpha, which uses a stated integer power instead of libm's pow, so that host and device agree bit for bit:
 *     ipow(b, t):  r = 1.0; while (t) { if (t & 1) r = r * b; t >>= 1; if (t) b = b * b; }     (every product ONE IEEE double)
 *     alpha = (float)((lr * sqrt(1 - ipow(beta2, t))) / (1 - ipow(beta1, t)))                    (ADAM; sqrt and / correctly
 *             rounded in double, as scone_grad_ctl_set relies on; SGD, ADAGRAD: alpha = (float)lr)
 *   It can differ from scone_opt_scalars_of's alpha by at most one fp32 ulp (the two powers differ by a few double ulps, far
 *   below half an fp32 ulp except at a rounding boundary); for lr = 1e-3, betas (0.9, 0.999), (0.9, 0.95), (0.5, 0.99),
 *   (0.0, 0.999) and t = 1 .. 20000, 10^6, 12345678, 2^31 - 1 the two were identical.  Refusals: scone_opt_scalars_of's.
 *
 * 2. scone_opt_hyper_init(h, cfg, seed, d_hyper): ONE launch of one thread stores the six doubles of cfg (taken by value),
 *   seed, step = cfg->step -- here the number of steps ALREADY APPLIED, so >= 0 (0 for a fresh optimizer) -- and sc = 0,
 *   applied = 0, bad = 0.  cfg->kind is only checked: the block holds no kind.  SCONE_EINVAL (prefixed
 *   "scone_opt_hyper_init: "): what scone_opt_step refuses of a cfg, with step < 0 (any kind) in place of step < 1; a null d_hyper.
 *
 * 3. scone_opt_hyper_advance(h, kind, d_hyper, d_ctl): ONE launch of one thread, once per optimizer step, before the step
 *   kernels.  kind is SCONE_OPT_*; the lean steps advance with SCONE_OPT_SGD (alpha = lr).  d_ctl may be NULL.
 *     d_ctl != NULL and d_ctl->skip != 0:   applied = 0; NOTHING else changes, step included
 *     else, any of the six doubles is inf or NaN, or step == INT64_MAX:   applied = 0, bad = 1; nothing else changes
 *     else:   step = step + 1; sc = scone_opt_hyper_scalars_of's values at the new step; applied = 1; bad = 0
 *   So step counts the steps APPLIED: a step the device skipped does not advance Adam's t or the stochastic bits.  All stores
 *   are plain stores of thread 0.  SCONE_EINVAL: a bad kind, a null d_hyper.
 *
 * 4. scone_opt_step_dh / scone_opt_step_lean_dh: scone_opt_step_dn / scone_opt_step_lean_dn (next section) with the scalars
 *   read from d_hyper->sc, and for SCONE_ROUND_STOCHASTIC the random bits' seed and step read from d_hyper->seed / d_hyper->step (the
 *   step the advance left: the number of this step).  kind (and rounding) come by value; d_n is required -- a caller who knows n
 *   on the host passes a device word that holds it.  Every wavefront first reads `applied`: if it is 0, or d_ctl != NULL and
 *   d_ctl->skip is set, the launch changes NOTHING -- no row, no state, no scale, no status bit.  Otherwise, with d_ctl,
 *   gscale_eff = sc.gscale * coef is ONE fp32 product, as in the _ctl steps.  Contract: every bit of master, state, table and
 *   scales equals scone_opt_step_dn / scone_opt_step_lean_dn given those scalars (and that seed and step): the same kernels,
 *   instantiated for scalars on the device; the block's fields are loaded once per wavefront, before its first row.
 *   ONE launch, no synchronisation, no allocation; n_cap == 0: a no-op.  SCONE_EINVAL: the refusals of the _dn calls that the
 *   host can still check (handle, table, kind, rounding, modes and formats, null pointers and state arrays, a null d_n), plus a
 *   null d_hyper.  What the host can no longer check -- a value that is not finite -- is the advance's `bad`.
 *
 * 5. scone_grad_ctl_set_dh: scone_grad_ctl_set with grad_scale read from d_hyper->grad_scale; the arithmetic and the bits are
 *   the same.  A grad_scale that is inf or NaN on the device gives skip = 1 and coef = 1.0f (the by-value call refuses such a
 *   value; on the device the call can only decline to step).  One launch.  SCONE_EINVAL: as scone_grad_ctl_set, plus a null
 *   d_hyper.
 *
 * Order of a guarded step: scone_grad_sqnorm_dn, scone_grad_ctl_set_dh, scone_opt_hyper_advance(d_ctl), then
 * scone_opt_step_dh / scone_opt_step_lean_dh(d_ctl).  One block may serve several tables or shards: advance ONCE, step each
 * (with steps of the kind the advance was given; SGD and the lean steps share alpha = lr).
 *
 * The stream.  As in the next section: every call that enqueues work takes `stream` last, a hipStream_t passed as void *.
 *
 * Left out, and meant to be: scone_backward_apply_lean in this form, and accumulation in _dn form (see the next section). */
typedef struct scone_opt_hyper {
  /* inputs: written by scone_opt_hyper_init; between steps the caller may overwrite any of them with stream-ordered device
     work of their own (a copy, a fill, a scheduler kernel) */
  double lr, beta1, beta2, eps, weight_decay, grad_scale; /* 0 .. 48 */
  uint64_t seed;                                          /* 48: stochastic rounding only */
  int64_t step;                                           /* 56: t = steps APPLIED so far */
  /* derived by scone_opt_hyper_advance */
  scone_opt_scalars sc;                                   /* 64: the 8 floats the step kernels use */
  uint32_t applied;                                       /* 96: 1 = the last advance advanced */
  uint32_t bad;                                           /* 100: 1 = the last advance found a non-finite input */
} scone_opt_hyper;                                        /* 104 bytes */
int scone_opt_hyper_scalars_of(const scone_opt_cfg *cfg, scone_opt_scalars *out);
int scone_opt_hyper_init(scone_handle *h, const scone_opt_cfg *cfg, uint64_t seed, scone_opt_hyper *d_hyper, void *stream);
int scone_opt_hyper_advance(scone_handle *h, int32_t kind, scone_opt_hyper *d_hyper, const scone_grad_ctl *d_ctl /* may be NULL */,
                            void *stream);
int scone_opt_step_dh(scone_handle *h, int32_t kind, const int64_t *d_row_ids, const float *d_grad_rows, const uint64_t *d_n,
                      uint64_t n_cap, float *d_master, float *d_state1, float *d_state2, const scone_opt_hyper *d_hyper,
                      const scone_grad_ctl *d_ctl, void *stream);
int scone_opt_step_lean_dh(scone_handle *h, int32_t kind, int32_t rounding, const int64_t *d_row_ids, const float *d_grad_rows,
                           const uint64_t *d_n, uint64_t n_cap, float *d_master, float *d_row_state,
                           const scone_opt_hyper *d_hyper, const scone_grad_ctl *d_ctl, void *stream);
int scone_grad_ctl_set_dh(scone_handle *h, const double *d_terms, int32_t n_terms, const scone_opt_hyper *d_hyper, double max_norm,
                          int32_t skip_nonfinite, scone_grad_ctl *d_ctl, void *stream);

/* ---- backward and optimizer step without a host synchronisation: a step that can be captured (new here; appended,
 * SCONE_ABI_VERSION unchanged; every entry point above keeps its bits, its refusals and its place in the stream contract).
 * What it is for: scone_backward_plan reads its counts back (one synchronisation), allocates the partial slots from them and
 * allocates and frees its scratch inside the call, so it is the one call of a training step that keeps the host in lockstep
 * with the device and out of a hipGraph.  The forms below hold the same buffers in a CONTEXT that is allocated once, leave the
 * counts on the device, and give the same bits: plan, rows, norm, control block and optimizer step can be enqueued without the
 * host waiting, and captured once and replayed on new tokens.
 *
 * 1. Context.  scone_backward_ctx_create(h, max_tokens, &ctx) allocates everything a plan of up to max_tokens positions can
 *   need on this handle, in one device allocation: the match records [max_tokens, ELL width] (the context's matcher uses no
 *   stream workspace, so it never allocates either), the build's scratch arrays and rocPRIM's scratch, the plan arrays, and the
 *   partial slots at their worst case.  With R = max_tokens * max_n (max_n + 1) / 2 references at most (R = max_tokens in
 *   longest_suffix mode) and C = scone_backward_chunk(): a row of r > C references has ceil(r / C) <= (r - 1) / C + 1 chunks;
 *   m such rows hold R' <= R references and m <= R' / (C + 1), so their chunks -- the partial slots -- number at most
 *     (R' - m) / C + m  <=  R' / C + (R' / (C + 1)) (C - 1) / C  =  2 R' / (C + 1)  <=  floor(2 R / (C + 1)),
 *   reached when every row has C + 1 references.  scone_backward_ctx_partial_slots(R, &slots) returns floor(2 R / (C + 1))
 *   (no device work; R >= 2^32: SCONE_EINVAL); the context holds min(that, the chunk bound R / C + min(R, owned rows) + 1)
 *   slots of d floats.  The bounds are checked against each other at creation, the counts of a plan against them by
 *   scone_backward_ctx_counts on the host and by every kernel of scone_backward_rows_dn on the device.
 *   scone_backward_ctx_bytes reports the device memory held; scone_backward_ctx_destroy frees it (NULL: a no-op; not while work
 *   that uses the context is in flight).  A context is used by one host thread at a time and belongs to its handle.
 *   SCONE_EINVAL (prefixed "scone_backward_ctx_create: "): what scone_backward_plan refuses of the handle (dim == 0, d % 8 != 0,
 *   2^32 - 1 rows or more), max_tokens < 0, max_tokens > 2^31 - 1 or R >= 2^32, a null out.  Synchronises (it allocates).
 *
 * 2. Plans.  scone_backward_plan_dn (rectangle [B, T]) and scone_backward_plan_varlen_dn (packed, d_cu_seqlens [n_seqs + 1])
 *   build in the context the plan that scone_backward_plan / scone_backward_plan_varlen return for the same batch: the same id
 *   lists, the same stable sort, the same chunks and partial slots -- the same enqueue sequence, over the context's buffers.
 *   No synchronisation, no allocation, no free; the counts (U, the references, the chunks) stay on the device inside the
 *   context.  A new plan overwrites the previous one; stream order protects consumers that are already enqueued, so plans and
 *   their consumers belong on one stream (or are ordered by the caller's events).  B * T == 0, n_seqs == 0 and a batch without a
 *   hit are empty plans: every count is 0.  Capture: a plan whose batch can have more than 2^20 references (B * T * max_n
 *   (max_n + 1) / 2; rocPRIM's merge-sort limit) is REFUSED while `stream` is capturing (SCONE_EINVAL, nothing enqueued): above
 *   that size the sort runs kernels with a private segment, and replaying a graph that holds them faulted on the runtime this
 *   was developed on.  Called eagerly such a plan is as sync-free as any other.  SCONE_ERANGE: more positions than max_tokens.  SCONE_EINVAL: a null ctx / pointer, a
 *   context of another handle, negative sizes, and for the packed form what scone_backward_plan_varlen refuses.  There is NO
 *   form for the caller's CSR lists: scone_backward_plan_csr needs the owned-reference count on the host before it can size
 *   anything, which is the synchronisation this section removes.
 *   scone_backward_ctx_counts(ctx, &n_rows, &n_refs, stream) is the synchronising read of U and the reference count of the
 *   plan last enqueued on `stream` (either pointer may be NULL); SCONE_ESTATE if a count is outside the context's bounds.
 *
 * 3. Rows.  scone_backward_rows_dn(h, ctx, d_grad_out, grad_dtype, reduce, d_row_ids_out, d_grad_rows_out, rows_cap, d_n_out)
 *   writes, with U read on the device,
 *     d_row_ids_out[0, U)    bit for bit what scone_backward_rows writes for a plan of the same batch
 *     d_grad_rows_out[0, U)  likewise bit for bit (the walk of a chunk and the order of the partials are the same code)
 *     *d_n_out               U (ONE uint64 on the device)
 *   Rows [U, rows_cap) of both arrays are not touched.  U > rows_cap: NOTHING is written to the two arrays, *d_n_out = 0 and the
 *   sticky status bit 4 is raised (scone_status); every workgroup of every launch takes this exit before its first store, so
 *   an optimizer step behind it that takes n from d_n_out changes nothing.  At most three launches; their grids are sized from
 *   the host-known bounds of the plan, capped, and walk the device counts grid-stride.  No synchronisation, no allocation.
 *   The partial slots are scratch of the call, as with scone_backward_rows.  SCONE_EINVAL: a null ctx / d_n_out, a context of
 *   another handle, a bad grad_dtype / reduce, a null d_grad_out / output array unless the plan is empty on the host's
 *   knowledge (no positions) or rows_cap == 0.
 *
 * 4. Optimizer steps.  scone_opt_step_dn and scone_opt_step_lean_dn are scone_opt_step / scone_opt_step_lean -- or, with
 *   d_ctl != NULL, scone_opt_step_ctl / scone_opt_step_lean_ctl -- with n = min(*d_n, n_cap), read on the device by every
 *   wavefront (a scalar load) before it touches a row; d_row_ids / d_grad_rows have room for n_cap rows.  The same kernels,
 *   instantiated for a count on the device: every bit of master, state, table and scales equals the by-value call with that n.
 *   ONE launch (grid sized from n_cap as the by-value call sizes it from n), no synchronisation, no allocation.  n_cap == 0: a
 *   no-op.  The refusals of the by-value calls, plus a null d_n.
 *
 * 5. Squared norm.  scone_grad_sqnorm_dn(h, d_grad_rows, d_n, n_cap, d_scratch, d_sq_out): d_scratch holds
 *   scone_grad_sqnorm_scratch(n_cap) doubles -- Q_r at [0, n_cap), the tile sums behind them.  With n = min(*d_n, n_cap),
 *   *d_sq_out and Q_r, r < n, have the bits scone_grad_sqnorm(n) gives.  Proof: Q_r is computed per row by the same code.  The
 *   call reduces the ceil(n_cap / 1024) tiles of the capacity, of which the first ceil(n / 1024) are those of
 *   scone_grad_sqnorm(n): a thread's partial sum of a tile adds the rows r < n it owns in the same order, and a tile past n adds
 *   nothing, so its tree yields +0.0.  In the total, thread t adds P_(t + 256 i) in ascending i: the tiles of the by-value call
 *   first, then +0.0 terms.  Every sum here starts at +0.0 and holds only squares and sums of squares, so it is never -0.0, and
 *   x + (+0.0) has the bits of x for every such x (NaN and +inf included).  The tree that follows is the same.  Three launches,
 *   no synchronisation, no allocation.  Q_r, r >= n, is not written.  SCONE_EINVAL: as scone_grad_sqnorm, plus a null d_n.
 *   scone_grad_ctl_set is unchanged: it never took a count.
 *
 * The stream.  Every call of this section that enqueues work takes `stream` last: a hipStream_t passed as void * (what
 * scone_stream_t is; NULL = the default stream), the stream all of its device work is enqueued on.
 *
 * Scalars under capture.  The steps of THIS section take their hyper-parameters by value (scone_opt_scalars_of /
 * scone_lean_scalars_of run on the host): lr, grad_scale, Adam's step t inside alpha and the stochastic rounding's `step` are
 * part of a captured launch and a replayed graph repeats them AS CAPTURED.  The section "optimizer hyper-parameters on the
 * device" in front of this one keeps them in a block on the device instead: scone_opt_step_dh / scone_opt_step_lean_dh are
 * the steps of this section with the scalars read there, and every kind and rounding can be captured.
 *
 * Left out, and meant to be: scone_backward_apply_lean in this form (the fused backward + lean step still takes a
 * scone_bwd_plan), and accumulation (scone_backward_rows_acc, scone_grad_merge_*) in this form -- a step that accumulates over
 * micro-batches takes the by-value road. */
typedef struct scone_bwd_ctx scone_bwd_ctx;
int scone_backward_ctx_partial_slots(uint64_t max_refs, uint64_t *slots);
int scone_backward_ctx_create(scone_handle *h, int64_t max_tokens, scone_bwd_ctx **out);
int scone_backward_ctx_bytes(scone_bwd_ctx *ctx, uint64_t *bytes);
void scone_backward_ctx_destroy(scone_bwd_ctx *ctx);
int scone_backward_plan_dn(scone_handle *h, scone_bwd_ctx *ctx, const int32_t *d_tok, int32_t B, int32_t T, void *stream);
int scone_backward_plan_varlen_dn(scone_handle *h, scone_bwd_ctx *ctx, const int32_t *d_tok, const int32_t *d_cu_seqlens,
                                  int32_t n_seqs, int64_t total_tokens, void *stream);
int scone_backward_ctx_counts(scone_bwd_ctx *ctx, uint64_t *h_n_rows, uint64_t *h_n_refs, void *stream);
int scone_backward_rows_dn(scone_handle *h, scone_bwd_ctx *ctx, const void *d_grad_out, int32_t grad_dtype, int32_t reduce,
                           int64_t *d_row_ids_out, float *d_grad_rows_out, uint64_t rows_cap, uint64_t *d_n_out,
                           void *stream);
int scone_opt_step_dn(scone_handle *h, const scone_opt_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                      const uint64_t *d_n, uint64_t n_cap, float *d_master, float *d_state1, float *d_state2,
                      const scone_grad_ctl *d_ctl, void *stream);
int scone_opt_step_lean_dn(scone_handle *h, const scone_lean_cfg *cfg, const int64_t *d_row_ids, const float *d_grad_rows,
                           const uint64_t *d_n, uint64_t n_cap, float *d_master, float *d_row_state, const scone_grad_ctl *d_ctl,
                           void *stream);
int scone_grad_sqnorm_dn(scone_handle *h, const float *d_grad_rows, const uint64_t *d_n, uint64_t n_cap, double *d_scratch,
                         double *d_sq_out, void *stream);

/* ---- the fused lookup at CHOSEN positions only (new here: the reference recomputes a window on the host, engine.py:151-170).
 * What it is for: a serving loop wants few rows matched against context that is already on the device -- the last token of
 * every sequence in a decoding step, the last k tokens in a speculative-verify step, the new chunk of a chunked prefill.
 *   for j in [0, n_sel), p = d_sel[j]:  out[j,:] = exactly the bits the full lookup over the same tokens writes to its row p
 * d_cu_seqlens == NULL: the tokens are a rectangle, rows of T tokens (total_tokens % T == 0; n_seqs ignored) -- scone_embed's
 * batch.  d_cu_seqlens given: the packed stream of scone_embed_varlen ([n_seqs + 1] int32 on the device), T ignored.  All rules
 * of the full lookup hold: the id list in the reference's order, the sequential fp32 sum, the IEEE mean, zero-fill for K = 0,
 * (base row + fg) + wpe, both lookup modes, the row_begin / row_end ownership rule with divisor = full K.
 * Everything per OUTPUT is indexed by j, not by p: d_base is [n_sel, d] in out_dtype and row j is the base of output j (the
 * caller holds embeddings of the selected tokens only); d_pos is int32 [n_sel], or NULL for the place of p inside its sequence;
 * d_out is [n_sel, d].  d_wte / vocab: the base row is wte[tok[p]] as in scone_embed.  d_wte and d_base together: SCONE_EINVAL;
 * neither: the term is omitted.  d_out == d_base is the defined in-place call, any other overlap of the two [n_sel, d] ranges
 * returns SCONE_EINVAL.  d_sel may be unsorted and may repeat positions: each j is written on its own.  For d_sel[j] outside
 * [0, total_tokens) nothing is read, row j is NOT written and SCONE_ST_BAD_TOKEN is raised.  Whatever d_cu_seqlens holds, no
 * token outside d_tok[0, total_tokens) is read.  Token / position ids out of range: as scone_embed ("Ids out of range"), for the
 * token tok[d_sel[j]] and the position id of OUTPUT j; a bad id at a position that is not selected raises nothing.
 * n_sel comes from the host: ONE launch of ceil(n_sel / 4) workgroups for every n_sel that fits a grid, at every d % 8 == 0
 * and every table format (d = 768 / 1024 / 1280 specialised, any other dim -- and INT4 / MXFP4 at 768 / 1280 -- walked in
 * units of 8 elements); no workspace, no lock, no synchronisation; thread-safe like scone_embed.  n_sel == 0 or
 * total_tokens == 0 (or a packed batch of n_seqs == 0): a no-op.
 * What it is NOT for: n_sel comparable to total_tokens.  A wavefront probes every candidate window of its token, like the
 * one-launch road of scone_embed; above that road's measured crossover (32768 tokens) the full lookup, one probe per window,
 * is the faster way to most of a batch.
 * SCONE_EINVAL (scone_last_error names the reason): a null d_tok / d_sel / d_out, negative sizes, total_tokens > 2^31 - 1, a
 * rectangle with T <= 0 or total_tokens % T != 0, a bad reduce / out_dtype, d_wte with vocab <= 0, d_wpe with n_pos <= 0,
 * d % 8 != 0, a pinned-host table created with stage_tokens > 0 (tables read in place from pinned host memory work). */
int scone_embed_select(scone_handle *h, const int32_t *d_tok, int64_t total_tokens, int32_t T,
                       const int32_t *d_cu_seqlens, int32_t n_seqs,
                       const int32_t *d_sel, int64_t n_sel,
                       const void *d_wte, int64_t vocab, const void *d_base,
                       const void *d_wpe, int64_t n_pos, const int32_t *d_pos,
                       int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONE_HIP_H */
