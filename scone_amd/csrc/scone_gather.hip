// The bandwidth-bound core: sparse row gather + dequantise + ordered fp32 reduce +
// combine with the base token / position embeddings.  No MFMA: every byte fetched
// is used once; the kernel is priced against the HBM roofline.
//
// Replaces, on the GPU:
//   EmbeddingCache.get_token_embeddings / get_embeddings  scone/inference/embedding_cache.py:113-181
//   embeddings.mean(dim=0), zero-fill, .half()            scone/inference/engine.py:247-266
//   wte(input_ids) + f_gram_embeddings + wpe(position_ids) scone/models/language_model.py:239-254
//
// This file holds the entry points (scone_embed, scone_gather_reduce, scone_embed_partial, scone_finalize, the embed
// halves of the shard exchanges) and the staged-prefetch driver; the kernels are in scone_embed_wave.h (wave per token:
// every d % 8 == 0) and scone_gather_impl.h (k_embed, the lane-group fallback for other dims: a group of LPT lanes owns
// one token, each lane 16-byte vectors of every row).  Accumulation is sequential in the reference's list order in
// fp32 everywhere, so results do not depend on the launch geometry.
//
// Host path.  Every entry point is its argument checks, in its own order (tests/test_gpu_entry_errors.py pins the order and
// the texts), and then the pieces below: lookup_args / combine / slice build the embed_args, match_into gives the stream's
// workspace its records, profiled brackets the launch, launch_fmt / launch_select pick the table format's translation unit.
#include "scone_gather_impl.h"
#include "scone_embed_select.h"
#include "scone_embed_rows.h"
#ifdef SCONE_PROBE_PERM
#include <cstdlib>
#endif

using namespace scone_gather;

// One-launch limit (scone_handle::fused_max_tokens, default 32768): measured crossover (round 2's tools/latency.py; now bench.py's `latency` block) -- 8K tokens
// 15.5 -> 9.9 us, 16K 20.5 -> 16.8, 32K 30.2 -> 29.3, 64K 45.7 -> 53.7: above it the two-kernel form wins (one probe per
// window, not per covered token).

namespace {

int launch_fmt(scone_handle *h, const embed_args &a, int src, int mode, int out_dtype, hipStream_t s) {
  if (mode == MODE_FINALIZE) return launch_f32(h, a, src, mode, out_dtype, s);
  switch (h->cfg.table_fmt) {
    case SCONE_FMT_F32: return launch_f32(h, a, src, mode, out_dtype, s);
    case SCONE_FMT_F16: return launch_f16(h, a, src, mode, out_dtype, s);
    case SCONE_FMT_I8: return launch_i8(h, a, src, mode, out_dtype, s);
    case SCONE_FMT_I4: return launch_i4(h, a, src, mode, out_dtype, s);
    case SCONE_FMT_BF16: return launch_bf16(h, a, src, mode, out_dtype, s);
    case SCONE_FMT_MXFP4: return launch_mxfp4(h, a, src, mode, out_dtype, s);
    default: return scone_fail(h, SCONE_EINVAL, "unknown table_fmt");
  }
}
int launch_select(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s) {
  switch (h->cfg.table_fmt) {
    case SCONE_FMT_F32: return launch_select_f32(h, a, out_dtype, s);
    case SCONE_FMT_F16: return launch_select_f16(h, a, out_dtype, s);
    case SCONE_FMT_I8: return launch_select_i8(h, a, out_dtype, s);
    case SCONE_FMT_I4: return launch_select_i4(h, a, out_dtype, s);
    case SCONE_FMT_BF16: return launch_select_bf16(h, a, out_dtype, s);
    case SCONE_FMT_MXFP4: return launch_select_mxfp4(h, a, out_dtype, s);
    default: return scone_fail(h, SCONE_EINVAL, "unknown table_fmt");
  }
}
// The launch (a callable returning a status; the packed lookup's launches twice) between the profiling calls, which are no-ops
// unless profiling is on.  A template, not std::function: this runs in front of lookups of about 10 us.
template <typename Launch>
int profiled(scone_handle *h, hipStream_t s, Launch &&launch) {
  SCONE_TRY(scone_prof_begin(h, s));
  const int rc = launch();
  if (rc) {
    scone_prof_abort(h);
    return rc;
  }
  return scone_prof_end(h, s);
}

// formats / dims served by k_embed_wave (scone_embed_wave.h: wave_geom<>::OK)
bool scone_wave_kernel_covers(int fmt, int d) {
  (void)fmt;
  return d % 8 == 0;  // specialised kernels for 768 / 1024 / 1280, the unit-walking kernel otherwise
}

void fill_table_view(const scone_handle *h, table_view &tv) {
  tv.st = scone_store_of(h);
  tv.scales = reinterpret_cast<const __half *>(h->scales);
  tv.row_begin = (long long)h->cfg.row_begin;
  tv.row_end = (long long)h->cfg.row_end;
  tv.n_rows = (long long)h->cfg.n_rows;
  tv.row_bytes = (int)h->row_payload_bytes;
  tv.d = h->cfg.dim;
}

// What a lookup of ntok tokens, walked as rows of T, takes from the handle: the table, the zero row, the lookup mode, the status word.
embed_args lookup_args(const scone_handle *h, long long ntok, int T) {
  embed_args a = {};
  fill_table_view(h, a.tv);
  a.BT = ntok, a.ntok = ntok, a.T = T, a.max_n = h->cfg.max_n;
  a.zero_row = h->d_zero_row, a.mode = (int)h->cfg.lookup_mode, a.status = h->d_status;
  return a;
}
// ... and from the caller: what is added to the reduced f-gram rows (d_base: the dense base of scone_embed_base, in the place of wte[tok])
void combine(embed_args &a, const int32_t *d_tok, const int32_t *d_pos, const void *d_wte, int64_t vocab, const void *d_base,
             const void *d_wpe, int64_t n_pos, int32_t reduce, void *d_out) {
  a.tok = d_tok, a.pos = d_pos, a.wte = d_wte, a.vocab = vocab, a.wpe = d_wpe, a.n_pos = n_pos, a.base = d_base;
  a.reduce = reduce, a.out = d_out;
}
// The same lookup on tokens [t0, t0 + ntok) of a's: tok, pos, the id records, out and the dense base (same rows as out) move together.
embed_args slice(const embed_args &a, long long t0, long long ntok, int out_dtype) {
  const size_t row0 = (size_t)t0 * a.tv.d * scone_dt_bytes(out_dtype);
  embed_args r = a;
  r.BT = ntok, r.ntok = ntok;
  r.tok = a.tok + t0;
  if (a.pos) r.pos = a.pos + t0;
  if (a.ell) r.ell = a.ell + t0 * SCONE_ELL_W(a.max_n);
  r.out = reinterpret_cast<uint8_t *>(a.out) + row0;
  if (a.base) r.base = reinterpret_cast<const uint8_t *>(a.base) + row0;
  return r;
}

// The match of a [B, T] batch into the stream's workspace, in the record form this table's lookup kernels read.
int match_into(scone_handle *h, scone_ws *w, int32_t B, int32_t T, embed_args &a, hipStream_t s) {
  if (scone_wave_kernel_covers(h->cfg.table_fmt, h->cfg.dim)) {
    // fast path: per-token id records (one scalar load per token in the gather kernel)
    SCONE_TRY(scone_ensure_ell(h, w, a.BT));
    SCONE_TRY(scone_launch_match_ell(h, a.tok, B, T, w->d_ell, s));
    a.ell = w->d_ell;
  } else {
    SCONE_TRY(scone_ensure_hits(h, w, a.BT));
    SCONE_TRY(scone_launch_match(h, a.tok, B, T, w->d_hits, s));
    a.hits = w->d_hits;
  }
  return SCONE_OK;
}

// ---- argument checks, each stated once; `who` is the entry point's name in the message
int check_shape(scone_handle *h, const char *who, int32_t B, int32_t T) {
  return B < 0 || T < 0 ? scone_refuse(h, SCONE_EINVAL, who, "negative B or T") : SCONE_OK;
}
int check_reduce(scone_handle *h, const char *who, int32_t reduce) {
  return reduce != SCONE_REDUCE_MEAN && reduce != SCONE_REDUCE_SUM ? scone_refuse(h, SCONE_EINVAL, who, "bad reduce") : SCONE_OK;
}
int check_out_dtype(scone_handle *h, const char *who, int32_t out_dtype) {
  if (out_dtype == SCONE_DT_F32 || out_dtype == SCONE_DT_F16 || out_dtype == SCONE_DT_BF16) return SCONE_OK;
  return scone_refuse(h, SCONE_EINVAL, who, "bad out_dtype");
}
int check_wte_wpe(scone_handle *h, const char *who, const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos) {
  if ((d_wte && vocab <= 0) || (d_wpe && n_pos <= 0)) return scone_refuse(h, SCONE_EINVAL, who, "wte/wpe given without vocab/n_pos");
  return SCONE_OK;
}
int check_wpe(scone_handle *h, const char *who, const void *d_wpe, int64_t n_pos) {
  return d_wpe && n_pos <= 0 ? scone_refuse(h, SCONE_EINVAL, who, "wpe given without n_pos") : SCONE_OK;
}
int check_total(scone_handle *h, const char *who, int64_t total_tokens) {
  return total_tokens > 0x7FFFFFFFll ? scone_refuse(h, SCONE_EINVAL, who, "total_tokens above 2^31 - 1") : SCONE_OK;
}
// out == base is the in-place call (a wave reads the words of row p in the lanes that store them); any other overlap of the
// two [n, d] ranges would let one wave's store reach a row another wave has not read yet.
int check_base(scone_handle *h, const char *who, const void *d_base, const void *d_out, long long n, int32_t out_dtype) {
  const unsigned long long bytes = (unsigned long long)n * h->cfg.dim * scone_dt_bytes(out_dtype);
  const unsigned long long b = (unsigned long long)reinterpret_cast<uintptr_t>(d_base), o = (unsigned long long)reinterpret_cast<uintptr_t>(d_out);
  if (b != o && b < o + bytes && o < b + bytes)
    return scone_refuse(h, SCONE_EINVAL, who, "d_base overlaps d_out (only d_out == d_base, the in-place call, is defined)");
  return SCONE_OK;
}
bool is_staged(const scone_handle *h) { return h->cfg.stage_tokens && h->rows_host; }
// what both packed entry points check before an empty batch returns
int check_packed(scone_handle *h, const char *who, int32_t n_seqs, int64_t total_tokens, int32_t reduce, int32_t out_dtype) {
  if (n_seqs < 0 || total_tokens < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative n_seqs or total_tokens");
  SCONE_TRY(check_total(h, who, total_tokens));
  SCONE_TRY(check_reduce(h, who, reduce));
  SCONE_TRY(check_out_dtype(h, who, out_dtype));
  if (h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0 (the lane-group fallback reads another record form)");
  if (is_staged(h))
    return scone_refuse(h, SCONE_EINVAL, who, "not for stage_tokens > 0 (the staging pipeline chunks whole rectangular sequences)");
  return SCONE_OK;
}
int check_mode(scone_handle *h, const char *who) {
  if (h->cfg.lookup_mode == SCONE_MODE_COVER) return SCONE_OK;
  if (h->cfg.lookup_mode == SCONE_MODE_LONGEST_SUFFIX && scone_wave_kernel_covers(h->cfg.table_fmt, h->cfg.dim)) return SCONE_OK;
  return scone_refuse(h, SCONE_EINVAL, who, "lookup_mode longest_suffix needs d % 8 == 0");
}

// decode-size batches are launch-bound: one fused launch (k_embed_fused) instead of match + gather
// (INT4 has no specialised kernel at d = 768 / 1280: a row segment would be narrower than one 16-B access; MXFP4 has INT4's
// payload geometry and follows the same rule)
bool scone_embed_takes_one_launch(const scone_handle *h, long long BT) {
  return BT <= h->fused_max_tokens && (h->cfg.dim == 768 || h->cfg.dim == 1024 || h->cfg.dim == 1280) &&
         !((h->cfg.table_fmt == SCONE_FMT_I4 || h->cfg.table_fmt == SCONE_FMT_MXFP4) && h->cfg.dim != 1024);
}

#ifdef SCONE_PROBE_PERM
// TRAFFIC PROBE of a token-ordered ("run-ordered") lookup (tools/run_order_probe.py; a -DSCONE_PROBE_PERM build only, never the
// shipped library).  The caller's process puts the device address of a permutation perm[B*T] into the environment
// (SCONE_PROBE_PERM_PTR); scone_embed then looks up, at slot j of the launch, the token of position perm[j] -- its id record,
// token id and position row -- and stores the result to out[j].  Every vector is the right one for SOME position, only its
// place in `out` is permuted: the bytes the kernel moves are those of a kernel that visits the positions in the order the
// permutation gives, which is what the probe measures (FETCH_SIZE, kernel time).
__global__ void k_probe_permute(const int32_t *__restrict__ perm, const int32_t *__restrict__ ell, const int32_t *__restrict__ tok,
                                int32_t *__restrict__ ell2, int32_t *__restrict__ tok2, int32_t *__restrict__ pos2, long long BT,
                                int T, int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long j = t / W;
  const int w = (int)(t % W);
  if (j >= BT) return;
  const long long p = perm[j];
  ell2[j * W + w] = ell[p * W + w];
  if (w == 0) tok2[j] = tok[p], pos2[j] = (int32_t)(p % T);
}
static int32_t *g_probe_buf = nullptr;
static long long g_probe_cap = 0;
#endif

}  // namespace

// Pinned-host table, prefetch through the persistent HBM cache of cold rows (scone_stage.hip): chunks of whole sequences;
// side streams prepare chunk c+2 and copy the rows chunk c+1 misses while the caller's stream reduces chunk c out of
// [hot head | cache].
// chunk geometry of a staged batch: sequences per chunk (0 = a sequence does not fit a chunk)
static int staged_geometry(scone_handle *h, int32_t B, int32_t T, long long *seqs_out) {
  long long seqs = (long long)h->cfg.stage_tokens / T;
  if (seqs < 1) seqs = 1;
  if (seqs > B) seqs = B;
  SCONE_TRY(scone_stage_prepare(h, seqs * T));
  seqs = scone_stage_chunk_tokens(h) / T;
  if (seqs < 1) return scone_fail(h, SCONE_EINVAL, "scone_embed(staged): sequence too long for one staging chunk");
  if (seqs > B) seqs = B;
  *seqs_out = seqs;
  return SCONE_OK;
}

static int embed_staged_chunks(scone_handle *h, const embed_args &full, int32_t B, int32_t T, int32_t out_dtype, hipStream_t s) {
  long long seqs = 0;
  SCONE_TRY(staged_geometry(h, B, T, &seqs));
  SCONE_TRY(scone_stage_bind(h, s));
  const long long nchunks = (B + seqs - 1) / seqs;
  auto chunk_b = [&](long long c) { return (int32_t)((c + 1) * seqs <= B ? seqs : B - c * seqs); };
  // chunks scone_embed_prefetch prepared for exactly this batch are taken over (their side-stream work was ordered behind the
  // stream the caller named THEN); otherwise the side stream starts after everything already queued on the caller's stream
  // (tokens may be produced there)
  long long staged = scone_stage_take_prefetched(h, full.tok, B, T, seqs);
  if (staged == 0) {
    SCONE_HIP(h, hipEventRecord(scone_stage_start_event(h), s));
    SCONE_HIP(h, hipStreamWaitEvent(scone_stage_side(h), scone_stage_start_event(h), 0));
  }
  // chunks 0 .. AHEAD-1 are staged ahead; inside the loop chunk c + AHEAD is queued before chunk c is reduced
  for (; staged < nchunks && staged < SCONE_STAGE_AHEAD; ++staged) SCONE_TRY(scone_stage_chunk(h, full.tok + staged * seqs * T, chunk_b(staged), T));
  for (long long c = 0; c < nchunks; ++c) {
    if (staged < nchunks && staged <= c + SCONE_STAGE_AHEAD) {  // (its set was last used by a chunk whose lookup is already queued)
      SCONE_TRY(scone_stage_chunk(h, full.tok + staged * seqs * T, chunk_b(staged), T));
      ++staged;
    }
    const int buf = scone_stage_consume_buf(h);
    embed_args a = slice(full, c * seqs * T, (long long)chunk_b(c) * T, out_dtype);
    a.ell = scone_stage_ell(h, buf);
    a.tv.st.cold = scone_stage_rows(h);  // the records now hold n_hot + cache slot: the cold half of the row store is the cache
    if (h->scale_bytes_per_row) a.tv.scales = reinterpret_cast<const __half *>(scone_stage_scales(h));
    SCONE_HIP(h, hipStreamWaitEvent(s, scone_stage_staged_event(h, buf), 0));
    SCONE_TRY(profiled(h, s, [&] { return launch_fmt(h, a, SRC_HITS, MODE_FULL, out_dtype, s); }));
    SCONE_TRY(scone_stage_mark_consumed(h, buf, s));
  }
  return SCONE_OK;
}

// One staging pipeline per handle: the whole call holds stage_mu (calls from several host threads are serialised; on the
// device their chunks follow each other through the pipeline's events like those of consecutive calls from one thread).  A
// call that fails after chunks were prepared drops the whole pipeline (scone_stage_resync): the next call starts a cold cache.
static int embed_staged(scone_handle *h, const embed_args &full, int32_t B, int32_t T, int32_t out_dtype, hipStream_t s) {
  std::lock_guard<std::mutex> g(h->stage_mu);
  const int rc = embed_staged_chunks(h, full, B, T, out_dtype, s);
  if (rc && h->stage) scone_stage_resync(h);
  return rc;
}

// The north-star's "async prefetch" as an entry point: the first chunks of the NEXT batch are matched, placed and copied on the
// side streams now -- behind `stream`, where its tokens are (or were) produced -- so that the scone_embed of that batch finds them
// done.  A no-op for tables without a prefetch pipeline.
extern "C" int scone_embed_prefetch(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t tokens_ready,
                                    scone_stream_t stream) {
  const char *who = "scone_embed_prefetch";
  SCONE_TRY(scone_need_table(h, who));
  SCONE_TRY(check_shape(h, who, B, T));
  if ((long long)B * T == 0) return SCONE_OK;
  if (!d_tok) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  if (!scone_wave_kernel_covers(h->cfg.table_fmt, h->cfg.dim)) return SCONE_OK;
  SCONE_ON_DEVICE(h);
  // Rows in HBM (or read in place over PCIe): nothing to do.  What could run ahead there is the match of the next batch; built
  // and measured in round 5 (k_match_ell on a side stream of the handle beside the previous gather, 2-4 record buffers, every
  // stream priority): 1-19 % SLOWER than match-then-gather on one stream at every batch size from 33k to 1M tokens -- the
  // gather kernel holds every wave slot of the chip, a match workgroup only gets in where a gather workgroup retires, and
  // the gather loses exactly the time the match takes (profiles/r05b, profiles/r05c; the implementation is kept there as a
  // diff).  Removed.
  if (!is_staged(h)) return SCONE_OK;
  std::lock_guard<std::mutex> g(h->stage_mu);
  long long seqs = 0;
  SCONE_TRY(staged_geometry(h, B, T, &seqs));
  SCONE_TRY(scone_stage_bind(h, (hipStream_t)stream));
  (void)scone_stage_take_prefetched(h, nullptr, -1, -1, -1);  // an earlier prefetch that was never used is dropped
  const long long nchunks = (B + seqs - 1) / seqs;
  if (!tokens_ready) {  // behind whatever is queued on `stream` -- a lookup queued there just before this call included
    SCONE_HIP(h, hipEventRecord(scone_stage_start_event(h), (hipStream_t)stream));
    SCONE_HIP(h, hipStreamWaitEvent(scone_stage_side(h), scone_stage_start_event(h), 0));
  }
  long long n = 0;
  for (; n < nchunks && n < SCONE_STAGE_AHEAD; ++n) {
    const int32_t bc = (int32_t)((n + 1) * seqs <= B ? seqs : B - n * seqs);
    const int rc = scone_stage_chunk(h, d_tok + n * seqs * T, bc, T);
    if (rc) {
      scone_stage_resync(h);
      return rc;
    }
  }
  return scone_stage_note_prefetched(h, d_tok, B, T, seqs, n);
}

extern "C" int scone_gather_reduce(scone_handle *h, const int32_t *d_offsets, const int32_t *d_ids, int64_t ntok,
                                   const void *d_base, int32_t reduce, void *d_out, int32_t out_dtype,
                                   scone_stream_t stream) {
  const char *who = "scone_gather_reduce";
  SCONE_TRY(scone_need_table(h, who));
  if (ntok < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative ntok");
  if (ntok == 0) return SCONE_OK;
  if (!d_offsets || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_TRY(check_reduce(h, who, reduce));
  SCONE_ON_DEVICE(h);
  embed_args a = lookup_args(h, ntok, (int)(ntok > 0x7FFFFFFF ? 0x7FFFFFFF : ntok));
  combine(a, nullptr, nullptr, nullptr, 0, d_base, nullptr, 0, reduce, d_out);
  a.offsets = d_offsets, a.ids = d_ids;
  a.mode = SCONE_MODE_COVER;  // the caller's lists are reduced as they stand: the lookup mode belongs to the match
  return launch_fmt(h, a, SRC_CSR, MODE_FULL, out_dtype, (hipStream_t)stream);
}

// The rectangular lookup behind scone_embed (a.base == NULL: the base row of a token is wte[tok]) and scone_embed_base (a dense
// base [B*T, d]: the base row of position p is base[p]; the kernels take it in their wte parameter, wave_params::vocab < 0).
// Arguments are validated by the two entry points.
static int embed_rect(scone_handle *h, embed_args &a, int32_t B, int32_t T, int32_t out_dtype, hipStream_t s) {
  SCONE_TRY(check_mode(h, "scone_embed"));
  if (is_staged(h)) {
    if (!scone_wave_kernel_covers(h->cfg.table_fmt, h->cfg.dim))
      return scone_fail(h, SCONE_EINVAL, "scone_embed: staged prefetch needs d % 8 == 0");
    return embed_staged(h, a, B, T, out_dtype, s);
  }
  auto launch = [&] { return launch_fmt(h, a, SRC_HITS, MODE_FULL, out_dtype, s); };
  if (scone_embed_takes_one_launch(h, a.BT)) {
    a.fused = 1;
    return profiled(h, s, launch);
  }
  // the workspace of THIS stream, held while the match that writes it and the lookup that reads it are enqueued
  scone_ws_lock ws(scone_ws_acquire(h, s));
  if (!ws.w) return scone_fail(h, SCONE_ENOMEM, "scone_embed: out of memory");
  SCONE_TRY(match_into(h, ws.w, B, T, a, s));
#ifdef SCONE_PROBE_PERM
  if (const char *e = getenv("SCONE_PROBE_PERM_PTR")) {
    const int32_t *perm = reinterpret_cast<const int32_t *>(strtoull(e, nullptr, 0));
    const int W = h->cfg.max_n <= 3 ? 8 : 16;
    const long long BT = a.BT;
    if (perm && a.ell && !a.pos && !a.base) {
      if (g_probe_cap < BT) {
        if (g_probe_buf) (void)hipFree(g_probe_buf);
        SCONE_HIP(h, hipMalloc(&g_probe_buf, (size_t)BT * (W + 2) * sizeof(int32_t)));
        g_probe_cap = BT;
      }
      int32_t *ell2 = g_probe_buf, *tok2 = g_probe_buf + BT * W, *pos2 = tok2 + BT;
      const long long n = BT * W;
      hipLaunchKernelGGL(k_probe_permute, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, perm, a.ell, a.tok, ell2, tok2, pos2,
                         BT, T, W);
      a.ell = ell2, a.tok = tok2, a.pos = pos2;
    }
  }
#endif
  return profiled(h, s, launch);
}

extern "C" int scone_embed(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, const void *d_wte,
                           int64_t vocab, const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce,
                           void *d_out, int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_embed";
  SCONE_TRY(scone_need_table(h, who));
  SCONE_TRY(check_shape(h, who, B, T));
  if ((long long)B * T == 0) return SCONE_OK;
  if (!d_tok || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_TRY(check_reduce(h, who, reduce));
  SCONE_TRY(check_wte_wpe(h, who, d_wte, vocab, d_wpe, n_pos));
  SCONE_ON_DEVICE(h);
  embed_args a = lookup_args(h, (long long)B * T, T);
  combine(a, d_tok, d_pos, d_wte, vocab, nullptr, d_wpe, n_pos, reduce, d_out);
  return embed_rect(h, a, B, T, out_dtype, (hipStream_t)stream);
}

// Dense base (new here): the caller already holds its token embeddings (the inputs_embeds of language_model.py:239-243).
extern "C" int scone_embed_base(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, const void *d_base,
                                const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce, void *d_out,
                                int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_embed_base";
  SCONE_TRY(scone_need_table(h, who));
  SCONE_TRY(check_shape(h, who, B, T));
  SCONE_TRY(check_reduce(h, who, reduce));
  SCONE_TRY(check_out_dtype(h, who, out_dtype));
  const long long BT = (long long)B * T;
  if (BT == 0) return SCONE_OK;
  if (!d_tok || !d_base || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_tok, d_base and d_out are required)");
  SCONE_TRY(check_wpe(h, who, d_wpe, n_pos));
  SCONE_TRY(check_base(h, who, d_base, d_out, BT, out_dtype));
  SCONE_ON_DEVICE(h);
  embed_args a = lookup_args(h, BT, T);
  combine(a, d_tok, d_pos, nullptr, 0, d_base, d_wpe, n_pos, reduce, d_out);
  return embed_rect(h, a, B, T, out_dtype, (hipStream_t)stream);
}

// The packed lookup behind scone_embed_varlen and scone_embed_base_varlen (a.base: as in embed_rect); `a` spans the whole stream.
// Two-kernel form: k_match_ell_varlen (scone_index.hip) knows the sequence boundaries and leaves
// one id record and one position per token; from there on nothing depends on where a sequence begins, so the large-batch
// kernels run unchanged with explicit positions and (B, T) as a mere TRAVERSAL of the packed stream.  Measured on the headline
// table (tools/varlen_compare.py, profiles/r08b): the whole stream as ONE row (B = 1, T = total: a wave per token, 4
// consecutive tokens per workgroup, no walk) 765 us per 1M tokens, rows of 128 / 512 / 2048 tokens walked by persistent
// workgroups 792 / 778 / 780 us -- with per-token positions a walk has no position row to keep, and the hardware's own
// workgroup dispatch balances better than the fixed runs.  So: one row.  SCONE_VARLEN_T=<T'> (scone_handle::varlen_t, A/B runs
// and tests) takes [total / T', T'] plus one launch for the total % T' tokens left over; streams above 2^25 tokens take
// T' = 512 (one workgroup per 4 tokens would not fit a grid).  Decode-size batches: k_embed_fused<VARLEN>, one launch.
static int embed_packed(scone_handle *h, embed_args &a, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t out_dtype, hipStream_t s) {
  const long long total = a.BT;
  if (scone_embed_takes_one_launch(h, total)) {
    a.fused = 1, a.cu = d_cu_seqlens, a.n_seqs = n_seqs;
    return profiled(h, s, [&] { return launch_fmt(h, a, SRC_HITS, MODE_FULL, out_dtype, s); });
  }
  // the workspace of THIS stream, held while the match that writes it and the lookups that read it are enqueued
  scone_ws_lock ws(scone_ws_acquire(h, s));
  if (!ws.w) return scone_fail(h, SCONE_ENOMEM, "scone_embed_varlen: out of memory");
  SCONE_TRY(scone_ensure_ell(h, ws.w, total));
  int32_t *vpos = nullptr;
  if (a.wpe && !a.pos) {  // default positions p - cu[s]: written by the match
    SCONE_TRY(scone_ensure_vpos(h, ws.w, total));
    vpos = ws.w->d_vpos;
    a.pos = vpos;
  }
  SCONE_TRY(scone_launch_match_ell_varlen(h, a.tok, d_cu_seqlens, n_seqs, total, ws.w->d_ell, vpos, s));
  a.ell = ws.w->d_ell;
  const long long row = h->varlen_t > 0 ? h->varlen_t : (total <= (1ll << 25) ? total : 512);
  const long long Tp = total < row ? total : row;
  const long long main_tok = total / Tp * Tp;
  return profiled(h, s, [&] {
    embed_args m = slice(a, 0, main_tok, out_dtype);
    m.T = (int)Tp;
    int rc = launch_fmt(h, m, SRC_HITS, MODE_FULL, out_dtype, s);
    if (!rc && main_tok < total) {
      embed_args r = slice(a, main_tok, total - main_tok, out_dtype);
      r.T = (int)r.BT;
      rc = launch_fmt(h, r, SRC_HITS, MODE_FULL, out_dtype, s);
    }
    return rc;
  });
}

extern "C" int scone_embed_base_varlen(scone_handle *h, const int32_t *d_tok, const int32_t *d_cu_seqlens, int32_t n_seqs,
                                       int64_t total_tokens, const void *d_base, const void *d_wpe, int64_t n_pos,
                                       const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype,
                                       scone_stream_t stream) {
  const char *who = "scone_embed_base_varlen";
  SCONE_TRY(scone_need_table(h, who));
  SCONE_TRY(check_packed(h, who, n_seqs, total_tokens, reduce, out_dtype));
  if (total_tokens == 0 || n_seqs == 0) return SCONE_OK;
  if (!d_tok || !d_cu_seqlens || !d_base || !d_out)
    return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_tok, d_cu_seqlens, d_base and d_out are required)");
  SCONE_TRY(check_wpe(h, who, d_wpe, n_pos));
  SCONE_TRY(check_base(h, who, d_base, d_out, total_tokens, out_dtype));
  SCONE_ON_DEVICE(h);
  embed_args a = lookup_args(h, total_tokens, (int)total_tokens);
  combine(a, d_tok, d_pos, nullptr, 0, d_base, d_wpe, n_pos, reduce, d_out);
  return embed_packed(h, a, d_cu_seqlens, n_seqs, out_dtype, (hipStream_t)stream);
}

// Packed variable-length batch (embed_packed).
extern "C" int scone_embed_varlen(scone_handle *h, const int32_t *d_tok, const int32_t *d_cu_seqlens, int32_t n_seqs,
                                  int64_t total_tokens, const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos,
                                  const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_embed_varlen";
  SCONE_TRY(scone_need_table(h, who));
  SCONE_TRY(check_packed(h, who, n_seqs, total_tokens, reduce, out_dtype));
  if (total_tokens == 0 || n_seqs == 0) return SCONE_OK;
  if (!d_tok || !d_cu_seqlens || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_TRY(check_wte_wpe(h, who, d_wte, vocab, d_wpe, n_pos));
  SCONE_ON_DEVICE(h);
  embed_args a = lookup_args(h, total_tokens, (int)total_tokens);
  combine(a, d_tok, d_pos, d_wte, vocab, nullptr, d_wpe, n_pos, reduce, d_out);
  return embed_packed(h, a, d_cu_seqlens, n_seqs, out_dtype, (hipStream_t)stream);
}

// ---- the fused lookup over a batch's live rows (scone_embed_rows.h): the existing match, then k_embed_rows in the place of
// the table's gather kernel.  The handle's table is never read, so pinned-host and staged handles take this road as any other.
namespace {
int launch_rows(scone_handle *h, const live_rows_view &live, int dtype, const embed_args &a, int out_dtype, hipStream_t s) {
  switch (dtype) {
    case SCONE_DT_F32: return launch_rows_f32(h, live, a, out_dtype, s);
    case SCONE_DT_F16: return launch_rows_f16(h, live, a, out_dtype, s);
    default: return launch_rows_bf16(h, live, a, out_dtype, s);  // (check_live_ptrs admits three types)
  }
}
// what both live-row entry points check before an empty batch returns: the handle and the scalars
int check_live_handle(scone_handle *h, const char *who, int32_t reduce, int32_t out_dtype) {
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim <= 0 || h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs a handle with dim > 0 and dim % 8 == 0");
  if (h->cfg.row_begin != 0 || h->cfg.row_end != h->cfg.n_rows)
    return scone_refuse(h, SCONE_EINVAL, who, "not for a row-sharded handle (its match records leave out the other shards' hits)");
  SCONE_TRY(check_reduce(h, who, reduce));
  return check_out_dtype(h, who, out_dtype);
}
// ... and with work to do
int check_live_ptrs(scone_handle *h, const char *who, const scone_live_rows *live, const void *d_tok, const void *d_out,
                    const void *d_wte, int64_t vocab, const void *d_base, const void *d_wpe, int64_t n_pos, long long ntok,
                    int32_t out_dtype) {
  if (!live) return scone_refuse(h, SCONE_EINVAL, who, "null live");
  if (live->struct_size != sizeof(scone_live_rows)) return scone_refuse(h, SCONE_EINVAL, who, "bad struct_size");
  if (live->dtype != SCONE_DT_F32 && live->dtype != SCONE_DT_F16 && live->dtype != SCONE_DT_BF16)
    return scone_refuse(h, SCONE_EINVAL, who, "bad dtype (live rows are fp32, fp16 or bf16)");
  if (live->n > 0x7FFFFFFFull) return scone_refuse(h, SCONE_EINVAL, who, "n above 2^31 - 1");
  if (!d_tok || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_tok and d_out are required)");
  if (live->n && (!live->d_row_ids || !live->d_rows))
    return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_row_ids and d_rows are required with n > 0)");
  if (reinterpret_cast<uintptr_t>(live->d_rows) % 16 != 0) return scone_refuse(h, SCONE_EINVAL, who, "d_rows is not 16-byte aligned");
  if (d_wte && d_base) return scone_refuse(h, SCONE_EINVAL, who, "d_wte and d_base are exclusive");
  SCONE_TRY(check_wte_wpe(h, who, d_wte, vocab, d_wpe, n_pos));
  if (d_base) SCONE_TRY(check_base(h, who, d_base, d_out, ntok, out_dtype));
  return SCONE_OK;
}
live_rows_view live_view(const scone_live_rows *live) {
  live_rows_view v;
  v.rows = reinterpret_cast<const uint8_t *>(live->d_rows), v.ids = live->d_row_ids;
  v.n = live->n, v.d_n = reinterpret_cast<const unsigned long long *>(live->d_n);
  return v;
}
// the handle's part of the lookup without its table: the records, the zero row, the lookup mode, the status word
embed_args rows_args(const scone_handle *h, long long ntok, int T) {
  embed_args a = {};
  a.tv.d = h->cfg.dim;
  a.BT = ntok, a.ntok = ntok, a.T = T, a.max_n = h->cfg.max_n;
  a.zero_row = h->d_zero_row, a.mode = (int)h->cfg.lookup_mode, a.status = h->d_status;
  return a;
}
}  // namespace

extern "C" int scone_embed_rows(scone_handle *h, const scone_live_rows *live, const int32_t *d_tok, int32_t B, int32_t T,
                                const void *d_wte, int64_t vocab, const void *d_base, const void *d_wpe, int64_t n_pos,
                                const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_embed_rows";
  SCONE_TRY(check_live_handle(h, who, reduce, out_dtype));
  SCONE_TRY(check_shape(h, who, B, T));
  const long long BT = (long long)B * T;
  if (BT == 0) return SCONE_OK;
  SCONE_TRY(check_live_ptrs(h, who, live, d_tok, d_out, d_wte, vocab, d_base, d_wpe, n_pos, BT, out_dtype));
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  embed_args a = rows_args(h, BT, T);
  combine(a, d_tok, d_pos, d_wte, vocab, d_base, d_wpe, n_pos, reduce, d_out);
  // the workspace of THIS stream, held while the match that writes it and the lookup that reads it are enqueued
  scone_ws_lock ws(scone_ws_acquire(h, s));
  if (!ws.w) return scone_refuse(h, SCONE_ENOMEM, who, "out of memory");
  SCONE_TRY(scone_ensure_ell(h, ws.w, BT));
  SCONE_TRY(scone_launch_match_ell(h, d_tok, B, T, ws.w->d_ell, s));
  a.ell = ws.w->d_ell;
  const live_rows_view lv = live_view(live);
  return profiled(h, s, [&] { return launch_rows(h, lv, live->dtype, a, out_dtype, s); });
}

// Packed batch: k_match_ell_varlen leaves one record and one position per token, as in embed_packed, and the same traversal
// follows ([total / T', T'] plus the remainder when SCONE_VARLEN_T or a stream above 2^25 tokens asks for rows).
extern "C" int scone_embed_rows_varlen(scone_handle *h, const scone_live_rows *live, const int32_t *d_tok,
                                       const int32_t *d_cu_seqlens, int32_t n_seqs, int64_t total_tokens, const void *d_wte,
                                       int64_t vocab, const void *d_base, const void *d_wpe, int64_t n_pos, const int32_t *d_pos,
                                       int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_embed_rows_varlen";
  SCONE_TRY(check_live_handle(h, who, reduce, out_dtype));
  if (n_seqs < 0 || total_tokens < 0) return scone_refuse(h, SCONE_EINVAL, who, "negative n_seqs or total_tokens");
  SCONE_TRY(check_total(h, who, total_tokens));
  if (total_tokens == 0 || n_seqs == 0) return SCONE_OK;
  if (!d_cu_seqlens) return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_cu_seqlens is required)");
  SCONE_TRY(check_live_ptrs(h, who, live, d_tok, d_out, d_wte, vocab, d_base, d_wpe, n_pos, total_tokens, out_dtype));
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  const long long total = total_tokens;
  embed_args a = rows_args(h, total, (int)total);
  combine(a, d_tok, d_pos, d_wte, vocab, d_base, d_wpe, n_pos, reduce, d_out);
  scone_ws_lock ws(scone_ws_acquire(h, s));
  if (!ws.w) return scone_refuse(h, SCONE_ENOMEM, who, "out of memory");
  SCONE_TRY(scone_ensure_ell(h, ws.w, total));
  int32_t *vpos = nullptr;
  if (a.wpe && !a.pos) {  // default positions p - cu[s]: written by the match
    SCONE_TRY(scone_ensure_vpos(h, ws.w, total));
    vpos = ws.w->d_vpos;
    a.pos = vpos;
  }
  SCONE_TRY(scone_launch_match_ell_varlen(h, d_tok, d_cu_seqlens, n_seqs, total, ws.w->d_ell, vpos, s));
  a.ell = ws.w->d_ell;
  const long long row = h->varlen_t > 0 ? h->varlen_t : (total <= (1ll << 25) ? total : 512);
  const long long Tp = total < row ? total : row;
  const long long main_tok = total / Tp * Tp;
  const live_rows_view lv = live_view(live);
  return profiled(h, s, [&] {
    embed_args m = slice(a, 0, main_tok, out_dtype);
    m.T = (int)Tp;
    int rc = launch_rows(h, lv, live->dtype, m, out_dtype, s);
    if (!rc && main_tok < total) {
      embed_args r = slice(a, main_tok, total - main_tok, out_dtype);
      r.T = (int)r.BT;
      rc = launch_rows(h, lv, live->dtype, r, out_dtype, s);
    }
    return rc;
  });
}

// The fused lookup at chosen positions only (scone_embed_select.h): one launch of ceil(n_sel / 4) workgroups, no workspace, no
// lock, no synchronisation -- thread-safe like the one-launch road of scone_embed.
extern "C" int scone_embed_select(scone_handle *h, const int32_t *d_tok, int64_t total_tokens, int32_t T,
                                  const int32_t *d_cu_seqlens, int32_t n_seqs, const int32_t *d_sel, int64_t n_sel,
                                  const void *d_wte, int64_t vocab, const void *d_base, const void *d_wpe, int64_t n_pos,
                                  const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_embed_select";
  SCONE_TRY(scone_need_table(h, who));
  if (total_tokens < 0 || n_sel < 0 || (d_cu_seqlens && n_seqs < 0))
    return scone_refuse(h, SCONE_EINVAL, who, "negative total_tokens, n_sel or n_seqs");
  SCONE_TRY(check_total(h, who, total_tokens));
  SCONE_TRY(check_reduce(h, who, reduce));
  SCONE_TRY(check_out_dtype(h, who, out_dtype));
  if (h->cfg.dim % 8 != 0) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0");
  if (is_staged(h))
    return scone_refuse(h, SCONE_EINVAL, who, "not for stage_tokens > 0 (the staging pipeline prefetches whole batches; "
                                              "tables read in place from pinned host memory work)");
  if (!d_cu_seqlens && total_tokens > 0 && (T <= 0 || total_tokens % T != 0))
    return scone_refuse(h, SCONE_EINVAL, who, "a rectangle needs T > 0 and total_tokens % T == 0");
  if (d_wte && d_base) return scone_refuse(h, SCONE_EINVAL, who, "d_wte and d_base are exclusive");
  SCONE_TRY(check_wte_wpe(h, who, d_wte, vocab, d_wpe, n_pos));
  if (n_sel == 0 || total_tokens == 0 || (d_cu_seqlens && n_seqs == 0)) return SCONE_OK;
  if (!d_tok || !d_sel || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer (d_tok, d_sel and d_out are required)");
  if (!scone_grid_fits(((unsigned long long)n_sel + 3) / 4, 256))
    return scone_refuse(h, SCONE_EINVAL, who, "too many selected positions for one launch");
  if (d_base) SCONE_TRY(check_base(h, who, d_base, d_out, n_sel, out_dtype));
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  select_args a = {};
  fill_table_view(h, a.tv);
  a.tok = d_tok, a.total = total_tokens, a.T = d_cu_seqlens ? 0 : T, a.cu = d_cu_seqlens, a.n_seqs = n_seqs;
  a.sel = d_sel, a.n_sel = n_sel;
  a.wte = d_wte, a.vocab = vocab, a.base = d_base, a.wpe = d_wpe, a.n_pos = n_pos, a.pos = d_pos;
  a.reduce = reduce, a.mode = (int)h->cfg.lookup_mode, a.max_n = h->cfg.max_n;
  a.zero_row = h->d_zero_row, a.out = d_out, a.status = h->d_status;
  return profiled(h, s, [&] { return launch_select(h, a, out_dtype, s); });
}

// All-gather form.  The gathered records (one per distinct row, every shard's) join the handle's row map with
// scone_shard_gather_add_records -- all at once, or chunk by chunk as the all-gathers of a pipelined exchange complete --
// and scone_shard_gather_embed_range reduces a run of sequences of the planned batch out of
// [replicated head | records received so far]; scone_shard_gather_embed is the two for a whole batch.
extern "C" int scone_shard_gather_add_records(scone_handle *h, const void *d_records_base, uint64_t record0, uint64_t n_records,
                                              uint64_t n_total, scone_stream_t stream) {
  const char *who = "scone_shard_gather_add_records";
  SCONE_TRY(scone_need_table(h, who));
  if (!h->shard) return scone_refuse(h, SCONE_ESTATE, who, "call scone_shard_gather_plan first");
  if (n_records && !d_records_base) return scone_refuse(h, SCONE_EINVAL, who, "null records");
  SCONE_ON_DEVICE(h);
  const uint8_t *p = reinterpret_cast<const uint8_t *>(d_records_base) + (size_t)record0 * (size_t)scone_shard_rec_bytes(h);
  return scone_shard_gather_add(h, p, n_records, record0, n_total, (hipStream_t)stream);
}

namespace {
// What the two shard embeds share: the lookup of sequences [seq_begin, seq_end) of the planned batch out of the row store
// [replicated head | the n_total rows received at d_rows], written to d_out, which begins at token out_tok0 of the batch.
// `bad`: the entry point's own arguments are wrong; `remap` resolves the range's id records against the received rows and
// points tv.st.hot / n_hot / row_bytes and tv.scales at its head rows and scales.
template <typename Remap>
int shard_embed(scone_handle *h, const char *who, bool bad, const int32_t *d_tok, int32_t B, int32_t T, int32_t seq_begin,
                int32_t seq_end, const void *d_rows, uint64_t n_total, const void *d_wte, int64_t vocab, const void *d_wpe,
                int64_t n_pos, const int32_t *d_pos, int32_t reduce, void *d_out, int64_t out_tok0, int32_t out_dtype, hipStream_t s,
                Remap &&remap) {
  SCONE_TRY(scone_need_table(h, who));
  if (!h->shard) return scone_refuse(h, SCONE_ESTATE, who, "call scone_shard_gather_plan first");
  int32_t pB = 0, pT = 0;
  scone_shard_plan_shape(h, &pB, &pT);
  if (bad || B < 0 || T <= 0 || B != pB || T != pT || seq_begin < 0 || seq_end < seq_begin || seq_end > B || (n_total && !d_rows) ||
      out_tok0 < 0 || out_tok0 > (long long)seq_begin * T)
    return scone_refuse(h, SCONE_EINVAL, who, "bad argument (B, T must be the planned batch's)");
  if (!scone_wave_kernel_covers(h->cfg.table_fmt, h->cfg.dim)) return scone_refuse(h, SCONE_EINVAL, who, "needs d % 8 == 0");
  SCONE_TRY(check_reduce(h, who, reduce));
  const long long nt = (long long)(seq_end - seq_begin) * T;
  if (nt == 0) return SCONE_OK;
  if (!d_tok || !d_out) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_ON_DEVICE(h);
  embed_args full = lookup_args(h, (long long)B * T, T);
  combine(full, d_tok, d_pos, d_wte, vocab, nullptr, d_wpe, n_pos, reduce, d_out);
  embed_args a = slice(full, (long long)seq_begin * T, nt, out_dtype);
  a.out = reinterpret_cast<uint8_t *>(a.out) - (size_t)out_tok0 * h->cfg.dim * scone_dt_bytes(out_dtype);
  SCONE_TRY(remap(s, &a.ell, a.tv));  // the records it writes are the range's own
  a.tv.st.cold = n_total ? reinterpret_cast<uint8_t *>(const_cast<void *>(d_rows)) : reinterpret_cast<uint8_t *>(h->d_zero_row);
  a.tv.row_begin = 0, a.tv.row_end = (long long)(a.tv.st.n_hot + (n_total ? n_total : 1));
  return launch_fmt(h, a, SRC_HITS, MODE_FULL, out_dtype, s);
}
}  // namespace

// scone_shard_gather_embed_range reports as scone_shard_gather_embed (callers match on the texts).  Row store: [replicated head |
// gathered records], both in record layout.
extern "C" int scone_shard_gather_embed_range(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t seq_begin,
                                              int32_t seq_end, const void *d_records_base, uint64_t n_total, const void *d_wte,
                                              int64_t vocab, const void *d_wpe, int64_t n_pos, const int32_t *d_pos,
                                              int32_t reduce, void *d_out, int64_t out_tok0, int32_t out_dtype,
                                              scone_stream_t stream) {
  return shard_embed(h, "scone_shard_gather_embed", false, d_tok, B, T, seq_begin, seq_end, d_records_base, n_total, d_wte, vocab,
                     d_wpe, n_pos, d_pos, reduce, d_out, out_tok0, out_dtype, (hipStream_t)stream,
                     [&](hipStream_t s, const int32_t **ell, table_view &tv) {
                       const void *scales = nullptr;
                       SCONE_TRY(scone_shard_gather_remap(h, T, seq_begin, seq_end, ell, &scales, s));
                       tv.st.hot = scone_shard_head(h, &tv.st.n_hot);
                       tv.st.row_bytes = (unsigned int)scone_shard_rec_bytes(h);
                       tv.scales = reinterpret_cast<const __half *>(scales);
                       return (int)SCONE_OK;
                     });
}

// Columns exchange (scone_shard.hip): the received payload rows are read in place at the table's own stride, the scales come
// from the caller's [head scales | received scales] buffer, the id lists are resolved through the senders' hash fragments.
// Row store: [replicated head | received rows], both at the payload stride.
extern "C" int scone_shard_cols_embed(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, int32_t seq_begin,
                                      int32_t seq_end, const void *d_rows, uint64_t n_total, const void *d_scales_full,
                                      const void *d_frags, uint64_t frag_slots_total, const uint64_t *h_frag_off,
                                      const uint64_t *h_frag_slots, const uint64_t *h_rec_base, const uint64_t *h_row_lo,
                                      int32_t world, const void *d_wte, int64_t vocab,
                                      const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce, void *d_out,
                                      int64_t out_tok0, int32_t out_dtype, scone_stream_t stream) {
  const bool bad = !d_frags || !h_frag_off || !h_frag_slots || !h_rec_base || (h && h->scale_bytes_per_row && !d_scales_full);
  return shard_embed(h, "scone_shard_cols_embed", bad, d_tok, B, T, seq_begin, seq_end, d_rows, n_total, d_wte, vocab, d_wpe, n_pos,
                     d_pos, reduce, d_out, out_tok0, out_dtype, (hipStream_t)stream,
                     [&](hipStream_t s, const int32_t **ell, table_view &tv) {
                       const uint8_t *head_p = nullptr;
                       SCONE_TRY(scone_shard_cols_remap(h, T, seq_begin, seq_end, d_frags, frag_slots_total, h_frag_off, h_frag_slots,
                                                        h_rec_base, h_row_lo, world, n_total, ell, &head_p, &tv.st.n_hot, s));
                       tv.st.hot = const_cast<uint8_t *>(head_p);
                       tv.st.row_bytes = (unsigned int)h->row_payload_bytes;
                       tv.scales = reinterpret_cast<const __half *>(d_scales_full);
                       return (int)SCONE_OK;
                     });
}

extern "C" int scone_shard_gather_embed(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, const void *d_records,
                                        uint64_t n_records, const void *d_wte, int64_t vocab, const void *d_wpe, int64_t n_pos,
                                        const int32_t *d_pos, int32_t reduce, void *d_out, int32_t out_dtype,
                                        scone_stream_t stream) {
  SCONE_TRY(scone_shard_gather_add_records(h, d_records, 0, n_records, n_records, stream));
  if ((long long)B * T == 0) return SCONE_OK;
  return scone_shard_gather_embed_range(h, d_tok, B, T, 0, B, d_records, n_records, d_wte, vocab, d_wpe, n_pos, d_pos, reduce,
                                        d_out, 0, out_dtype, stream);
}

extern "C" int scone_embed_partial(scone_handle *h, const int32_t *d_tok, int32_t B, int32_t T, float *d_partial,
                                   int32_t *d_counts, scone_stream_t stream) {
  const char *who = "scone_embed_partial";
  SCONE_TRY(scone_need_table(h, who));
  SCONE_TRY(check_shape(h, who, B, T));
  const long long BT = (long long)B * T;
  if (BT == 0) return SCONE_OK;
  if (!d_tok || !d_partial || !d_counts) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  SCONE_TRY(check_mode(h, who));
  embed_args a = lookup_args(h, BT, T);
  a.tok = d_tok, a.reduce = SCONE_REDUCE_SUM, a.partial = d_partial, a.counts = d_counts;
  scone_ws_lock ws(scone_ws_acquire(h, s));
  if (!ws.w) return scone_refuse(h, SCONE_ENOMEM, who, "out of memory");
  SCONE_TRY(match_into(h, ws.w, B, T, a, s));
  return launch_fmt(h, a, SRC_HITS, MODE_PARTIAL, SCONE_DT_F32, s);
}

extern "C" int scone_finalize(scone_handle *h, const float *d_sum, const int32_t *d_counts, const int32_t *d_tok,
                              int32_t B, int32_t T, int64_t tok_begin, int64_t tok_end, const void *d_wte,
                              int64_t vocab, const void *d_wpe, int64_t n_pos, const int32_t *d_pos, int32_t reduce,
                              void *d_out, int32_t out_dtype, scone_stream_t stream) {
  const char *who = "scone_finalize";
  if (!h) return SCONE_EINVAL;
  if (h->cfg.dim <= 0) return scone_refuse(h, SCONE_ESTATE, who, "handle has no table (dim == 0)");  // the sums need no rows
  const long long BT = (long long)B * T;
  if (B < 0 || T < 0 || tok_begin < 0 || tok_end < tok_begin || tok_end > BT) return scone_refuse(h, SCONE_EINVAL, who, "bad token range");
  if (tok_end == tok_begin) return SCONE_OK;
  if (!d_sum || !d_counts || !d_out || ((d_wte || d_wpe) && !d_tok)) return scone_refuse(h, SCONE_EINVAL, who, "null pointer");
  SCONE_TRY(check_reduce(h, who, reduce));
  SCONE_ON_DEVICE(h);
  embed_args a = lookup_args(h, BT, T);
  a.tok_begin = tok_begin, a.ntok = tok_end - tok_begin;
  combine(a, d_tok, d_pos, d_wte, vocab, nullptr, d_wpe, n_pos, reduce, d_out);
  a.sums = d_sum, a.counts = const_cast<int32_t *>(d_counts);
  return launch_fmt(h, a, SRC_HITS, MODE_FINALIZE, out_dtype, (hipStream_t)stream);
}
