"""TEST CODE ONLY -- a pure-Python mirror of how the two large-batch lookup kernels cut a batch into workgroups
(scone_amd/csrc/scone_embed_wave.h: `launch_wave` for k_embed_wave, `launch_wave_any` for k_embed_wave_any), so that a test
can ASSERT that its batch makes a workgroup walk several sequences instead of hoping so.  Nothing under scone_amd/ may import
this module.

A workgroup's 4 waves own 4 consecutive positions of a sequence (`pos_groups = ceil(T / 4)` workgroups side by side cover one
sequence) and walk `seqs_per_block` sequences one after the other; `chunks` such runs cover the B sequences, the last one
with `last_run <= seqs_per_block` of them.

k_embed_wave sizes its grid from `target = 3 * CUs * WAVES`, where WAVES (<= 8) depends on the instantiation's register
estimate.  A larger target gives more runs, never longer ones (chunks is non-decreasing in target, seqs_per_block =
ceil(B / chunks) non-increasing), so the geometry at WAVES = 8 is a LOWER bound of seqs_per_block for every instantiation on
the same number of compute units.  `wave()` therefore takes `waves=8` by default; `wave_all()` gives the geometry at every
WAVES in 1..8 for the claims that are not monotone (a last run shorter than the others).
"""

from collections import namedtuple

Geometry = namedtuple("Geometry", "pos_groups chunks seqs_per_block last_run blocks")

WAVE_ANY_BLOCKS = 4096           # SCONE_WAVE_BLOCKS
FUSED_MAX_TOKENS = 32768         # scone_handle::fused_max_tokens without SCONE_FUSED_MAX_TOKENS
WAVE_DIMS = (768, 1024, 1280)    # dims with a specialised k_embed_wave / k_embed_fused


def _cut(B, T, chunks):
    pos_groups = (T + 3) // 4
    chunks = max(1, min(int(chunks), B))
    spb = (B + chunks - 1) // chunks
    chunks = (B + spb - 1) // spb
    return Geometry(pos_groups, chunks, spb, B - (chunks - 1) * spb, chunks * pos_groups)


def wave(B, T, cus, waves=8):
    """launch_wave: target = 3 * cus * waves workgroups, `cus` = compute units minus the handle's CU reserve."""
    pos_groups = (T + 3) // 4
    target = 3 * max(int(cus), 1) * waves
    return _cut(B, T, (target + pos_groups // 2) // pos_groups)


def wave_all(B, T, cus):
    return [wave(B, T, cus, w) for w in range(1, 9)]


def wave_any(B, T):
    """launch_wave_any: a fixed target of SCONE_WAVE_BLOCKS workgroups."""
    return _cut(B, T, WAVE_ANY_BLOCKS // ((T + 3) // 4))


def kernel_family(fmt, d):
    """Which kernel a two-kernel-form lookup of this table takes (try_launch_wave_on / wave_geom<>::OK)."""
    if d % 8:
        return "k_embed"
    if d in WAVE_DIMS and not (fmt == "int4" and d != 1024):
        return "k_embed_wave"
    return "k_embed_wave_any"


def takes_one_launch(fmt, d, n_tokens, fused_max_tokens=FUSED_MAX_TOKENS):
    """scone_embed_takes_one_launch: match + gather in one launch (k_embed_fused), no walk at all."""
    return n_tokens <= fused_max_tokens and d in WAVE_DIMS and not (fmt == "int4" and d != 1024)


def max_list_length(T, max_n, mode="cover"):
    """The longest id list a token of a length-T sequence can get: in cover mode every window of length n <= max_n that
    fits in the sequence and covers the token; in longest_suffix mode at most one f-gram (of length >= 2)."""
    if mode != "cover":
        return 1 if T >= 2 and max_n >= 2 else 0
    best = 0
    for i in range(T):
        k = 0
        for n in range(1, min(max_n, T) + 1):
            k += sum(1 for s in range(n) if i - s >= 0 and i - s + n <= T)
        best = max(best, k)
    return best
