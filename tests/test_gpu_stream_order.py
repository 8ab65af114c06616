"""The stream contract of every entry point: its device work is ordered on the stream it is given, and it synchronises exactly
when include/scone_hip.h says so.

Every case runs the protocol of tests/stream_fixture.py on a side stream S behind a ~50 ms delay kernel: the input buffers hold
a valid POISON until copies queued behind the delay bring the truth, the call under test follows, the poison is copied back and
clones of every output and of all mutated state are taken -- all on S, nothing synchronised in between.  The clones are compared
bit for bit (`edge_fixture.same_bits`) with the references the rest of the suite uses (oracle/ref_port.py and the
`*_fixture.py` statements of the backward, the optimizer steps, the norm and the merge); there is no tolerance anywhere.

Two classes, from the header's wording (the table `CONTRACT` quotes the sentence beside every entry point):
  A  "stream-ordered, no synchronisation": the call returned while the delay was still running, and the bits are right;
  S  "synchronises the stream (once)": everything queued before it on S had completed when it returned, and the host value it
     returned (U, n_refs, n_out, total, status bits) is the reference's.
A kernel on stream 0, a copy or memset on the wrong stream, a missing cross-stream wait, a hidden synchronise and a count read
back behind another stream's synchronise each fail a case here and no other test of the suite (tools/stream_mutants.sh builds
six such libraries and shows it).

Shapes are the smallest that reach each code path: edge_fixture's vocabularies with its 2 x 33 and 4 x 64 token streams, the
backward suite's "small" packed batch (rows of several chunks) and its 9 x 37 rectangle (none), d = 64 for the generic kernels,
768 for the specialised ones, INT4 at d = 1024 for the permuted scale slots.

Measured on an MI355X: 82 cases, 6.7 s of wall time for the whole file (0.06 s for a typical case: two runs of the sequence
and one delay, which the device ran for 49 to 50 ms in every case).

Findings of the file when it was written.  (1) `BackwardPlan.row_ids()` kept its tensor without an event: with the parent's
wrapper `test_row_ids_made_on_one_stream_serve_another` reads ids that are not yet written; the wrapper now records an event
behind the launch and a caller on another stream waits for it.  (2) No entry point of the library violated its sentence.
(3) Which stream `scone_backward_plan`'s final synchronise names cannot be observed under this HIP runtime: the copy of the
counts to pageable host memory in front of it already waits (tools/stream_mutants.sh, `plan_sync_wrong_stream`).
"""

import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import bf16_fixture as BF  # noqa: E402
import edge_fixture as E  # noqa: E402
import grad_merge_fixture as GM  # noqa: E402
import grad_norm_fixture as GN  # noqa: E402
import lean_fixture as LF  # noqa: E402
import mxfp4_fixture as MX  # noqa: E402
import opt_fixture as OF  # noqa: E402
import stream_fixture as SF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only: the batches, their id lists, gradients and expectations)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, rounding)

pytestmark = pytest.mark.gpu

A, S = SF.A, SF.S
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scone_hip.h")

# Every entry point of include/scone_hip.h that takes a scone_stream_t: (class, the header's sentence, the test that holds its
# case -- or, class None, why it is not a case here).  test_the_table_names_every_entry_point_that_takes_a_stream keeps it whole.
_LOOKUP = "lookups are thread-safe and stream-ordered"
_EMBED = "Stream-ordered, no hidden synchronisation"
_CONV = "all device work is enqueued on the given stream ... and the call returns without synchronising unless documented otherwise"
_SHARD = "the scone_shard_* exchange calls: their one early-return check is test_gpu_parity.py's async-plan test; an exchange needs the ranks' buffers"
_IPC = "scone_ipc_*: interprocess buffers and events need a second process (tests/test_gpu_multiprocess.py)"
_FIT = "scone_fit*: every call is documented as synchronising, some twice, and the state is host-mirrored; the fit suites compare its results"
CONTRACT = {
    "scone_status": (S, "synchronises the stream, returns the bits in *bits and clears them", "test_table"),
    "scone_index_build_device": (A, "the device variant is stream-ordered", "test_table"),
    "scone_table_upload": (A, _CONV + " (device source pointers)", "test_table"),
    "scone_table_download": (A, "synchronises for host destinations (so not for device ones)", "test_table"),
    "scone_table_store_f32": (A, _CONV, "test_table"),
    "scone_table_store_f32_ids": (A, _CONV, "test_table"),
    "scone_table_fill_synthetic": (A, _CONV, "test_table"),
    "scone_table_gather_rows": (A, _LOOKUP, "test_table"),
    "scone_match": (A, _LOOKUP, "test_forward"),
    "scone_match_csr": (S, "Writes the total to *h_total after synchronising the stream", "test_forward"),
    "scone_gather_reduce": (A, _LOOKUP, "test_forward"),
    "scone_embed": (A, _EMBED, "test_forward"),
    "scone_embed_varlen": (A, "Stream-ordered, no hidden synchronisation: total_tokens comes from the host", "test_forward"),
    "scone_embed_base": (A, "Same launches, workspaces and stream ordering as scone_embed / scone_embed_varlen", "test_forward"),
    "scone_embed_base_varlen": (A, "Same launches, workspaces and stream ordering as scone_embed / scone_embed_varlen", "test_forward"),
    "scone_embed_select": (A, "no workspace, no lock, no synchronisation", "test_forward"),
    "scone_embed_prefetch": (A, "ordered behind `stream` (the stream on which the tokens are produced) ... and the call returns",
                             "test_cross_stream_hops"),
    "scone_embed_partial": (A, _LOOKUP, "test_forward"),
    "scone_finalize": (A, _LOOKUP, "test_forward"),
    "scone_backward_plan": (S, "Synchronises the stream ONCE, to return U in *h_n_rows and the reference count in *h_n_refs", "test_backward_plan"),
    "scone_backward_plan_varlen": (S, "the same for scone_embed_varlen's packed batch", "test_backward_plan"),
    "scone_backward_plan_csr": (S, "Synchronises twice more than the token forms", "test_backward_plan"),
    "scone_backward_rows": (A, "Stream-ordered: no synchronisation, no allocation", "test_backward_rows"),
    "scone_backward_counts": (A, "K_p per position, int32 [ntok]; stream-ordered", "test_backward_rows"),
    "scone_backward_row_ids": (A, "No call synchronises ... One launch", "test_backward_rows"),
    "scone_backward_rows_acc": (A, "Stream-ordered, at most three launches, no allocation, no synchronisation", "test_backward_rows"),
    "scone_backward_apply_lean": (A, "The call is stream-ordered: it does not synchronise and allocates nothing", "test_backward_rows"),
    "scone_grad_merge_map": (S, "h_n_out != NULL: the stream is synchronised ONCE and n_out returned ...; h_n_out == NULL: no synchronisation (A)",
                             "test_accumulate"),
    "scone_grad_merge_rows": (A, "Stream-ordered, ONE launch", "test_accumulate"),
    "scone_grad_sqnorm": (A, "No call synchronises or allocates; all are stream-ordered", "test_norm_and_clip"),
    "scone_grad_ctl_set": (A, "No call synchronises or allocates; all are stream-ordered", "test_norm_and_clip"),
    "scone_opt_step_ctl": (A, "Still one launch, no synchronisation, no allocation", "test_norm_and_clip"),
    "scone_opt_step_lean_ctl": (A, "Still one launch, no synchronisation, no allocation", "test_norm_and_clip"),
    "scone_opt_step": (A, "The call is stream-ordered: it does not synchronise, allocates nothing", "test_optimizer"),
    "scone_opt_step_lean": (A, "The call is stream-ordered: no synchronisation, no allocation", "test_optimizer"),
    # ---- named, and out of scope here
    "scone_streams_overlap": (None, "synchronises both streams", "a probe that synchronises by definition; stream_fixture.side_stream uses it"),
    "scone_shard_head_store_f32": (None, "", "scone_table_store_f32 into the replicated head: the same launch (scone_store_f32_into); " + _SHARD),
    "scone_shard_gather_plan": (None, "", _SHARD), "scone_shard_gather_pack": (None, "", _SHARD),
    "scone_shard_gather_embed": (None, "", _SHARD), "scone_shard_gather_plan_chunks": (None, "", _SHARD),
    "scone_shard_gather_match": (None, "", _SHARD), "scone_shard_gather_plan_ell": (None, "", _SHARD),
    "scone_shard_gather_pack_range": (None, "", _SHARD), "scone_shard_gather_add_records": (None, "", _SHARD),
    "scone_shard_gather_remap_range": (None, "", _SHARD), "scone_shard_gather_embed_range": (None, "", _SHARD),
    "scone_shard_gather_plan_async": (None, "", _SHARD), "scone_shard_gather_plan_ell_async": (None, "", _SHARD),
    "scone_shard_cols_pack_cap": (None, "", _SHARD), "scone_shard_cols_pack": (None, "", _SHARD),
    "scone_shard_cols_build_frag": (None, "", _SHARD), "scone_shard_head_scales": (None, "", _SHARD),
    "scone_shard_cols_embed": (None, "", _SHARD),
    "scone_ipc_event_record": (None, "", _IPC), "scone_ipc_event_wait": (None, "", _IPC), "scone_ipc_push": (None, "", _IPC),
    "scone_fit": (None, "", _FIT), "scone_fit_update": (None, "", _FIT), "scone_fit_update_part": (None, "", _FIT),
    "scone_fit_finalize": (None, "", _FIT), "scone_fit_finalize_seq": (None, "", _FIT), "scone_fit_export": (None, "", _FIT),
    "scone_fit_merge": (None, "", _FIT),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def stream_entry_points(text):
    """Names of the prototypes of the header that take a scone_stream_t."""
    protos = re.findall(r"^(?:int|void|uint32_t)\s+(scone_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S | re.M)
    return sorted(name for name, args in protos if "scone_stream_t" in args)


def test_the_table_names_every_entry_point_that_takes_a_stream():
    with open(HEADER) as f:
        names = stream_entry_points(f.read())
    assert len(names) > 60 and "scone_embed" in names and "scone_grad_merge_rows" in names
    assert sorted(CONTRACT) == names, (sorted(set(names) - set(CONTRACT)), sorted(set(CONTRACT) - set(names)))
    for name, (klass, sentence, where) in CONTRACT.items():
        if klass is None:
            assert len(where) > 20, f"{name}: out of scope without a reason"
        else:
            assert klass in (A, S) and sentence and callable(globals().get(where)), f"{name}: no case"


# ------------------------------------------------------------------ shared pieces
def _lib():
    from scone_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _cur():
    return torch.cuda.current_stream().cuda_stream


def _table(max_n, n, d, fmt, fused_max_tokens=None, **kw):
    """A handle; SCONE_FUSED_MAX_TOKENS is read when it is created ("0": every batch takes the two-kernel road)."""
    from scone_amd.hip_backend import SconeTable
    key, old = "SCONE_FUSED_MAX_TOKENS", os.environ.get("SCONE_FUSED_MAX_TOKENS")
    try:
        if fused_max_tokens is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = str(fused_max_tokens)
        return SconeTable(max_n, n, dim=d, table_format=fmt, **kw)
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old


def _stored(rows, fmt):
    """What the format holds, as fp32: the oracle's table."""
    if fmt == "fp32":
        return rows
    if fmt == "bf16":
        return BF.from_bf16_bits(BF.to_bf16_bits(rows))
    if fmt == "int8":
        return R.dequantize_i8(*R.quantize_i8(rows))
    if fmt == "mxfp4":
        return MX.stored(rows)
    assert fmt == "int4"
    return R.dequantize_i4(*R.quantize_i4(rows))


def _same(res, name, want, who):
    got = res.out[name]
    want = SF.to_numpy(want) if isinstance(want, torch.Tensor) else np.ascontiguousarray(want)
    if want.dtype.kind in "iub" and want.dtype != np.uint16:
        ok = got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64))
        assert ok, f"{who}: {name} differs from the reference ({res.describe()})"
    else:
        want = want.reshape(got.shape)
        ok = want.dtype == got.dtype and E.same_bits(got, want)
        assert ok, f"{who}: {name}: {E.first_difference(got, want)} ({res.describe()})"


def _finish(res, klass, who, want, host_want=None, status=0):
    """Class, bits, host value, status: the four checks of every case."""
    SF.check_class(res, klass, who)
    for name, w in want.items():
        _same(res, name, w, who)
    if host_want is not None:
        assert res.host == host_want, f"{who}: returned {res.host!r} to the host, the reference says {host_want!r} ({res.describe()})"
    assert res.status == status, f"{who}: status {res.status}"


def _other(rng, like, lo=None, hi=None):
    """A poison for an array: same shape and type, other valid contents."""
    like = np.asarray(like)
    if like.dtype.kind == "f":
        return rng.standard_normal(like.shape).astype(like.dtype)
    for _ in range(8):
        x = rng.integers(lo, hi, size=like.shape).astype(like.dtype)
        if not np.array_equal(x, like):
            return x
    raise AssertionError("no poison found")


def _other_offsets(rng, off):
    """Monotone offsets of the same length that start at 0 and end at the same total."""
    off = np.asarray(off)
    x = np.sort(rng.integers(0, int(off[-1]) + 1, size=len(off))).astype(off.dtype)
    x[0], x[-1] = 0, off[-1]
    assert (np.diff(x) >= 0).all() and not np.array_equal(x, off)
    return x


def _other_ids(rng, ids, lo, hi):
    """Another ascending list of distinct ids in [lo, hi), as long as `ids`."""
    x = np.sort(rng.choice(np.arange(lo, hi), size=len(ids), replace=False)).astype(np.int64)
    assert not np.array_equal(x, ids)
    return x


# ------------------------------------------------------------------ 1. forward
N_POS = 64
ROADS = {
    "one_launch": dict(fmt="int8", d=768, max_n=4, shape=(4, 64), fused=None, dt=torch.float16),     # k_embed_fused
    "two_kernels": dict(fmt="int8", d=768, max_n=4, shape=(4, 64), fused=0, dt=torch.float16),       # k_match_ell + k_embed_wave
    "generic": dict(fmt="fp32", d=64, max_n=3, shape=(2, 33), fused=None, dt=torch.float32),         # k_embed_wave_any
    "fp32_wave": dict(fmt="fp32", d=768, max_n=3, shape=(2, 33), fused=0, dt=torch.float32),         # the fp32 case; finalize's wave kernel
}
FORWARD = ["embed", "embed_varlen", "embed_base", "embed_base_varlen", "embed_select", "gather_reduce", "match", "match_csr"]
FORWARD_CASES = [(r, e) for r in ("one_launch", "two_kernels", "generic") for e in FORWARD] + \
                [("generic", "partial_finalize"), ("fp32_wave", "partial_finalize"), ("fp32_wave", "embed"), ("two_kernels", "embed_partial")]


class _World:
    pass


def _forward_world(name, **table_kw):
    """Table, truth and poison of every forward input, on one road."""
    cfg = ROADS[name]
    w = _World()
    w.name, w.fmt, w.d, w.max_n, w.dt = name, cfg["fmt"], cfg["d"], cfg["max_n"], cfg["dt"]
    w.keys, w.lens = E.vocabulary(w.max_n)
    w.n = len(w.lens)
    rng = np.random.default_rng(31 * w.d + w.max_n)
    w.rows = rng.standard_normal((w.n, w.d)).astype(np.float32)
    w.stored = _stored(w.rows, w.fmt)
    w.t = _table(w.max_n, w.n, w.d, w.fmt, cfg["fused"], **table_kw)
    w.t.index_build(w.keys, w.lens)
    w.t.store_f32(torch.from_numpy(w.rows))
    w.B, w.T = cfg["shape"]
    si = E.STREAM_SHAPES.index(cfg["shape"])
    w.tok, w.tok_p = (E.streams(w.max_n, seed)[si].astype(np.int32) for seed in (0, 1))
    w.ntok = w.B * w.T
    w.pos = rng.integers(0, N_POS, size=(w.B, w.T)).astype(np.int32)
    w.pos_p = _other(rng, w.pos, 0, N_POS)
    mk = lambda rows: WS._to(rng.standard_normal((rows, w.d)).astype(np.float32), w.dt)     # noqa: E731
    w.wte, w.wte_p, w.wpe, w.wpe_p = mk(3), mk(3), mk(N_POS), mk(N_POS)
    w.base, w.base_p = mk(w.ntok), mk(w.ntok)
    w.cu = np.asarray([0, 7, 7, 40, w.ntok - 3, w.ntok], dtype=np.int32)                     # an empty sequence among five
    w.cu_p = np.asarray([0, 3, 20, 21, w.ntok - 10, w.ntok], dtype=np.int32)
    w.sel = rng.permutation(w.ntok)[:17].astype(np.int32)
    w.sel_p = rng.permutation(w.ntok)[:17].astype(np.int32)
    w.rng = rng
    return w


_road = functools.lru_cache(maxsize=None)(_forward_world)


def _lists(w, tok_flat, cu):
    """CSR id lists over the flattened positions, every sequence matched on its own."""
    offs, ids, base = [np.zeros(1, dtype=np.int64)], [], 0
    for s in range(len(cu) - 1):
        if cu[s + 1] == cu[s]:
            continue
        off, i = R.hits_to_csr(R.match_hits(w.keys, w.lens, np.asarray(tok_flat[cu[s]:cu[s + 1]], dtype=np.int64)[None, :], w.max_n))
        offs.append(np.asarray(off[1:], dtype=np.int64) + base)
        ids.append(np.asarray(i, dtype=np.int64))
        base += int(off[-1])
    return np.concatenate(offs), (np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64))


def _lookup_ref(w, off, ids, base_t, wpe_t, pos, reduce="mean"):
    """cast((base + reduce_k row_k) + wpe[pos]) from the fp32 upcasts of what the kernel is given."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = R.embed_numpy(w.stored, off, ids, reduce).astype(np.float32)
        if base_t is not None:
            x = (base_t.float().numpy() + x).astype(np.float32)
        if wpe_t is not None:
            x = (x + wpe_t.float().numpy()[np.asarray(pos).reshape(-1)]).astype(np.float32)
    return WS._to(x, w.dt)


def _forward_case(w, entry):
    """(call, inputs, want, klass, host_want) of one forward entry point."""
    t = w.t
    rect = np.arange(w.B + 1, dtype=np.int64) * w.T
    tok = SF.Input(w.tok, w.tok_p)
    pos = SF.Input(w.pos, w.pos_p)
    wte, wpe = SF.Input(w.wte, w.wte_p), SF.Input(w.wpe, w.wpe_p)
    flat = w.tok.reshape(-1)
    wte_rows = w.wte[torch.from_numpy(flat.astype(np.int64))]
    host_want = None
    klass = A
    if entry in ("embed", "partial_finalize"):
        want = {"out": _lookup_ref(w, *_lists(w, flat, rect), wte_rows, w.wpe, w.pos)}
        inputs = [tok, pos, wte, wpe]
        if entry == "embed":
            def call():
                return {"out": t.embed(tok.buf, wte=wte.buf, wpe=wpe.buf, position_ids=pos.buf, out_dtype=w.dt)}, None
        else:
            def call():
                partial, counts = t.embed_partial(tok.buf)
                out = t.finalize(partial, counts, tok.buf, 0, w.ntok, wte=wte.buf, wpe=wpe.buf, position_ids=pos.buf, out_dtype=w.dt)
                return {"out": out, "counts": counts}, None
            want["counts"] = np.diff(_lists(w, flat, rect)[0]).astype(np.int32)
    elif entry == "embed_partial":
        off, ids = _lists(w, flat, rect)
        with np.errstate(over="ignore", invalid="ignore"):
            want = {"partial": R.embed_numpy(w.stored, off, ids, "sum").astype(np.float32), "counts": np.diff(off).astype(np.int32)}
        inputs = [tok]

        def call():
            partial, counts = t.embed_partial(tok.buf)
            return {"partial": partial, "counts": counts}, None
    elif entry in ("embed_varlen", "embed_base_varlen"):
        cu = SF.Input(w.cu, w.cu_p)
        tok1, pos1 = SF.Input(flat, w.tok_p.reshape(-1)), SF.Input(w.pos.reshape(-1), w.pos_p.reshape(-1))
        base = SF.Input(w.base, w.base_p)
        lists = _lists(w, flat, w.cu.astype(np.int64))
        if entry == "embed_varlen":
            want = {"out": _lookup_ref(w, *lists, wte_rows, w.wpe, w.pos)}
            inputs = [tok1, cu, pos1, wte, wpe]

            def call():
                return {"out": t.embed_varlen(tok1.buf, cu.buf, wte=wte.buf, wpe=wpe.buf, position_ids=pos1.buf, out_dtype=w.dt)}, None
        else:
            want = {"out": _lookup_ref(w, *lists, w.base, w.wpe, w.pos)}
            inputs = [tok1, cu, pos1, base, wpe]

            def call():
                return {"out": t.embed_base_varlen(tok1.buf, cu.buf, base.buf, wpe=wpe.buf, position_ids=pos1.buf, out_dtype=w.dt)}, None
    elif entry == "embed_base":
        base = SF.Input(w.base, w.base_p)
        want = {"out": _lookup_ref(w, *_lists(w, flat, rect), w.base, w.wpe, w.pos)}
        inputs = [tok, pos, base, wpe]

        def call():
            return {"out": t.embed_base(tok.buf, base.buf.view(w.B, w.T, w.d), wpe=wpe.buf, position_ids=pos.buf, out_dtype=w.dt)}, None
    elif entry == "embed_select":
        sel = SF.Input(w.sel, w.sel_p)
        pos_sel = SF.Input(w.pos.reshape(-1)[:17].copy(), w.pos_p.reshape(-1)[:17].copy())
        off, ids = _lists(w, flat, rect)
        at = w.sel.astype(np.int64)
        o2 = np.zeros(len(at) + 1, dtype=np.int64)
        np.cumsum((off[1:] - off[:-1])[at], out=o2[1:])
        i2 = np.concatenate([ids[off[p]:off[p + 1]] for p in at]) if len(at) else ids[:0]
        want = {"out": _lookup_ref(w, o2, i2, wte_rows[torch.from_numpy(at)], w.wpe, pos_sel.truth.cpu().numpy())}
        inputs = [tok, sel, pos_sel, wte, wpe]

        def call():
            return {"out": t.embed_select(tok.buf, sel.buf, wte=wte.buf, wpe=wpe.buf, position_ids=pos_sel.buf, out_dtype=w.dt)}, None
    elif entry == "gather_reduce":
        off, ids = _lists(w, flat, rect)
        offs = SF.Input(off.astype(np.int32), _other_offsets(w.rng, off.astype(np.int32)))
        idl = SF.Input(ids.astype(np.int32), _other(w.rng, ids.astype(np.int32), 0, w.n))
        base = SF.Input(w.base, w.base_p)
        want = {"out": _lookup_ref(w, off, ids, w.base, None, None)}
        inputs = [offs, idl, base]

        def call():
            return {"out": t.gather_reduce(offs.buf, idl.buf, "mean", base=base.buf, out_dtype=w.dt)}, None
    elif entry == "match":
        want = {"hits": R.match_hits(w.keys, w.lens, w.tok.astype(np.int64), w.max_n).astype(np.int32)}
        inputs = [tok]

        def call():
            return {"hits": t.match(tok.buf)}, None
    else:
        assert entry == "match_csr"
        off, ids = _lists(w, flat, rect)
        want = {"offsets": off.astype(np.int32), "ids": ids.astype(np.int32)}
        inputs, klass, host_want = [tok], S, int(off[-1])

        def call():
            o, i = t.match_csr(tok.buf)
            return {"offsets": o, "ids": i}, int(i.numel())
    return call, inputs, want, klass, host_want


@pytest.mark.parametrize("road,entry", FORWARD_CASES, ids=[f"{r}-{e}" for r, e in FORWARD_CASES])
def test_forward(road, entry):
    """scone_embed and its relatives, scone_gather_reduce, scone_match (A), scone_match_csr (S: *h_total), scone_embed_partial +
    scone_finalize (A), on the one-launch road, the two-kernel road and the any-dim kernel.  Inputs: tok, pos, wte / base, wpe,
    cu_seqlens, the selection, the caller's lists."""
    w = _road(road)
    call, inputs, want, klass, host_want = _forward_case(w, entry)
    res = SF.run(call, inputs, stream=SF.side_stream(w.t), table=w.t)
    _finish(res, klass, f"{entry} ({road})", want, host_want)


HOPS = ["cu_reserve_foreign_stream", "cu_reserve_own_stream", "staged_embed", "staged_prefetch"]


@pytest.mark.parametrize("hop", HOPS)
def test_cross_stream_hops(hop):
    """The library's own cross-stream hops.  CU reserve: from a foreign stream the lookup kernel goes to the handle's masked
    stream between two events (scone_lookup_enter / _leave); called on `lookup_stream()` itself it is launched there directly.
    Staging pipeline of a pinned-host table with stage_tokens > 0: chunks are matched and fetched on the handle's side streams
    behind the caller's stream and reduced on it; scone_embed_prefetch(tokens_ready = 0) starts them behind the delay and the
    scone_embed of the same batch takes them over.  (The pipeline's one synchronise per caller stream, its stream pick, is
    spent in the warm-up: the header's stated exception.)"""
    if hop.startswith("cu_reserve"):
        w = _forward_world("generic")                             # d = 64: every batch takes try_launch_wave, hence the hop
        w.t.set_cu_reserve(8)
        masked = w.t.lookup_stream()
        assert masked is not None
        stream = SF.side_stream(w.t, beside=(masked,), tag="cu") if hop == "cu_reserve_foreign_stream" else masked
    else:
        w = _forward_world("two_kernels", placement="pinned_host", hot_rows=8, stage_tokens=64)
        stream = SF.side_stream(w.t)
    call, inputs, want, klass, _ = _forward_case(w, "embed")
    if hop == "staged_prefetch":
        embed, tok = call, inputs[0]

        def call():                                              # noqa: F811
            w.t.embed_prefetch(tok.buf, tokens_ready=False)
            return embed()
    res = SF.run(call, inputs, stream=stream, table=w.t)
    _finish(res, klass, hop, want)
    if hop.startswith("staged"):
        assert w.t.stage_counters()["chunks"] > 0, "the staging pipeline did not run"


# ------------------------------------------------------------------ 2. table
TABLE_CASES = ["store_f32", "store_f32_ids", "SconeTable.store_f32", "upload_download-int8-768", "upload_download-int4-1024",
               "upload_download-mxfp4-1024", "gather_rows", "fill_synthetic", "index_build_device", "status"]


@functools.lru_cache(maxsize=None)
def _raw(fmt, d, n, seed):
    """(fp32 rows, raw payload, raw scales in the ABI's logical order) of a table in `fmt`, through a handle of its own."""
    rows = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    t = _table(3, n, d, fmt)
    t.store_f32(torch.from_numpy(rows))
    payload, scales = t.download(0, n)
    return rows, payload.copy(), scales.copy()


def _dequant(fmt, payload, scales):
    if fmt == "int8":
        return R.dequantize_i8(payload.view(np.int8), scales.reshape(-1))
    if fmt == "mxfp4":
        return MX.dequantize(payload, scales)
    return R.dequantize_i4(payload, scales)


@pytest.mark.parametrize("case", TABLE_CASES)
def test_table(case):
    """Table mutations and reads at the C level (`SconeTable.store_f32` synchronises by design: class S, asserted too).  After
    every mutation the table is read by a lookup on S in the same chain (`gather_rows` of every row): the mutation is ordered
    before its reader.  INT4 at d = 1024 keeps its scales in permuted slots, so upload and download launch a reorder kernel
    behind their copies."""
    L = _lib()
    lib = L.lib()
    rng = np.random.default_rng(len(case))
    if case.startswith("upload_download"):
        _, fmt, d = case.split("-")
        d, n = int(d), 48
        rows0, _, _ = _raw(fmt, d, n, 1)
        _, pay, sc = _raw(fmt, d, n, 2)
        _, pay_p, sc_p = _raw(fmt, d, n, 3)
        t = _table(3, n, d, fmt)
        t.store_f32(torch.from_numpy(rows0))
        lo, m = 8, 32                                             # rows [8, 40) are replaced
        p_in = SF.Input(pay[lo:lo + m], pay_p[lo:lo + m])
        s_in = SF.Input(sc[lo:lo + m].view(np.uint8), sc_p[lo:lo + m].view(np.uint8))
        out_p, out_s = torch.empty_like(p_in.buf), torch.empty_like(s_in.buf)

        def call():
            rc = lib.scone_table_upload(t._h, _ptr(p_in.buf), _ptr(s_in.buf), lo, m, 1, _cur())
            rc2 = lib.scone_table_download(t._h, _ptr(out_p), _ptr(out_s), lo, m, 1, _cur())
            assert rc == 0 and rc2 == 0
            return {}, None
        want_rows = _stored(rows0, fmt).copy()
        want_rows[lo:lo + m] = _dequant(fmt, pay[lo:lo + m], sc[lo:lo + m])
        res = SF.run(call, [p_in, s_in], stream=SF.side_stream(t), state={"table": SF.TableState(t)},
                     outputs={"payload": out_p, "scales": out_s}, table=t)
        _finish(res, A, case, {"table": want_rows, "payload": pay[lo:lo + m], "scales": sc[lo:lo + m].view(np.uint8)})
        return
    if case == "index_build_device":
        keys, lens = E.vocabulary(3)
        half = len(lens) // 2
        k_in = SF.Input(keys[:half].view(np.int32), keys[half:2 * half].view(np.int32))
        l_in = SF.Input(lens[:half], lens[half:2 * half])
        tok = E.streams(3)[5].astype(np.int32)
        want = R.match_hits(keys[:half], lens[:half], tok.astype(np.int64), 3).astype(np.int32)
        assert not np.array_equal(want, R.match_hits(keys[:2 * half], lens[:2 * half], tok.astype(np.int64), 3)), "the poison keys match nothing"
        t = _table(3, len(lens), 0, "fp32")
        tok_d = torch.from_numpy(tok).cuda()

        def call():                                              # built twice (warm-up, sequence): a duplicate key keeps its id
            t.index_build_device(k_in.buf, l_in.buf, id0=0)
            return {"hits": t.match(tok_d)}, None
        res = SF.run(call, [k_in, l_in], stream=SF.side_stream(t), table=t)
        _finish(res, A, case, {"hits": want})
        return
    fmt, d, n = "int8", 768, 64
    rows0, _, _ = _raw(fmt, d, n, 1)
    t = _table(3, n, d, fmt)
    t.store_f32(torch.from_numpy(rows0))
    state = {"table": SF.TableState(t)}
    want_rows = _stored(rows0, fmt).copy()
    new = rng.standard_normal((32, d)).astype(np.float32)
    r_in = SF.Input(new, _other(rng, new))
    klass, host_want, status, inputs = A, None, 0, [r_in]
    want, outputs = {}, {}
    if case == "store_f32":
        def call():
            assert lib.scone_table_store_f32(t._h, _ptr(r_in.buf), 8, 32, _cur()) == 0
            return {}, None
        want_rows[8:40] = _stored(new, fmt)
    elif case == "SconeTable.store_f32":
        klass = S                                                # "`rows`/`ids` may be temporaries": the wrapper waits for the kernel

        def call():
            t.store_f32(r_in.buf, row0=8)
            return {}, None
        want_rows[8:40] = _stored(new, fmt)
    elif case == "store_f32_ids":
        ids = np.sort(rng.choice(n, size=32, replace=False)).astype(np.int64)
        i_in = SF.Input(ids, _other_ids(rng, ids, 0, n))
        inputs.append(i_in)

        def call():
            assert lib.scone_table_store_f32_ids(t._h, _ptr(r_in.buf), _ptr(i_in.buf), 32, _cur()) == 0
            return {}, None
        want_rows[ids] = _stored(new, fmt)
    elif case == "gather_rows":
        ids = rng.integers(0, n, size=40).astype(np.int64)
        i_in = SF.Input(ids, _other(rng, ids, 0, n))
        inputs, state = [i_in], {}
        out = torch.empty((40, d), dtype=torch.float32, device="cuda")

        outputs["rows"] = out

        def call():
            assert lib.scone_table_gather_rows(t._h, _ptr(i_in.buf), 40, _ptr(out), _cur()) == 0
            return {}, None
        want["rows"] = want_rows[ids]
    elif case == "fill_synthetic":
        seed, scale = 77, 0.02 / 127                              # a store queued on S just before must lose against the fill

        def call():
            assert lib.scone_table_store_f32(t._h, _ptr(r_in.buf), 8, 32, _cur()) == 0
            assert lib.scone_table_fill_synthetic(t._h, seed, scale, _cur()) == 0
            return {}, None
        all_ids = np.arange(n)
        want_rows = R.synth_rows_i8(seed, all_ids, d).astype(np.float32) * R.synth_scale_f16(seed, all_ids, scale).astype(np.float32)[:, None]
    else:
        assert case == "status"
        wte = WS._to(rng.standard_normal((3, d)).astype(np.float32), torch.float16).cuda()
        t.index_build(*E.vocabulary(3))
        tok = E.streams(3)[4].astype(np.int32)
        bad = tok.copy()
        bad[1, 5] = 3                                             # == vocab: defined, a row of +0.0, and bit 0 of the status
        tok_in = SF.Input(bad, E.streams(3, 1)[4].astype(np.int32))
        inputs, state, klass, host_want = [tok_in], {}, S, L.ST_BAD_TOKEN

        def call():
            out = t.embed(tok_in.buf, wte=wte, out_dtype=torch.float16)
            return {"out": out}, t.status()
    if state:
        want["table"] = want_rows
    res = SF.run(call, inputs, stream=SF.side_stream(t), state=state, outputs=outputs, table=t)
    _finish(res, klass, case, want, host_want, status)


# ------------------------------------------------------------------ 3. backward
BWD_D = 64
PLANS = {"rect": ("r37", 3), "packed": ("small", 4)}             # rows of one chunk only / rows of several chunks


def _plan_inputs(batch, max_n):
    tok, cu = TB._batch(batch, max_n)
    rng = np.random.default_rng(len(tok))
    return tok, cu, np.roll(tok, 5), _other_offsets(rng, cu)


def _owned_refs(batch, max_n):
    off, ids = TB._lists(batch, max_n, "cover")
    return len(BW.references(off, ids, 0, None, TB.N_ROWS[max_n])[0])


def _assert_chunks(batch, max_n):
    lens = BW.row_lengths(*TB._lists(batch, max_n, "cover"))[1]
    if batch == "small":
        assert lens.max() > TB._chunk(), "no row of several chunks: the partials launch is not reached"
    else:
        assert lens.max() <= TB._chunk(), "a row of several chunks in the one-chunk plan"


@pytest.mark.parametrize("form", ["rect", "packed", "csr"])
def test_backward_plan(form):
    """scone_backward_plan / _varlen / _plan_csr (S): U and the reference count come back through a synchronise of S, and
    `rows` on S right behind the plan reads the plan's buffers complete."""
    batch, max_n = PLANS["rect" if form == "csr" else form]
    t = TB._table(max_n, BWD_D)
    tok, cu, tok_p, cu_p = _plan_inputs(batch, max_n)
    off, ids = TB._lists(batch, max_n, "cover")
    g = TB._grad(len(off) - 1, BWD_D, "fp16")
    g_d = g.cuda()
    want_ids, want_rows = TB._want(batch, max_n, "cover", "mean", BWD_D, "fp16")
    if form == "rect":
        B, T = TB.RECTS[batch]
        x = SF.Input(tok.reshape(B, T).astype(np.int32), tok_p.reshape(B, T).astype(np.int32))
        inputs, make = [x], lambda: t.backward_plan(x.buf)
    elif form == "packed":
        x, c = SF.Input(tok.astype(np.int32), tok_p.astype(np.int32)), SF.Input(cu.astype(np.int32), cu_p.astype(np.int32))
        inputs, make = [x, c], lambda: t.backward_plan(x.buf, c.buf)
    else:
        rng = np.random.default_rng(3)
        o = SF.Input(off.astype(np.int32), _other_offsets(rng, off.astype(np.int32)))
        i = SF.Input(ids.astype(np.int32), _other(rng, ids.astype(np.int32), 0, TB.N_ROWS[max_n]))
        inputs, make = [o, i], lambda: t.backward_plan_csr(o.buf, i.buf)
    plans = []

    def call():
        plan = make()
        plans.append(plan)                                       # freeing a plan waits for the device: after the sequence
        rid, rows = plan.rows(g_d, "mean")
        return {"ids": rid, "rows": rows}, (plan.n_rows, plan.n_refs)
    res = SF.run(call, inputs, stream=SF.side_stream(t), table=t)
    _finish(res, S, f"backward_plan ({form})", {"ids": want_ids, "rows": want_rows}, (len(want_ids), _owned_refs(batch, max_n)))
    for p in plans:
        p.close()


ROWS_CASES = [("rows", "rect", "fp16"), ("rows", "packed", "fp16"), ("rows", "packed", "fp32"), ("counts", "packed", None),
              ("row_ids", "packed", None), ("rows_acc", "rect", "fp16"), ("rows_acc", "packed", "fp16"),
              ("apply_lean-fp32-sgd", "packed", "fp16"), ("apply_lean-bf16-rowwise_adagrad", "rect", "fp16")]


@pytest.mark.parametrize("entry,plan_kind,dtype", ROWS_CASES, ids=[f"{e}-{p}-{d}" for e, p, d in ROWS_CASES])
def test_backward_rows(entry, plan_kind, dtype):
    """scone_backward_rows / _counts / _row_ids / _rows_acc / _apply_lean (A) on a plan made beforehand: with rows of several
    chunks (the partials launch and the combine behind it) and without."""
    L = _lib()
    lib = L.lib()
    batch, max_n = PLANS[plan_kind]
    _assert_chunks(batch, max_n)
    n = TB.N_ROWS[max_n]
    tok, cu = TB._batch(batch, max_n)
    off, ids = TB._lists(batch, max_n, "cover")
    ntok = len(off) - 1
    d = 768 if entry.startswith("apply_lean") else BWD_D
    fmt = entry.split("-")[1] if entry.startswith("apply_lean") else "fp32"
    t = TB._table(max_n, d, fmt=fmt)
    plan = TB._plan(t, batch, max_n)
    torch.cuda.synchronize()
    U = plan.n_rows
    want_ids = TB._want(batch, max_n, "cover", "mean", d, dtype or "fp16")[0]
    assert U == len(want_ids)
    stream = SF.side_stream(t)
    who = f"{entry} ({plan_kind})"
    if entry in ("counts", "row_ids"):
        if entry == "counts":
            out = torch.empty(ntok, dtype=torch.int32, device="cuda")
            fn, want = (lambda: lib.scone_backward_counts(t._h, plan._p, _ptr(out), _cur())), np.diff(off).astype(np.int32)
        else:
            out = torch.empty(U, dtype=torch.int64, device="cuda")
            fn, want = (lambda: lib.scone_backward_row_ids(t._h, plan._p, _ptr(out), U, _cur())), want_ids

        def call():
            assert fn() == 0
            return {}, None
        res = SF.run(call, [], stream=stream, outputs={"out": out}, table=t)
        _finish(res, A, who, {"out": want})
        return
    g = TB._grad(ntok, d, dtype)
    g_in = SF.Input(g, TB._grad(ntok, d, dtype, seed=9))
    g32 = TB._g32(g)
    want_rows = TB._want(batch, max_n, "cover", "mean", d, dtype)[1]
    if entry == "rows":
        out_ids = torch.empty(U, dtype=torch.int64, device="cuda")
        out_rows = torch.empty((U, d), dtype=torch.float32, device="cuda")

        def call():
            plan.rows(g_in.buf, "mean", out=(out_ids, out_rows))
            return {}, None
        res = SF.run(call, [g_in], stream=stream, outputs={"ids": out_ids, "rows": out_rows}, table=t)
        _finish(res, A, who, {"ids": want_ids, "rows": want_rows})
        return
    if entry == "rows_acc":
        rng = np.random.default_rng(5)
        old_ids = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.int64)        # the "interleaved" relation
        old_rows = rng.standard_normal((len(old_ids), d)).astype(np.float32)
        m_ids, src_a, src_b, _, pos_b = GM.merge_map(old_ids, want_ids)
        assert 0 < len(np.intersect1d(old_ids, want_ids)) < min(len(old_ids), U)
        want = GM.merge_rows(src_a, src_b, old_rows, want_rows)
        n_out = len(m_ids)
        # poison maps: every entry stays what the kernels may index with (absent, or an index inside its list; an output row)
        sa, sb, pb = (SF.Input(x.view(np.int32), x[::-1].copy().view(np.int32)) for x in (src_a, src_b, pos_b))
        r_in = SF.Input(old_rows, _other(rng, old_rows))
        out = torch.empty((n_out, d), dtype=torch.float32, device="cuda")

        def call():
            rc = lib.scone_backward_rows_acc(t._h, plan._p, _ptr(g_in.buf), L.DT_F16, L.REDUCE_MEAN, _ptr(sa.buf), _ptr(sb.buf),
                                             _ptr(pb.buf), n_out, _ptr(r_in.buf), _ptr(out), _cur())
            assert rc == 0
            return {}, None
        res = SF.run(call, [g_in, sa, sb, pb, r_in], stream=stream, outputs={"rows": out}, table=t)
        _finish(res, A, who, {"rows": want})
        return
    # apply_lean: the served rows are the weights
    from scone_amd.hip_backend import lean_scalars
    kind = entry.split("-")[2]
    rng = np.random.default_rng(13)
    w0 = rng.standard_normal((n, d)).astype(np.float32)
    t.store_f32(torch.from_numpy(w0))
    s0 = (rng.standard_normal(n) ** 2).astype(np.float32)
    row_state = torch.from_numpy(s0).cuda()
    hp = dict(lr=0.05, eps=1e-10, weight_decay=0.01)
    sc = lean_scalars(kind, **hp)
    state = {"table": SF.TableState(t)}
    if kind == "rowwise_adagrad":
        state["row_state"] = SF.TensorState(row_state)
    if fmt == "fp32":
        want_w, want_s, _, _ = LF.apply(kind, sc, want_ids, want_rows, w0, s0)
    else:
        bits, want_s, _, _, _ = LF.apply_bf16(kind, sc, want_ids, want_rows, BF.to_bf16_bits(w0), s0, rounding=LF.STOCHASTIC, seed=11,
                                              step_no=3)
        want_w = BF.from_bf16_bits(bits)

    def call():
        plan.apply_lean(g_in.buf, "mean", kind=kind, row_state=row_state if kind == "rowwise_adagrad" else None,
                        rounding="stochastic" if fmt == "bf16" else "nearest", seed=11, step=3, **hp)
        return {}, None
    res = SF.run(call, [g_in], stream=stream, state=state, table=t)
    want = {"table": want_w}
    if kind == "rowwise_adagrad":
        want["row_state"] = want_s
    _finish(res, A, who, want)


# ------------------------------------------------------------------ 4. accumulate
def _interleaved(n=90, d=BWD_D, seed=0):
    """Two ascending id lists of equal length that interleave and share a third of their ids, and their rows."""
    rng = np.random.default_rng(100 + seed)
    pool = np.sort(rng.choice(400, size=2 * n, replace=False)).astype(np.int64)
    a, b = pool[0::2].copy(), pool[1::2].copy()
    b[::3] = a[::3]
    b = np.unique(b)
    a = a[:len(b)]
    assert len(a) == len(b) and 0 < len(np.intersect1d(a, b)) < len(a)
    return a, b, GM.edge_rows(len(a), d, seed + 1), GM.edge_rows(len(b), d, seed + 2)


@pytest.mark.parametrize("entry", ["merge_map-no_count", "merge_map-count", "merge_rows"])
def test_accumulate(entry):
    """scone_grad_merge_map with h_n_out == NULL (A) and != NULL (S, n_out), scone_grad_merge_rows (A)."""
    d = BWD_D
    t = _table(3, 400, d, "fp32")
    a, b, rows_a, rows_b = _interleaved()
    a_p, b_p, _, _ = _interleaved(seed=7)
    ids, src_a, src_b, pos_a, pos_b = GM.merge_map(a, b)
    n_out, cap = len(ids), len(a) + len(b)
    stream = SF.side_stream(t)
    if entry.startswith("merge_map"):
        sync = entry.endswith("-count")
        a_in, b_in = SF.Input(a, a_p[:len(a)]), SF.Input(b, b_p[:len(b)])
        assert GM.is_valid(a_in.poison.cpu().numpy()) and GM.is_valid(b_in.poison.cpu().numpy())

        def call():
            m = t.grad_merge_map(a_in.buf, b_in.buf, sync=sync)
            return {"ids": m.ids[:n_out], "src_a": m.src_a, "src_b": m.src_b, "pos_a": m.pos_a, "pos_b": m.pos_b, "n_out": m.d_n_out}, m.n_out
        pad = np.full(0 if sync else cap - n_out, -1, dtype=np.int64)       # the library's "absent", as the wrapper's int32 shows it
        want = {"ids": ids, "src_a": np.concatenate([src_a.view(np.int32), pad]), "src_b": np.concatenate([src_b.view(np.int32), pad]),
                "pos_a": pos_a.view(np.int32), "pos_b": pos_b.view(np.int32), "n_out": np.asarray([n_out])}
        res = SF.run(call, [a_in, b_in], stream=stream, table=t)
        _finish(res, S if sync else A, entry, want, n_out if sync else None)
        assert sync or res.host is None
        return
    from scone_amd.hip_backend import GradMergeMap
    rng = np.random.default_rng(1)
    # poison maps: a's and b's exchanged -- the lists are equally long, so every entry stays an index inside its list
    sa, sb = SF.Input(src_a.view(np.int32), src_b.view(np.int32)), SF.Input(src_b.view(np.int32), src_a.view(np.int32))
    ra, rb = SF.Input(rows_a, _other(rng, rows_a)), SF.Input(rows_b, _other(rng, rows_b))
    m = GradMergeMap(None, sa.buf, sb.buf, torch.from_numpy(pos_a.view(np.int32)).cuda(), torch.from_numpy(pos_b.view(np.int32)).cuda(),
                     None, n_out)
    out = torch.empty((n_out, d), dtype=torch.float32, device="cuda")

    def call():
        t.grad_merge_rows(m, ra.buf, rb.buf, out=out)
        return {}, None
    res = SF.run(call, [sa, sb, ra, rb], stream=stream, outputs={"rows": out}, table=t)
    SF.check_class(res, A, entry)
    ok = GM.same_bits(res.out["rows"], GM.merge_rows(src_a, src_b, rows_a, rows_b))        # (a NaN matches any NaN: a + b)
    assert ok, f"{entry}: rows differ from the reference ({res.describe()})"
    assert res.status == 0


# ------------------------------------------------------------------ 5. optimizer, norm and clip
OPT_N = 300
HP = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


class _Opt:
    """A table stored from a random master, optimizer state, and truth / poison of an id list and its gradient rows."""

    def __init__(self, fmt, d, seed, in_place=False):
        rng = np.random.default_rng(seed)
        n = OPT_N
        self.fmt, self.d, self.rng = fmt, d, rng
        self.w = rng.standard_normal((n, d)).astype(np.float32)
        self.m = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
        self.v = (rng.standard_normal((n, d)) ** 2).astype(np.float32)
        self.s = (rng.standard_normal(n) ** 2).astype(np.float32)
        self.t = _table(3, n, d, fmt)
        self.t.store_f32(torch.from_numpy(self.w))
        if in_place:
            self.w = _stored(self.w, fmt)                        # the served rows are the weights
        self.ids = np.unique(np.concatenate([rng.choice(n - 1, size=100, replace=False), [0, n - 2]])).astype(np.int64)
        self.ids_p = _other_ids(rng, self.ids, 0, n)
        self.g = rng.standard_normal((len(self.ids), d)).astype(np.float32)
        self.ids_in, self.g_in = SF.Input(self.ids, self.ids_p), SF.Input(self.g, _other(rng, self.g))
        self.master, self.s1, self.s2, self.rs = (torch.from_numpy(x.copy()).cuda() for x in (self.w, self.m, self.v, self.s))
        assert n - 1 not in self.ids, "every test compares a neighbouring row that is not listed"

    def state(self, *names):
        st = {"table": SF.TableState(self.t)}
        for k in names:
            st[k] = SF.TensorState({"master": self.master, "state1": self.s1, "state2": self.s2, "row_state": self.rs}[k])
        return st


OPT_CASES = ["step-sgd", "step-adagrad", "step-adam", "lean-master", "lean-fp32-in_place", "lean-bf16-stochastic"]


def _opt_want(o, kind, sc, lean, in_place=False, stochastic=None):
    """name -> expected array after one step with scalars `sc` (None: the step is skipped, nothing changes)."""
    want = {"master": o.w, "state1": o.m, "state2": o.v, "row_state": o.s}
    if sc is not None and not lean:
        w, m, v, _, bad = OF.apply(kind, sc, o.ids, o.g, o.w, o.m if kind == "adam" else None, o.v if kind != "sgd" else None, 0, OPT_N)
        assert not bad
        want.update(master=w, state1=m if kind == "adam" else o.m, state2=v if kind != "sgd" else o.v)
    elif sc is not None and stochastic is None:
        w, s, _, bad = LF.apply(kind, sc, o.ids, o.g, o.w, o.s if kind == "rowwise_adagrad" else None)
        assert not bad
        want.update(master=w, row_state=s if kind == "rowwise_adagrad" else o.s)
    elif sc is not None:
        bits, s, _, bad, _ = LF.apply_bf16(kind, sc, o.ids, o.g, BF.to_bf16_bits(o.w), o.s, rounding=LF.STOCHASTIC, **stochastic)
        assert not bad
        want.update(master=BF.from_bf16_bits(bits), row_state=s)
    want["table"] = want["master"] if in_place else _stored(want["master"], o.fmt)
    return want


@pytest.mark.parametrize("case", OPT_CASES)
def test_optimizer(case):
    """scone_opt_step (A) for SGD / Adagrad / Adam on an INT8 served table (re-quantised in the same launch) and
    scone_opt_step_lean (A) in master mode, in place on fp32 rows and in place on bf16 rows with stochastic rounding.  Master,
    state, row state and the served rows are all compared whole, so a neighbouring row that is not listed is among them."""
    from scone_amd.hip_backend import lean_scalars, opt_scalars
    if case.startswith("step"):
        kind = case.split("-")[1]
        o = _Opt("int8", 768, 1)
        names = ("master",) + (("state1",) if kind == "adam" else ()) + (("state2",) if kind != "sgd" else ())
        want = _opt_want(o, kind, opt_scalars(kind, step=2, **HP), lean=False)

        def call():
            o.t.opt_step(o.ids_in.buf, o.g_in.buf, o.master, kind=kind, step=2, state1=o.s1 if kind == "adam" else None,
                         state2=o.s2 if kind != "sgd" else None, **HP)
            return {}, None
    else:
        kind, hp = "rowwise_adagrad", dict(lr=0.05, eps=1e-10, weight_decay=0.01)
        sc = lean_scalars(kind, **hp)
        if case == "lean-master":
            o = _Opt("int8", 768, 2)
            names, want = ("master", "row_state"), _opt_want(o, kind, sc, lean=True)
            kw = dict(master=o.master)
        elif case == "lean-fp32-in_place":
            o = _Opt("fp32", 64, 3, in_place=True)
            names, want = ("row_state",), _opt_want(o, kind, sc, lean=True, in_place=True)
            kw = {}
        else:
            o = _Opt("bf16", 768, 4, in_place=True)
            names, want = ("row_state",), _opt_want(o, kind, sc, lean=True, in_place=True, stochastic=dict(seed=5, step_no=2))
            kw = dict(rounding="stochastic", seed=5, step=2)

        def call():
            o.t.opt_step_lean(o.ids_in.buf, o.g_in.buf, kind=kind, row_state=o.rs, **hp, **kw)
            return {}, None
    res = SF.run(call, [o.ids_in, o.g_in], stream=SF.side_stream(o.t), state=o.state(*names), table=o.t)
    _finish(res, A, case, {k: want[k] for k in names + ("table",)})


def _ctl_bytes(fields):
    from scone_amd.hip_backend import GradCtl
    rec = np.zeros(1, dtype=GradCtl._DTYPE)
    for k, v in fields.items():
        rec[k] = v
    return rec.view(np.float64).copy()


NORM_CASES = ["sqnorm", "ctl_set", "step_ctl-poison_skip", "step_ctl-poison_coef", "lean_ctl-poison_skip", "chain-clip", "chain-skip"]


@pytest.mark.parametrize("case", NORM_CASES)
def test_norm_and_clip(case):
    """scone_grad_sqnorm, scone_grad_ctl_set, scone_opt_step_ctl, scone_opt_step_lean_ctl (A).  A control block handed to a
    step is poisoned as skip = 1 and as coef = 0.5; the chain sqnorm -> ctl_set -> step_ctl runs as three calls behind ONE delay
    with nothing read back in between, once with a gradient that is clipped (skip = 0) and once with one that holds an inf
    (skip = 1: the step changes nothing)."""
    from scone_amd.hip_backend import GradCtl, lean_scalars, opt_scalars
    o = _Opt("int8", 768, 6)
    t, kind, gs, max_norm = o.t, "adam", 0.5, 3.0
    stream = SF.side_stream(t)
    if case == "chain-skip":
        o.g[7, 5] = np.inf
        o.g_in = SF.Input(o.g, o.g_in.poison)
    with np.errstate(over="ignore", invalid="ignore"):
        total, row_sq, _ = GN.sqnorm(o.g)
    block = GN.ctl([total], gs, max_norm, True)
    assert block["skip"] == int(case == "chain-skip") and (block["skip"] or block["coef"] < 1.0)
    if case == "sqnorm":
        def call():
            sq, rows = t.grad_sqnorm(o.g_in.buf)
            return {"sq": sq.reshape(1), "row_sq": rows}, None
        res = SF.run(call, [o.g_in], stream=stream, table=t)
        _finish(res, A, case, {})
        assert np.array_equal(GN.bits64(res.out["sq"]), GN.bits64(total)) and np.array_equal(GN.bits64(res.out["row_sq"]), GN.bits64(row_sq))
        return
    if case == "ctl_set":
        terms = np.asarray([total, 2.5, 0.125])
        t_in = SF.Input(terms, np.asarray([1.0, 2.0, 3.0]))
        want = GN.ctl(terms, gs, max_norm, True)

        def call():
            return {"ctl": t.grad_ctl(t_in.buf, grad_scale=gs, max_norm=max_norm, skip_nonfinite=True).buf}, None
        res = SF.run(call, [t_in], stream=stream, table=t)
        _finish(res, A, case, {})
        assert np.array_equal(GN.bits64(res.out["ctl"]), GN.bits64(_ctl_bytes(want))), (res.out["ctl"], want)
        return
    names = ("master", "state1", "state2")
    lean = case.startswith("lean_ctl")
    if lean:
        kind, names = "rowwise_adagrad", ("master", "row_state")
        hp = dict(lr=0.05, eps=1e-10, weight_decay=0.01)
        sc = lean_scalars(kind, grad_scale=gs, **hp)
    else:
        sc = opt_scalars(kind, step=2, grad_scale=gs, **HP)
    if not block["skip"]:
        sc = dict(sc, gscale=np.float32(sc["gscale"] * block["coef"]))      # ONE fp32 product of the cfg's gscale and the block's coef
    want = _opt_want(o, kind, None if block["skip"] else sc, lean=lean)
    ctl = GradCtl(t.device)
    if case.startswith("chain"):
        def call():
            sq, _ = t.grad_sqnorm(o.g_in.buf)
            c = t.grad_ctl([sq], grad_scale=gs, max_norm=max_norm, skip_nonfinite=True)
            t.opt_step(o.ids_in.buf, o.g_in.buf, o.master, kind=kind, step=2, state1=o.s1, state2=o.s2, grad_scale=gs, ctl=c, **HP)
            return {"ctl": c.buf}, None
        inputs = [o.ids_in, o.g_in]
    else:
        poison = dict(block, skip=1) if case.endswith("poison_skip") else dict(block, coef=np.float32(0.5))
        c_in = SF.Input(_ctl_bytes(block), _ctl_bytes(poison))
        ctl.buf = c_in.buf
        inputs = [o.ids_in, o.g_in, c_in]
        if lean:
            def call():
                t.opt_step_lean(o.ids_in.buf, o.g_in.buf, kind=kind, master=o.master, row_state=o.rs, grad_scale=gs, ctl=ctl, **hp)
                return {}, None
        else:
            def call():
                t.opt_step(o.ids_in.buf, o.g_in.buf, o.master, kind=kind, step=2, state1=o.s1, state2=o.s2, grad_scale=gs, ctl=ctl, **HP)
                return {}, None
    res = SF.run(call, inputs, stream=stream, state=o.state(*names), table=t)
    _finish(res, A, case, {k: want[k] for k in names + ("table",)})
    if case.startswith("chain"):
        assert np.array_equal(GN.bits64(res.out["ctl"]), GN.bits64(_ctl_bytes(block)))


# ------------------------------------------------------------------ 6. the Python layer
_SYNC_DEBUG = None


def _no_torch_sync(fn):
    """Run a class-A call under torch.cuda.set_sync_debug_mode("error") where this build honours it: a synchronising torch
    call inside the wrappers (.item(), .cpu(), a blocking copy) raises.  The library's own synchronisations are `busy`'s."""
    global _SYNC_DEBUG
    if _SYNC_DEBUG is None:
        _SYNC_DEBUG = SF.sync_debug_honoured()

    def wrapped():
        if not _SYNC_DEBUG:
            return fn()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn()
        finally:
            torch.cuda.set_sync_debug_mode(before)
    return wrapped


def test_sync_debug_mode_is_honoured():
    """The optional variant: on a build whose set_sync_debug_mode does nothing, the class-A cases of the Python layer rely on
    `busy` alone, and this case says so."""
    if not SF.sync_debug_honoured():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build: the Python-layer cases rely on `busy`")


def _module(which, d=BWD_D, max_n=4):
    from scone_amd.training import InPlaceFGramTable, TrainableFGramTable
    n = TB.N_ROWS[max_n]
    w0 = np.random.default_rng(41).standard_normal((n, d)).astype(np.float32)
    if which == "trainable":
        cache = TB._cache("int8", d, max_n, "cover", torch.from_numpy(w0))
        return TrainableFGramTable(cache, torch.from_numpy(w0.copy())), w0, "int8"
    cache = TB._cache("fp32", d, max_n, "cover", torch.from_numpy(w0))
    return InPlaceFGramTable(cache), w0, "fp32"


PY_CASES = ["rows", "rows-accumulate", "apply_lean", "grad_merge", "step-max_norm-trainable", "step-max_norm-in_place", "step-skipped",
            "accumulate-trainable", "accumulate-in_place"]


@pytest.mark.parametrize("case", PY_CASES)
def test_python_layer(case):
    """The wrappers a training loop calls, run on S behind the delay: BackwardPlan.rows (A), rows(accumulate=) (S: the size of
    the union), apply_lean (A), SconeTable.grad_merge (S), FGramOptimizer.step(max_norm=, skip_nonfinite=True) (A: the "without
    a sync" road -- grad_sqnorm, grad_ctl and the _ctl step with nothing read back) and the modules' _accumulate over two
    micro-batches (S: one synchronise, in the second).  Class-A cases also run under torch's sync debug mode where honoured."""
    from scone_amd.hip_backend import lean_scalars, opt_scalars
    from scone_amd.training import FGramOptimizer
    max_n, d, batch = 4, BWD_D, "small"
    n = TB.N_ROWS[max_n]
    off, ids = TB._lists(batch, max_n, "cover")
    ntok = len(off) - 1
    g = TB._grad(ntok, d, "fp16")
    want_ids, want_rows = TB._want(batch, max_n, "cover", "mean", d, "fp16")
    rng = np.random.default_rng(17)
    old_ids = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.int64)
    old_rows = rng.standard_normal((len(old_ids), d)).astype(np.float32)
    m_ids, m_rows = GM.merge(old_ids, old_rows, want_ids, want_rows)
    if case in ("rows", "rows-accumulate", "apply_lean", "grad_merge"):
        t = TB._table(max_n, d)
        plan = TB._plan(t, batch, max_n)
        torch.cuda.synchronize()
        stream = SF.side_stream(t)
        g_in = SF.Input(g, TB._grad(ntok, d, "fp16", seed=9))
        if case == "rows":
            def call():
                rid, rows = plan.rows(g_in.buf, "mean")
                return {"ids": rid, "rows": rows}, None
            res = SF.run(_no_torch_sync(call), [g_in], stream=stream, table=t)
            _finish(res, A, case, {"ids": want_ids, "rows": want_rows})
        elif case == "apply_lean":
            w0 = rng.standard_normal((n, d)).astype(np.float32)
            t.store_f32(torch.from_numpy(w0))
            hp = dict(lr=0.05, eps=1e-10, weight_decay=0.0)

            def call():
                plan.apply_lean(g_in.buf, "mean", kind="sgd", **hp)
                return {}, None
            res = SF.run(_no_torch_sync(call), [g_in], stream=stream, state={"table": SF.TableState(t)}, table=t)
            _finish(res, A, case, {"table": LF.apply("sgd", lean_scalars("sgd", **hp), want_ids, want_rows, w0)[0]})
        else:
            i_in = SF.Input(old_ids, _other_ids(rng, old_ids, 0, n))
            r_in = SF.Input(old_rows, _other(rng, old_rows))
            if case == "rows-accumulate":
                def call():
                    rid, rows = plan.rows(g_in.buf, "mean", accumulate=(i_in.buf, r_in.buf))
                    return {"ids": rid, "rows": rows}, int(rid.numel())
                inputs = [g_in, i_in, r_in]
            else:
                new_i, new_r = SF.Input(want_ids, _other_ids(rng, want_ids, 0, n)), SF.Input(want_rows, _other(rng, want_rows))

                def call():
                    rid, rows = t.grad_merge(i_in.buf, r_in.buf, new_i.buf, new_r.buf)
                    return {"ids": rid, "rows": rows}, int(rid.numel())
                inputs = [i_in, r_in, new_i, new_r]
            res = SF.run(call, inputs, stream=stream, table=t)
            _finish(res, S, case, {"ids": m_ids, "rows": m_rows}, len(m_ids))
        plan.close()
        return
    which = "in_place" if case.endswith("in_place") else "trainable"
    module, w0, fmt = _module(which, d, max_n)
    t = module.cache.to_device()
    stream = SF.side_stream(t)
    i_in = SF.Input(old_ids, _other_ids(rng, old_ids, 0, n))
    r_in = SF.Input(old_rows, _other(rng, old_rows))

    def set_grad(ids_t, rows_t):
        if which == "in_place":
            module.grad = (ids_t, rows_t)
        else:
            module.weight.grad = torch.sparse_coo_tensor(ids_t[None], rows_t, tuple(module.weight.shape), is_coalesced=True)

    def clear_grad():
        if which == "in_place":
            module.grad = None
        else:
            module.weight.grad = None

    if case.startswith("accumulate"):
        new_i, new_r = SF.Input(want_ids, _other_ids(rng, want_ids, 0, n)), SF.Input(want_rows, _other(rng, want_rows))

        def call():
            clear_grad()
            module._accumulate(i_in.buf, r_in.buf)                # the first micro-batch: the gradient is set, nothing is launched
            module._accumulate(new_i.buf, new_r.buf)              # the second: scone_grad_merge_map (one synchronise) + _rows
            rid, rows = module.grad if which == "in_place" else (module.weight.grad._indices()[0], module.weight.grad._values())
            return {"ids": rid, "rows": rows}, int(rid.numel())
        res = SF.run(call, [i_in, r_in, new_i, new_r], stream=stream, table=t)
        _finish(res, S, case, {"ids": m_ids, "rows": m_rows}, len(m_ids))
        return
    # FGramOptimizer.step(max_norm=, skip_nonfinite=True)
    kind = "sgd" if which == "in_place" else "adam"
    gs, max_norm = 0.5, 1.0
    g_rows = old_rows.copy()
    if case == "step-skipped":
        g_rows[3, 1] = np.inf
        r_in = SF.Input(g_rows, r_in.poison)
    opt = FGramOptimizer(module, kind, lr=0.05, weight_decay=0.01)
    opt._ensure_state()
    with np.errstate(over="ignore", invalid="ignore"):
        block = GN.ctl([GN.sqnorm(g_rows)[0]], gs, max_norm, True)
    assert block["skip"] == int(case == "step-skipped") and (block["skip"] or block["coef"] < 1.0)
    if which == "in_place":
        sc = lean_scalars(kind, lr=0.05, eps=opt.eps, weight_decay=0.01, grad_scale=gs)
        sc = dict(sc, gscale=np.float32(sc["gscale"] * block["coef"]))
        want = {"table": LF.apply(kind, sc, old_ids, g_rows, w0)[0]}
        state = {"table": SF.TableState(t)}
    else:
        sc = opt_scalars(kind, lr=0.05, betas=opt.betas, eps=opt.eps, weight_decay=0.01, grad_scale=gs, step=1)
        sc = dict(sc, gscale=np.float32(sc["gscale"] * block["coef"]))
        zero = np.zeros_like(w0)
        if block["skip"]:
            w1, m1, v1 = w0, zero, zero
        else:
            w1, m1, v1, _, _ = OF.apply(kind, sc, old_ids, g_rows, w0, zero, zero, 0, n)
        want = {"master": w1, "state1": m1, "state2": v1, "table": _stored(w1, fmt)}
        state = {"table": SF.TableState(t), "master": SF.TensorState(module.weight.data), "state1": SF.TensorState(opt.state1),
                 "state2": SF.TensorState(opt.state2)}

    def reset():
        opt.t = 0

    def call():
        set_grad(i_in.buf, r_in.buf)
        assert opt.step(gs, max_norm=max_norm, skip_nonfinite=True) == len(old_ids)
        return {"ctl": opt.last_ctl.buf}, None
    res = SF.run(_no_torch_sync(call), [i_in, r_in], stream=stream, state=state, table=t, reset=reset)
    _finish(res, A, case, want)
    assert np.array_equal(GN.bits64(res.out["ctl"]), GN.bits64(_ctl_bytes(block)))


def test_row_ids_made_on_one_stream_serve_another():
    """`BackwardPlan.row_ids()` computes the ids once, on the stream that is current, and keeps the tensor.  Here that happens
    on S1 behind the delay, and `rows(accumulate=)` consumes the kept ids on a second stream S2 with no synchronisation by the
    caller -- who never sees the tensor and so cannot order it.  A plan serves every stream
    (test_a_plan_made_on_a_side_stream_serves_the_default_stream): the merged gradient must be right.  Ids that are not yet
    written reach only scone_grad_merge_map, which is bounded for any list by contract."""
    max_n, d, batch = 4, BWD_D, "small"
    n = TB.N_ROWS[max_n]
    t = TB._table(max_n, d)
    off, _ = TB._lists(batch, max_n, "cover")
    g = TB._grad(len(off) - 1, d, "fp16").cuda()
    want_ids, want_rows = TB._want(batch, max_n, "cover", "mean", d, "fp16")
    rng = np.random.default_rng(23)
    old_ids = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.int64)
    old_rows = rng.standard_normal((len(old_ids), d)).astype(np.float32)
    m_ids, m_rows = GM.merge(old_ids, old_rows, want_ids, want_rows)
    old = (torch.from_numpy(old_ids).cuda(), torch.from_numpy(old_rows).cuda())
    s1 = SF.side_stream(t)
    s2 = SF.side_stream(t, beside=(s1,), tag="second")
    assert s1.cuda_stream != s2.cuda_stream
    warm, plan = TB._plan(t, batch, max_n), TB._plan(t, batch, max_n)
    torch.cuda.synchronize()

    def sequence(p, with_delay):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s1):
            e0.record(s1)
            if with_delay:
                SF.delay()
            e1.record(s1)
            p.row_ids()
        with torch.cuda.stream(s2):
            rid, rows = p.rows(g, "mean", accumulate=old)
            got = rid.clone(), rows.clone()
        s1.synchronize()
        s2.synchronize()
        return e0.elapsed_time(e1), got
    with torch.cuda.stream(s1):
        SF.warm_delay()
    sequence(warm, False)
    warm._row_ids.fill_(-1)                                       # what the next allocation of this size on S1 will hold
    torch.cuda.synchronize()
    warm.close()
    del warm
    t.status()
    delay_ms, (rid, rows) = sequence(plan, True)
    assert delay_ms >= SF.DELAY_MS / 5, f"the delay ran {delay_ms:.1f} ms: too short to keep the ids unwritten"
    assert np.array_equal(rid.cpu().numpy(), m_ids), "rows(accumulate=) on a second stream read row ids that S1 had not written yet"
    assert GM.same_bits(rows.cpu().numpy(), m_rows)
    assert t.status() == 0
    plan.close()
