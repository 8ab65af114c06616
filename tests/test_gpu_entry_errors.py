"""What the host side of the lookup and optimizer entry points refuses, and in which order: a characterisation.

Every case calls the C ABI directly and pins the exact return code and the exact `scone_last_error` text of one refusal branch
of `scone_embed`, `scone_embed_base`, `scone_embed_varlen`, `scone_embed_base_varlen`, `scone_embed_select`,
`scone_gather_reduce`, `scone_embed_partial`, `scone_finalize`, `scone_embed_prefetch`, `scone_opt_step`,
`scone_opt_step_lean` and the `_ctl`, `_dn` and `_dh` forms of those two; the texts are literals (callers and other tests match
on them).  Doubly-wrong calls pin which refusal wins, the zero-size calls pin which checks come before the early `SCONE_OK`
(they pass null pointers that must not be touched), and the shard embeds are covered as far as their "no planned batch" refusal (the rest needs an exchange: test_gpu_multiprocess,
test_distributed_gloo).

No call here reaches a kernel launch: a refused call returns before one, an early return has nothing to do.  Every non-null
pointer still names real device memory (`P`, 64 KiB of zeros, which must stay zeros), and `scone_status` must stay clear.

Left out on purpose: `scone_embed`'s "unknown out_dtype" below the one-launch road (it comes after the match kernel has run on
the batch) and the staged "sequence too long for one staging chunk" refusal (it comes after the staging pipeline is built).
"""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, MAX_N = 64, 3
TOO_MANY = 2 ** 31                      # a token count one above what the packed entry points take
MEAN, F32 = 0, 0                        # SCONE_REDUCE_MEAN, SCONE_DT_F32
BAD_REDUCE, BAD_DT = 7, 9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


class _World:
    """The tables of the issue, one device buffer to point at, and `refused` / `accepted`."""

    def __init__(self):
        from scone_amd import _lib
        from scone_amd.hip_backend import SconeTable
        self.L, self.lib = _lib, _lib.lib()
        self.i8 = SconeTable(MAX_N, ROWS, 64, "int8")
        self.i8_768 = SconeTable(MAX_N, ROWS, 768, "int8")                       # takes the one-launch road
        self.f20 = SconeTable(MAX_N, ROWS, 20, "fp32")                           # d % 8 != 0: the lane-group fallback
        self.f20_suffix = SconeTable(MAX_N, ROWS, 20, "fp32", lookup_mode="longest_suffix")
        self.staged = SconeTable(MAX_N, ROWS, 64, "int8", placement="pinned_host", hot_rows=16, stage_tokens=1024)
        self.staged20 = SconeTable(MAX_N, ROWS, 20, "fp32", placement="pinned_host", hot_rows=16, stage_tokens=1024)
        self.index_only = SconeTable(MAX_N, ROWS)                                # dim == 0
        self.tables = (self.i8, self.i8_768, self.f20, self.f20_suffix, self.staged, self.staged20, self.index_only)
        self.buf = torch.zeros(16384, dtype=torch.int32, device="cuda")
        self.P = self.buf.data_ptr()

    def call(self, name, table, *args):
        h = None if table is None else table._h
        return getattr(self.lib, name)(h, *args)

    def refused(self, name, table, args, code, text):
        rc = self.call(name, table, *args)
        got = self.lib.scone_last_error(table._h).decode()
        assert (rc, got) == (code, text), (name, args)

    def accepted(self, name, table, args):
        rc = self.call(name, table, *args)
        assert rc == self.L.OK, (name, args, rc, self.lib.scone_last_error(table._h).decode())

    def null_handle(self, name, args):
        assert self.call(name, None, *args) == self.L.EINVAL, name

    def untouched(self):
        torch.cuda.synchronize()
        assert not bool(self.buf.any()), "a refused call wrote"
        for t in self.tables[:-1]:
            assert t.status() == 0


@pytest.fixture(scope="module")
def w():
    world = _World()
    yield world
    world.untouched()


def _args(defaults, order, **kw):
    a = dict(defaults, **kw)
    assert set(a) == set(order), set(a) ^ set(order)
    return tuple(a[k] for k in order)


# ------------------------------------------------------------------ scone_embed, scone_embed_base
def _embed(w, **kw):
    return _args(dict(tok=w.P, B=2, T=4, wte=None, vocab=0, wpe=None, n_pos=0, pos=None, reduce=MEAN, out=w.P, dt=F32, stream=None),
                 ("tok", "B", "T", "wte", "vocab", "wpe", "n_pos", "pos", "reduce", "out", "dt", "stream"), **kw)


def test_scone_embed(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed", t, _embed(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed", _embed(w))
    no(w.index_only, "scone_embed: handle has no table (dim == 0)", S)
    no(w.i8, "scone_embed: negative B or T", B=-1)
    no(w.i8, "scone_embed: negative B or T", T=-1)
    no(w.i8, "scone_embed: null pointer", tok=None)
    no(w.i8, "scone_embed: null pointer", out=None)
    no(w.i8, "scone_embed: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "scone_embed: wte/wpe given without vocab/n_pos", wte=w.P)
    no(w.i8, "scone_embed: wte/wpe given without vocab/n_pos", wpe=w.P, n_pos=-1)
    no(w.f20_suffix, "scone_embed: lookup_mode longest_suffix needs d % 8 == 0")
    no(w.staged20, "scone_embed: staged prefetch needs d % 8 == 0")
    no(w.i8_768, "unknown out_dtype", dt=BAD_DT)                                  # the one-launch road: refused at the launch
    # which refusal wins
    no(w.index_only, "scone_embed: handle has no table (dim == 0)", S, B=-1)
    no(w.i8, "scone_embed: negative B or T", B=-1, tok=None)
    no(w.i8, "scone_embed: null pointer", tok=None, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed: bad reduce", reduce=BAD_REDUCE, wte=w.P)
    no(w.f20_suffix, "scone_embed: wte/wpe given without vocab/n_pos", wte=w.P)
    # B * T == 0 returns before the pointers, the reduce and the lookup mode are looked at
    for kw in (dict(B=0), dict(T=0)):
        w.accepted("scone_embed", w.i8, _embed(w, tok=None, out=None, reduce=BAD_REDUCE, wte=w.P, **kw))
        w.accepted("scone_embed", w.f20_suffix, _embed(w, tok=None, out=None, **kw))
    no(w.i8, "scone_embed: negative B or T", B=0, T=-1)


def _embed_base(w, **kw):
    return _args(dict(tok=w.P, B=2, T=4, base=w.P, wpe=None, n_pos=0, pos=None, reduce=MEAN, out=w.P, dt=F32, stream=None),
                 ("tok", "B", "T", "base", "wpe", "n_pos", "pos", "reduce", "out", "dt", "stream"), **kw)


def test_scone_embed_base(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed_base", t, _embed_base(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed_base", _embed_base(w))
    no(w.index_only, "scone_embed_base: handle has no table (dim == 0)", S)
    no(w.i8, "scone_embed_base: negative B or T", B=-1)
    no(w.i8, "scone_embed_base: negative B or T", T=-1)
    no(w.i8, "scone_embed_base: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_base: bad out_dtype", dt=BAD_DT)
    no(w.i8, "scone_embed_base: bad out_dtype", dt=-1)
    for kw in (dict(tok=None), dict(base=None), dict(out=None)):
        no(w.i8, "scone_embed_base: null pointer (d_tok, d_base and d_out are required)", **kw)
    no(w.i8, "scone_embed_base: wpe given without n_pos", wpe=w.P)
    overlap = "scone_embed_base: d_base overlaps d_out (only d_out == d_base, the in-place call, is defined)"
    no(w.i8, overlap, out=w.P + 4)                                                # 8 x 64 fp32 = 2048 bytes each
    no(w.i8, overlap, base=w.P + 2044)
    no(w.i8, overlap, base=w.P + 1020, dt=1)                                      # fp16: 1024 bytes each
    no(w.f20_suffix, "scone_embed: lookup_mode longest_suffix needs d % 8 == 0")  # the shared body reports as scone_embed
    no(w.staged20, "scone_embed: staged prefetch needs d % 8 == 0")
    # which refusal wins
    no(w.i8, "scone_embed_base: negative B or T", B=-1, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_base: bad reduce", reduce=BAD_REDUCE, dt=BAD_DT)
    no(w.i8, "scone_embed_base: bad out_dtype", dt=BAD_DT, tok=None)
    no(w.i8, "scone_embed_base: null pointer (d_tok, d_base and d_out are required)", out=None, wpe=w.P)
    no(w.i8, "scone_embed_base: wpe given without n_pos", wpe=w.P, out=w.P + 4)
    no(w.f20_suffix, overlap, out=w.P + 4)
    # B * T == 0: the reduce and the out_dtype are checked before the early return, the pointers after it
    no(w.i8, "scone_embed_base: bad reduce", B=0, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_base: bad out_dtype", T=0, dt=BAD_DT)
    for kw in (dict(B=0), dict(T=0)):
        w.accepted("scone_embed_base", w.i8, _embed_base(w, tok=None, base=None, out=None, wpe=w.P, **kw))
        w.accepted("scone_embed_base", w.f20_suffix, _embed_base(w, tok=None, base=None, out=None, **kw))


# ------------------------------------------------------------------ the packed forms
def _varlen(w, **kw):
    return _args(dict(tok=w.P, cu=w.P, n_seqs=2, total=8, wte=None, vocab=0, wpe=None, n_pos=0, pos=None, reduce=MEAN, out=w.P, dt=F32,
                      stream=None),
                 ("tok", "cu", "n_seqs", "total", "wte", "vocab", "wpe", "n_pos", "pos", "reduce", "out", "dt", "stream"), **kw)


def test_scone_embed_varlen(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed_varlen", t, _varlen(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed_varlen", _varlen(w))
    no(w.index_only, "scone_embed_varlen: handle has no table (dim == 0)", S)
    no(w.i8, "scone_embed_varlen: negative n_seqs or total_tokens", n_seqs=-1)
    no(w.i8, "scone_embed_varlen: negative n_seqs or total_tokens", total=-1)
    no(w.i8, "scone_embed_varlen: total_tokens above 2^31 - 1", total=TOO_MANY)
    no(w.i8, "scone_embed_varlen: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_varlen: bad out_dtype", dt=BAD_DT)
    no(w.f20, "scone_embed_varlen: needs d % 8 == 0 (the lane-group fallback reads another record form)")
    staged = "scone_embed_varlen: not for stage_tokens > 0 (the staging pipeline chunks whole rectangular sequences)"
    no(w.staged, staged)
    for kw in (dict(tok=None), dict(cu=None), dict(out=None)):
        no(w.i8, "scone_embed_varlen: null pointer", **kw)
    no(w.i8, "scone_embed_varlen: wte/wpe given without vocab/n_pos", wte=w.P)
    no(w.i8, "scone_embed_varlen: wte/wpe given without vocab/n_pos", wpe=w.P)
    # which refusal wins
    no(w.i8, "scone_embed_varlen: negative n_seqs or total_tokens", n_seqs=-1, total=TOO_MANY)
    no(w.i8, "scone_embed_varlen: total_tokens above 2^31 - 1", total=TOO_MANY, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_varlen: bad reduce", reduce=BAD_REDUCE, dt=BAD_DT)
    no(w.f20, "scone_embed_varlen: bad out_dtype", dt=BAD_DT)
    no(w.staged20, "scone_embed_varlen: needs d % 8 == 0 (the lane-group fallback reads another record form)")
    no(w.staged, staged, tok=None)
    no(w.i8, "scone_embed_varlen: null pointer", tok=None, wte=w.P)
    # an empty batch: everything but the pointers and wte / wpe is checked first
    no(w.i8, "scone_embed_varlen: bad reduce", total=0, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_varlen: bad out_dtype", n_seqs=0, dt=BAD_DT)
    no(w.f20, "scone_embed_varlen: needs d % 8 == 0 (the lane-group fallback reads another record form)", total=0)
    no(w.staged, staged, n_seqs=0)
    for kw in (dict(total=0), dict(n_seqs=0)):
        w.accepted("scone_embed_varlen", w.i8, _varlen(w, tok=None, cu=None, out=None, wte=w.P, **kw))


def _base_varlen(w, **kw):
    return _args(dict(tok=w.P, cu=w.P, n_seqs=2, total=8, base=w.P, wpe=None, n_pos=0, pos=None, reduce=MEAN, out=w.P, dt=F32,
                      stream=None),
                 ("tok", "cu", "n_seqs", "total", "base", "wpe", "n_pos", "pos", "reduce", "out", "dt", "stream"), **kw)


def test_scone_embed_base_varlen(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed_base_varlen", t, _base_varlen(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed_base_varlen", _base_varlen(w))
    no(w.index_only, "scone_embed_base_varlen: handle has no table (dim == 0)", S)
    no(w.i8, "scone_embed_base_varlen: negative n_seqs or total_tokens", n_seqs=-1)
    no(w.i8, "scone_embed_base_varlen: negative n_seqs or total_tokens", total=-1)
    no(w.i8, "scone_embed_base_varlen: total_tokens above 2^31 - 1", total=TOO_MANY)
    no(w.i8, "scone_embed_base_varlen: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_base_varlen: bad out_dtype", dt=BAD_DT)
    no(w.f20, "scone_embed_base_varlen: needs d % 8 == 0 (the lane-group fallback reads another record form)")
    staged = "scone_embed_base_varlen: not for stage_tokens > 0 (the staging pipeline chunks whole rectangular sequences)"
    no(w.staged, staged)
    null = "scone_embed_base_varlen: null pointer (d_tok, d_cu_seqlens, d_base and d_out are required)"
    for kw in (dict(tok=None), dict(cu=None), dict(base=None), dict(out=None)):
        no(w.i8, null, **kw)
    no(w.i8, "scone_embed_base_varlen: wpe given without n_pos", wpe=w.P)
    overlap = "scone_embed_base_varlen: d_base overlaps d_out (only d_out == d_base, the in-place call, is defined)"
    no(w.i8, overlap, out=w.P + 4)
    no(w.i8, overlap, base=w.P + 1020, dt=2)                                      # bf16: 8 x 64 x 2 = 1024 bytes each
    # which refusal wins
    no(w.i8, "scone_embed_base_varlen: negative n_seqs or total_tokens", total=-1, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_base_varlen: bad reduce", reduce=BAD_REDUCE, dt=BAD_DT)
    no(w.f20, "scone_embed_base_varlen: bad out_dtype", dt=BAD_DT)
    no(w.staged20, "scone_embed_base_varlen: needs d % 8 == 0 (the lane-group fallback reads another record form)")
    no(w.staged, staged, base=None)
    no(w.i8, null, base=None, wpe=w.P)
    no(w.i8, "scone_embed_base_varlen: wpe given without n_pos", wpe=w.P, out=w.P + 4)
    # an empty batch
    no(w.i8, "scone_embed_base_varlen: bad out_dtype", total=0, dt=BAD_DT)
    no(w.staged, staged, total=0)
    for kw in (dict(total=0), dict(n_seqs=0)):
        w.accepted("scone_embed_base_varlen", w.i8, _base_varlen(w, tok=None, cu=None, base=None, out=None, wpe=w.P, **kw))


# ------------------------------------------------------------------ scone_embed_select
def _select(w, **kw):
    return _args(dict(tok=w.P, total=8, T=4, cu=None, n_seqs=0, sel=w.P, n_sel=2, wte=None, vocab=0, base=None, wpe=None, n_pos=0,
                      pos=None, reduce=MEAN, out=w.P, dt=F32, stream=None),
                 ("tok", "total", "T", "cu", "n_seqs", "sel", "n_sel", "wte", "vocab", "base", "wpe", "n_pos", "pos", "reduce", "out",
                  "dt", "stream"), **kw)


def test_scone_embed_select(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed_select", t, _select(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed_select", _select(w))
    no(w.index_only, "scone_embed_select: handle has no table (dim == 0)", S)
    negative = "scone_embed_select: negative total_tokens, n_sel or n_seqs"
    no(w.i8, negative, total=-8)
    no(w.i8, negative, n_sel=-1)
    no(w.i8, negative, cu=w.P, n_seqs=-1)
    no(w.i8, "scone_embed_select: total_tokens above 2^31 - 1", total=TOO_MANY)
    no(w.i8, "scone_embed_select: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_select: bad out_dtype", dt=BAD_DT)
    no(w.f20, "scone_embed_select: needs d % 8 == 0")
    staged = ("scone_embed_select: not for stage_tokens > 0 (the staging pipeline prefetches whole batches; "
              "tables read in place from pinned host memory work)")
    no(w.staged, staged)
    rectangle = "scone_embed_select: a rectangle needs T > 0 and total_tokens % T == 0"
    no(w.i8, rectangle, T=0)
    no(w.i8, rectangle, T=-4)
    no(w.i8, rectangle, T=3)
    no(w.i8, "scone_embed_select: d_wte and d_base are exclusive", wte=w.P, vocab=4, base=w.P)
    no(w.i8, "scone_embed_select: wte/wpe given without vocab/n_pos", wte=w.P)
    no(w.i8, "scone_embed_select: wte/wpe given without vocab/n_pos", wpe=w.P)
    null = "scone_embed_select: null pointer (d_tok, d_sel and d_out are required)"
    for kw in (dict(tok=None), dict(sel=None), dict(out=None)):
        no(w.i8, null, **kw)
    no(w.i8, "scone_embed_select: too many selected positions for one launch", n_sel=2 ** 26)
    overlap = "scone_embed_select: d_base overlaps d_out (only d_out == d_base, the in-place call, is defined)"
    no(w.i8, overlap, base=w.P + 508)                                             # 2 x 64 fp32 = 512 bytes each
    # which refusal wins
    no(w.i8, negative, n_sel=-1, total=TOO_MANY)
    no(w.i8, "scone_embed_select: total_tokens above 2^31 - 1", total=TOO_MANY, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_select: bad reduce", reduce=BAD_REDUCE, dt=BAD_DT)
    no(w.f20, "scone_embed_select: bad out_dtype", dt=BAD_DT)
    no(w.staged20, "scone_embed_select: needs d % 8 == 0")
    no(w.staged, staged, T=3)
    no(w.i8, rectangle, T=3, wte=w.P, vocab=4, base=w.P)
    no(w.i8, "scone_embed_select: d_wte and d_base are exclusive", wte=w.P, base=w.P)
    no(w.i8, "scone_embed_select: wte/wpe given without vocab/n_pos", wpe=w.P, tok=None)
    no(w.i8, null, tok=None, n_sel=2 ** 26)
    no(w.i8, "scone_embed_select: too many selected positions for one launch", n_sel=2 ** 26, base=w.P + 4)
    # nothing selected, or an empty batch: every check above the pointers comes first
    no(w.i8, "scone_embed_select: bad reduce", n_sel=0, reduce=BAD_REDUCE)
    no(w.i8, "scone_embed_select: d_wte and d_base are exclusive", n_sel=0, wte=w.P, vocab=4, base=w.P)
    no(w.i8, "scone_embed_select: wte/wpe given without vocab/n_pos", total=0, wpe=w.P)
    for kw in (dict(n_sel=0), dict(total=0), dict(total=0, T=0), dict(cu=w.P, n_seqs=0, T=0)):
        w.accepted("scone_embed_select", w.i8, _select(w, tok=None, sel=None, out=None, **kw))


# ------------------------------------------------------------------ scone_gather_reduce, scone_embed_partial, scone_finalize
def _reduce(w, **kw):
    return _args(dict(off=w.P, ids=w.P, ntok=8, base=None, reduce=MEAN, out=w.P, dt=F32, stream=None),
                 ("off", "ids", "ntok", "base", "reduce", "out", "dt", "stream"), **kw)


def test_scone_gather_reduce(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_gather_reduce", t, _reduce(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_gather_reduce", _reduce(w))
    no(w.index_only, "scone_gather_reduce: handle has no table (dim == 0)", S)
    no(w.i8, "scone_gather_reduce: negative ntok", ntok=-1)
    no(w.i8, "scone_gather_reduce: null pointer", off=None)
    no(w.i8, "scone_gather_reduce: null pointer", out=None)
    no(w.i8, "scone_gather_reduce: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "unknown out_dtype", dt=BAD_DT)                                      # refused at the launch
    no(w.f20, "unknown out_dtype", dt=BAD_DT)
    no(w.i8, "scone_gather_reduce: negative ntok", ntok=-1, off=None)
    no(w.i8, "scone_gather_reduce: null pointer", out=None, reduce=BAD_REDUCE)
    no(w.i8, "scone_gather_reduce: bad reduce", reduce=BAD_REDUCE, dt=BAD_DT)
    w.accepted("scone_gather_reduce", w.i8, _reduce(w, ntok=0, off=None, out=None, reduce=BAD_REDUCE, dt=BAD_DT))


def _partial(w, **kw):
    return _args(dict(tok=w.P, B=2, T=4, partial=w.P, counts=w.P, stream=None), ("tok", "B", "T", "partial", "counts", "stream"), **kw)


def test_scone_embed_partial(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed_partial", t, _partial(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed_partial", _partial(w))
    no(w.index_only, "scone_embed_partial: handle has no table (dim == 0)", S)
    no(w.i8, "scone_embed_partial: negative B or T", B=-1)
    no(w.i8, "scone_embed_partial: negative B or T", T=-1)
    for kw in (dict(tok=None), dict(partial=None), dict(counts=None)):
        no(w.i8, "scone_embed_partial: null pointer", **kw)
    no(w.f20_suffix, "scone_embed_partial: lookup_mode longest_suffix needs d % 8 == 0")
    no(w.i8, "scone_embed_partial: negative B or T", B=-1, tok=None)
    no(w.f20_suffix, "scone_embed_partial: null pointer", counts=None)
    for kw in (dict(B=0), dict(T=0)):
        w.accepted("scone_embed_partial", w.f20_suffix, _partial(w, tok=None, partial=None, counts=None, **kw))


def _finalize(w, **kw):
    return _args(dict(sums=w.P, counts=w.P, tok=w.P, B=2, T=4, t0=0, t1=8, wte=None, vocab=0, wpe=None, n_pos=0, pos=None, reduce=MEAN,
                      out=w.P, dt=F32, stream=None),
                 ("sums", "counts", "tok", "B", "T", "t0", "t1", "wte", "vocab", "wpe", "n_pos", "pos", "reduce", "out", "dt",
                  "stream"), **kw)


def test_scone_finalize(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_finalize", t, _finalize(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_finalize", _finalize(w))
    no(w.index_only, "scone_finalize: handle has no table (dim == 0)", S)
    for kw in (dict(B=-1, t1=0), dict(B=-2, T=-4), dict(t0=-1), dict(t0=5, t1=4), dict(t1=9)):
        no(w.i8, "scone_finalize: bad token range", **kw)
    for kw in (dict(sums=None), dict(counts=None), dict(out=None), dict(tok=None, wte=w.P, vocab=4), dict(tok=None, wpe=w.P, n_pos=4)):
        no(w.i8, "scone_finalize: null pointer", **kw)
    no(w.i8, "scone_finalize: bad reduce", reduce=BAD_REDUCE)
    no(w.i8, "unknown out_dtype", dt=BAD_DT)                                      # refused at the launch
    no(w.i8, "scone_finalize: bad token range", t1=9, sums=None)
    no(w.i8, "scone_finalize: null pointer", out=None, reduce=BAD_REDUCE)
    no(w.i8, "scone_finalize: bad reduce", reduce=BAD_REDUCE, dt=BAD_DT)
    for kw in (dict(t0=3, t1=3), dict(B=0, t0=0, t1=0)):
        w.accepted("scone_finalize", w.i8, _finalize(w, sums=None, counts=None, out=None, reduce=BAD_REDUCE, **kw))


# ------------------------------------------------------------------ scone_embed_prefetch
def _prefetch(w, **kw):
    return _args(dict(tok=w.P, B=2, T=4, ready=0, stream=None), ("tok", "B", "T", "ready", "stream"), **kw)


def test_scone_embed_prefetch(w):
    E, S = w.L.EINVAL, w.L.ESTATE
    no = lambda t, text, code=E, **kw: w.refused("scone_embed_prefetch", t, _prefetch(w, **kw), code, text)  # noqa: E731
    w.null_handle("scone_embed_prefetch", _prefetch(w))
    no(w.index_only, "scone_embed_prefetch: handle has no table (dim == 0)", S)
    no(w.i8, "scone_embed_prefetch: negative B or T", B=-1)
    no(w.i8, "scone_embed_prefetch: negative B or T", T=-1)
    no(w.i8, "scone_embed_prefetch: null pointer", tok=None)
    no(w.staged, "scone_embed_prefetch: null pointer", tok=None)
    no(w.i8, "scone_embed_prefetch: negative B or T", B=-1, tok=None)
    w.accepted("scone_embed_prefetch", w.staged, _prefetch(w, B=0, tok=None))
    w.accepted("scone_embed_prefetch", w.staged, _prefetch(w, T=0, tok=None))
    w.accepted("scone_embed_prefetch", w.i8, _prefetch(w))                         # rows in HBM: nothing to prefetch
    w.accepted("scone_embed_prefetch", w.staged20, _prefetch(w))                   # d % 8 != 0: no pipeline, nothing to prefetch
    no(w.staged20, "scone_embed_prefetch: null pointer", tok=None)


# ------------------------------------------------------------------ the optimizer steps
def _opt_cfg(w, **kw):
    a = dict(struct_size=C.sizeof(w.L.OptCfg), kind=w.L.OPT_SGD, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
             grad_scale=1.0, step=1)
    a.update(kw)
    return w.L.OptCfg(**a)


def _opt(w, cfg=None, **kw):
    return _args(dict(cfg=_opt_cfg(w) if cfg is None else cfg, ids=w.P, grad=w.P, n=4, master=w.P, s1=None, s2=None, stream=None),
                 ("cfg", "ids", "grad", "n", "master", "s1", "s2", "stream"), **kw)


def test_scone_opt_step(w):
    E = w.L.EINVAL
    no = lambda t, text, code=E, **kw: w.refused("scone_opt_step", t, _opt(w, **kw), code, text)  # noqa: E731
    inf, nan = float("inf"), float("nan")
    w.null_handle("scone_opt_step", _opt(w))
    assert C.sizeof(w.L.OptCfg) == 64
    assert w.call("scone_opt_step", w.i8, None, w.P, w.P, 4, w.P, None, None, None) == E
    assert w.lib.scone_last_error(w.i8._h) == b"scone_opt_step: null cfg"
    no(w.i8, "scone_opt_step: cfg.struct_size does not match this library", cfg=_opt_cfg(w, struct_size=60))
    no(w.i8, "scone_opt_step: bad kind", cfg=_opt_cfg(w, kind=3))
    no(w.i8, "scone_opt_step: bad kind", cfg=_opt_cfg(w, kind=-1))
    finite = "scone_opt_step: lr, beta1, beta2, eps, weight_decay and grad_scale must be finite"
    for bad in (dict(lr=nan), dict(beta1=inf), dict(beta2=-inf), dict(eps=nan), dict(weight_decay=inf), dict(grad_scale=nan)):
        no(w.i8, finite, cfg=_opt_cfg(w, **bad))
    adam = dict(kind=w.L.OPT_ADAM)
    no(w.i8, "scone_opt_step: Adam needs step >= 1", cfg=_opt_cfg(w, step=0, **adam), s1=w.P, s2=w.P)
    no(w.index_only, "scone_opt_step: handle has no table (dim == 0)")          # EINVAL here, SCONE_ESTATE in the lookups
    for kw in (dict(ids=None), dict(grad=None), dict(master=None)):
        no(w.i8, "scone_opt_step: null pointer", **kw)
    no(w.i8, "scone_opt_step: Adam needs d_state1 (m)", cfg=_opt_cfg(w, **adam), s2=w.P)
    state2 = "scone_opt_step: Adam / Adagrad need d_state2 (v / the sum of squares)"
    no(w.i8, state2, cfg=_opt_cfg(w, **adam), s1=w.P)
    no(w.i8, state2, cfg=_opt_cfg(w, kind=w.L.OPT_ADAGRAD))
    # which refusal wins
    no(w.i8, "scone_opt_step: cfg.struct_size does not match this library", cfg=_opt_cfg(w, struct_size=0, kind=9, lr=nan))
    no(w.i8, "scone_opt_step: bad kind", cfg=_opt_cfg(w, kind=9, lr=nan))
    no(w.i8, finite, cfg=_opt_cfg(w, lr=nan, step=0, **adam))
    no(w.index_only, "scone_opt_step: bad kind", cfg=_opt_cfg(w, kind=9))
    no(w.index_only, "scone_opt_step: handle has no table (dim == 0)", ids=None)
    no(w.i8, "scone_opt_step: null pointer", cfg=_opt_cfg(w, **adam), ids=None)
    no(w.i8, "scone_opt_step: Adam needs d_state1 (m)", cfg=_opt_cfg(w, **adam))
    # n == 0: the cfg and the handle are checked first, the pointers never
    no(w.i8, "scone_opt_step: bad kind", cfg=_opt_cfg(w, kind=9), n=0)
    no(w.index_only, "scone_opt_step: handle has no table (dim == 0)", n=0)
    w.accepted("scone_opt_step", w.i8, _opt(w, cfg=_opt_cfg(w, **adam), n=0, ids=None, grad=None, master=None))


def _lean_cfg(w, **kw):
    a = dict(struct_size=C.sizeof(w.L.LeanCfg), kind=w.L.LEAN_SGD, rounding=w.L.ROUND_NEAREST, reserved=0, lr=0.1, eps=1e-10,
             weight_decay=0.0, grad_scale=1.0, seed=1, step=1)
    a.update(kw)
    return w.L.LeanCfg(**a)


def _lean(w, cfg=None, **kw):
    return _args(dict(cfg=_lean_cfg(w) if cfg is None else cfg, ids=w.P, grad=w.P, n=4, master=w.P, state=None, stream=None),
                 ("cfg", "ids", "grad", "n", "master", "state", "stream"), **kw)


def test_scone_opt_step_lean(w):
    E = w.L.EINVAL
    no = lambda t, text, code=E, **kw: w.refused("scone_opt_step_lean", t, _lean(w, **kw), code, text)  # noqa: E731
    inf, nan = float("inf"), float("nan")
    w.null_handle("scone_opt_step_lean", _lean(w))
    assert C.sizeof(w.L.LeanCfg) == 64
    assert w.call("scone_opt_step_lean", w.i8, None, w.P, w.P, 4, w.P, None, None) == E
    assert w.lib.scone_last_error(w.i8._h) == b"scone_opt_step_lean: null cfg"
    no(w.i8, "scone_opt_step_lean: cfg.struct_size does not match this library", cfg=_lean_cfg(w, struct_size=56))
    no(w.i8, "scone_opt_step_lean: bad kind", cfg=_lean_cfg(w, kind=2))
    no(w.i8, "scone_opt_step_lean: bad rounding", cfg=_lean_cfg(w, rounding=2))
    no(w.i8, "scone_opt_step_lean: cfg.reserved must be 0", cfg=_lean_cfg(w, reserved=1))
    finite = "scone_opt_step_lean: lr, eps, weight_decay and grad_scale must be finite"
    for bad in (dict(lr=inf), dict(eps=nan), dict(weight_decay=-inf), dict(grad_scale=nan)):
        no(w.i8, finite, cfg=_lean_cfg(w, **bad))
    no(w.index_only, "scone_opt_step_lean: handle has no table (dim == 0)")
    in_place = "scone_opt_step_lean: in place (d_master == NULL) needs an fp32 or bf16 table, this one is int8"
    no(w.i8, in_place, master=None)
    stochastic = dict(rounding=w.L.ROUND_STOCHASTIC)
    no(w.i8, "scone_opt_step_lean: stochastic rounding with a master: there is nothing to round", cfg=_lean_cfg(w, **stochastic))
    no(w.f20, "scone_opt_step_lean: stochastic rounding on an fp32 table: there is nothing to round", cfg=_lean_cfg(w, **stochastic),
       master=None)
    no(w.i8, "scone_opt_step_lean: null pointer", ids=None)
    no(w.i8, "scone_opt_step_lean: null pointer", grad=None)
    rowwise = dict(kind=w.L.LEAN_ROWWISE_ADAGRAD)
    no(w.i8, "scone_opt_step_lean: row-wise Adagrad needs d_row_state (one fp32 per owned row)", cfg=_lean_cfg(w, **rowwise))
    # which refusal wins
    no(w.i8, "scone_opt_step_lean: bad kind", cfg=_lean_cfg(w, kind=2, rounding=2, reserved=1, lr=nan))
    no(w.i8, "scone_opt_step_lean: bad rounding", cfg=_lean_cfg(w, rounding=2, reserved=1, lr=nan))
    no(w.i8, "scone_opt_step_lean: cfg.reserved must be 0", cfg=_lean_cfg(w, reserved=1, lr=nan))
    no(w.index_only, "scone_opt_step_lean: bad rounding", cfg=_lean_cfg(w, rounding=2))
    no(w.index_only, "scone_opt_step_lean: handle has no table (dim == 0)", master=None)
    no(w.i8, in_place, cfg=_lean_cfg(w, **stochastic), master=None)
    no(w.f20, "scone_opt_step_lean: stochastic rounding with a master: there is nothing to round", cfg=_lean_cfg(w, **stochastic))
    no(w.i8, "scone_opt_step_lean: null pointer", cfg=_lean_cfg(w, **rowwise), ids=None)
    # n == 0: the mode refusals come first, the pointers never
    no(w.i8, in_place, n=0, master=None)
    no(w.f20, "scone_opt_step_lean: stochastic rounding on an fp32 table: there is nothing to round", cfg=_lean_cfg(w, **stochastic),
       n=0, master=None)
    w.accepted("scone_opt_step_lean", w.i8, _lean(w, cfg=_lean_cfg(w, **rowwise), n=0, ids=None, grad=None))
    w.accepted("scone_opt_step_lean", w.f20, _lean(w, n=0, ids=None, grad=None, master=None))


# ------------------------------------------------------------------ the _ctl, _dn and _dh forms of the two steps
# `n` is n_cap where the count is on the device; the _dh forms take the kind (and the rounding) where the others take the cfg.
# `need`: the pointers a form adds that must not be null, in the order they are refused (d_ctl of a _dn / _dh call is optional)
OPT_FORMS = {
    "scone_opt_step_ctl": (("cfg", "ids", "grad", "n", "master", "s1", "s2", "ctl", "stream"), ("ctl",)),
    "scone_opt_step_dn": (("cfg", "ids", "grad", "dn", "n", "master", "s1", "s2", "ctl", "stream"), ("dn",)),
    "scone_opt_step_dh": (("kind", "ids", "grad", "dn", "n", "master", "s1", "s2", "hyper", "ctl", "stream"), ("dn", "hyper")),
}
LEAN_FORMS = {
    "scone_opt_step_lean_ctl": (("cfg", "ids", "grad", "n", "master", "state", "ctl", "stream"), ("ctl",)),
    "scone_opt_step_lean_dn": (("cfg", "ids", "grad", "dn", "n", "master", "state", "ctl", "stream"), ("dn",)),
    "scone_opt_step_lean_dh": (("kind", "rounding", "ids", "grad", "dn", "n", "master", "state", "hyper", "ctl", "stream"),
                               ("dn", "hyper")),
}
NULL_OF = {"ctl": "null d_ctl", "dn": "null d_n", "hyper": "null d_hyper"}


def _form(w, order, default_cfg, **kw):
    a = dict(cfg=default_cfg, kind=0, rounding=0, ids=w.P, grad=w.P, n=4, master=w.P, s1=None, s2=None, state=None, ctl=w.P, dn=w.P,
             hyper=w.P, stream=None)
    assert set(kw) <= set(order), set(kw) - set(order)
    a.update(kw)
    return tuple(a[k] for k in order)


@pytest.mark.parametrize("name", list(OPT_FORMS))
def test_scone_opt_step_forms(w, name):
    E = w.L.EINVAL
    order, need = OPT_FORMS[name]
    dh = name.endswith("_dh")
    no = lambda t, text, **kw: w.refused(name, t, _form(w, order, _opt_cfg(w), **kw), E, f"{name}: {text}")  # noqa: E731
    kind = lambda k: dict(kind=k) if dh else dict(cfg=_opt_cfg(w, kind=k))  # noqa: E731
    adam, adagrad, bad = kind(w.L.OPT_ADAM), kind(w.L.OPT_ADAGRAD), kind(9)
    w.null_handle(name, _form(w, order, _opt_cfg(w)))
    no(w.i8, "bad kind", **bad)
    no(w.i8, "bad kind", **kind(-1))
    if not dh:                                                                    # the cfg is scone_opt_step's, checked as there
        no(w.i8, "null cfg", cfg=None)
        no(w.i8, "cfg.struct_size does not match this library", cfg=_opt_cfg(w, struct_size=60))
        no(w.i8, "lr, beta1, beta2, eps, weight_decay and grad_scale must be finite", cfg=_opt_cfg(w, lr=float("nan")))
        no(w.i8, "Adam needs step >= 1", cfg=_opt_cfg(w, kind=w.L.OPT_ADAM, step=0), s1=w.P, s2=w.P)
    no(w.index_only, "handle has no table (dim == 0)")
    for p in need:
        no(w.i8, NULL_OF[p], **{p: None})
    for kw in (dict(ids=None), dict(grad=None), dict(master=None)):
        no(w.i8, "null pointer", **kw)
    no(w.i8, "Adam needs d_state1 (m)", s2=w.P, **adam)
    state2 = "Adam / Adagrad need d_state2 (v / the sum of squares)"
    no(w.i8, state2, s1=w.P, **adam)
    no(w.i8, state2, **adagrad)
    # which refusal wins: the cfg (the kind), the table, the form's own pointers in their order, the data pointers, the states
    no(w.index_only, "bad kind", **bad)
    no(w.index_only, "handle has no table (dim == 0)", **{need[0]: None})
    for p in need:
        no(w.i8, "bad kind", **bad, **{p: None})
        no(w.i8, NULL_OF[p], n=0, **{p: None})
        no(w.i8, NULL_OF[p], ids=None, **{p: None})
    if dh:
        no(w.i8, "null d_n", dn=None, hyper=None)
    no(w.i8, "null pointer", ids=None, **adam)
    no(w.i8, "Adam needs d_state1 (m)", **adam)
    # n == 0: the cfg, the handle and the form's own pointers are checked first, the data pointers never
    no(w.i8, "bad kind", n=0, **bad)
    no(w.index_only, "handle has no table (dim == 0)", n=0)
    w.accepted(name, w.i8, _form(w, order, _opt_cfg(w), n=0, ids=None, grad=None, master=None, **adam))
    if "ctl" not in need:                                                         # the block is optional beside a device count
        w.accepted(name, w.i8, _form(w, order, _opt_cfg(w), n=0, ids=None, grad=None, master=None, ctl=None))


@pytest.mark.parametrize("name", list(LEAN_FORMS))
def test_scone_opt_step_lean_forms(w, name):
    E = w.L.EINVAL
    order, need = LEAN_FORMS[name]
    dh = name.endswith("_dh")
    no = lambda t, text, **kw: w.refused(name, t, _form(w, order, _lean_cfg(w), **kw), E, f"{name}: {text}")  # noqa: E731
    cfg = lambda **c: c if dh else dict(cfg=_lean_cfg(w, **c))  # noqa: E731
    stochastic, rowwise = cfg(rounding=w.L.ROUND_STOCHASTIC), cfg(kind=w.L.LEAN_ROWWISE_ADAGRAD)
    w.null_handle(name, _form(w, order, _lean_cfg(w)))
    no(w.i8, "bad kind", **cfg(kind=2))
    no(w.i8, "bad rounding", **cfg(rounding=2))
    if not dh:                                                                    # the cfg is scone_opt_step_lean's, checked as there
        no(w.i8, "null cfg", cfg=None)
        no(w.i8, "cfg.struct_size does not match this library", cfg=_lean_cfg(w, struct_size=56))
        no(w.i8, "cfg.reserved must be 0", cfg=_lean_cfg(w, reserved=1))
        no(w.i8, "lr, eps, weight_decay and grad_scale must be finite", cfg=_lean_cfg(w, eps=float("nan")))
    no(w.index_only, "handle has no table (dim == 0)")
    for p in need:
        no(w.i8, NULL_OF[p], **{p: None})
    in_place = "in place (d_master == NULL) needs an fp32 or bf16 table, this one is int8"
    with_master = "stochastic rounding with a master: there is nothing to round"
    on_fp32 = "stochastic rounding on an fp32 table: there is nothing to round"
    no(w.i8, in_place, master=None)
    no(w.i8, with_master, **stochastic)
    no(w.f20, on_fp32, master=None, **stochastic)
    no(w.i8, "null pointer", ids=None)
    no(w.i8, "null pointer", grad=None)
    state = "row-wise Adagrad needs d_row_state (one fp32 per owned row)"
    no(w.i8, state, **rowwise)
    # which refusal wins: the cfg (kind, then rounding), the table, the form's own pointers in their order, the mode, the data
    # pointers, the state
    no(w.i8, "bad kind", **cfg(kind=2, rounding=2))
    no(w.index_only, "bad rounding", **cfg(rounding=2))
    no(w.index_only, "handle has no table (dim == 0)", master=None, **{need[0]: None})
    for p in need:
        no(w.i8, "bad rounding", **cfg(rounding=2), **{p: None})
        no(w.i8, NULL_OF[p], master=None, **{p: None})                            # before the in-place refusal
        no(w.i8, NULL_OF[p], **stochastic, **{p: None})
        no(w.i8, NULL_OF[p], n=0, **{p: None})
    if dh:
        no(w.i8, "null d_n", dn=None, hyper=None)
    no(w.i8, in_place, master=None, **stochastic)
    no(w.f20, with_master, **stochastic)
    no(w.i8, in_place, master=None, ids=None)
    no(w.i8, "null pointer", ids=None, **rowwise)
    # n == 0: the mode refusals come first, the data pointers never
    no(w.i8, in_place, n=0, master=None)
    no(w.f20, on_fp32, n=0, master=None, **stochastic)
    no(w.i8, "bad kind", n=0, **cfg(kind=2))
    w.accepted(name, w.i8, _form(w, order, _lean_cfg(w), n=0, ids=None, grad=None, **rowwise))
    w.accepted(name, w.f20, _form(w, order, _lean_cfg(w), n=0, ids=None, grad=None, master=None))
    if "ctl" not in need:                                                         # the block is optional beside a device count
        w.accepted(name, w.f20, _form(w, order, _lean_cfg(w), n=0, ids=None, grad=None, master=None, ctl=None))


# ------------------------------------------------------------------ the shard embeds without a planned batch
def test_shard_embeds_need_a_planned_batch(w):
    S = w.L.ESTATE
    P = w.P
    rng = ("scone_shard_gather_embed_range", (P, 2, 4, 0, 2, P, 0, None, 0, None, 0, None, MEAN, P, 0, F32, None))
    whole = ("scone_shard_gather_embed", (P, 2, 4, P, 0, None, 0, None, 0, None, MEAN, P, F32, None))
    u64 = (C.c_uint64 * 1)(0)
    cols = ("scone_shard_cols_embed", (P, 2, 4, 0, 2, P, 0, None, P, 0, u64, u64, u64, u64, 1, None, 0, None, 0, None, MEAN, P, 0, F32,
                                       None))
    add = ("scone_shard_gather_add_records", (P, 0, 0, 0, None))
    for (name, args), who in ((rng, "scone_shard_gather_embed"), (whole, "scone_shard_gather_add_records"),
                              (cols, "scone_shard_cols_embed"), (add, "scone_shard_gather_add_records")):
        w.null_handle(name, args)
        w.refused(name, w.index_only, args, S, f"{who}: handle has no table (dim == 0)")
        w.refused(name, w.i8, args, S, f"{who}: call scone_shard_gather_plan first")
        w.refused(name, w.f20, args, S, f"{who}: call scone_shard_gather_plan first")   # before the d % 8 refusal
