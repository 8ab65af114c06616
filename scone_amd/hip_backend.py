"""Thin object wrapper over the C ABI: one :class:`SconeTable` = one ``scone_handle``
(device f-gram index + table shard).  Tensors cross the boundary as raw pointers
(``tensor.data_ptr()``); all work is enqueued on torch's current HIP stream."""

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L

_FMT = {"fp32": L.FMT_F32, "float32": L.FMT_F32, "f32": L.FMT_F32,
        "fp16": L.FMT_F16, "float16": L.FMT_F16, "f16": L.FMT_F16,
        "int8": L.FMT_I8, "i8": L.FMT_I8, "int4": L.FMT_I4, "i4": L.FMT_I4,
        "bf16": L.FMT_BF16, "bfloat16": L.FMT_BF16, "mxfp4": L.FMT_MXFP4}
_PLACE = {"hbm": L.PLACE_HBM, "pinned_host": L.PLACE_PINNED_HOST}
_REDUCE = {"mean": L.REDUCE_MEAN, "sum": L.REDUCE_SUM}
_MODE = {"cover": L.MODE_COVER, "longest_suffix": L.MODE_LONGEST_SUFFIX}
_DT = {torch.float32: L.DT_F32, torch.float16: L.DT_F16, torch.bfloat16: L.DT_BF16}

I4_GROUP = 128
MX_BLOCK = 32   # MXFP4: one E8M0 scale byte per 32 elements


def format_code(fmt) -> int:
    if isinstance(fmt, int):
        return fmt
    try:
        return _FMT[str(fmt).lower()]
    except KeyError:
        raise ValueError(f"unknown table format {fmt!r} (fp32, fp16, int8, int4, bf16, mxfp4)") from None


def row_bytes(fmt: int, d: int) -> int:
    """Algorithmic bytes per table row."""
    return {L.FMT_F32: 4 * d, L.FMT_F16: 2 * d, L.FMT_I8: d + 2,
            L.FMT_I4: d // 2 + 2 * (d // I4_GROUP), L.FMT_BF16: 2 * d, L.FMT_MXFP4: d // 2 + d // MX_BLOCK}[fmt]


class SconeError(RuntimeError):
    pass


def _raise(code: int, msg: str):
    text = f"{msg} [{L.lib().scone_strerror(code).decode()}]"
    if code == L.EINVAL:
        raise ValueError(text)
    if code == L.ERANGE:
        raise IndexError(text)
    if code == L.ENOMEM:
        raise MemoryError(text)
    raise SconeError(text)


class SconeInvalidArgument(SconeError, ValueError):
    """``SCONE_EINVAL`` from a call whose refusals are part of its contract (``scone_embed_varlen``)."""


def check_cu_seqlens(cu_seqlens, total: int) -> np.ndarray:
    """Host-side validation of a packed batch's boundaries: ``cu_seqlens`` (list, numpy array or CPU tensor of ``n + 1``
    integers) must start at 0, never decrease (repeats = empty sequences) and end at ``total``.  Returns it as a contiguous
    int32 array; raises ``ValueError`` otherwise.  Runs without a GPU.  (A DEVICE tensor is never passed here: checking it would
    need a synchronisation, so its contents are the caller's contract -- the kernels stay memory-safe whatever it holds.)"""
    if isinstance(cu_seqlens, torch.Tensor):
        if cu_seqlens.is_cuda:
            raise TypeError("check_cu_seqlens validates host data; a device tensor is trusted as it is")
        cu_seqlens = cu_seqlens.numpy()
    cu = np.asarray(cu_seqlens)
    if cu.ndim != 1 or cu.size < 1:
        raise ValueError("cu_seqlens must be a 1-D array of n_seqs + 1 offsets")
    if cu.dtype.kind not in "iu":
        raise ValueError("cu_seqlens must hold integers")
    cu = cu.astype(np.int64)
    total = int(total)
    if total > 2**31 - 1:
        raise ValueError("a packed batch holds at most 2^31 - 1 tokens")
    if cu[0] != 0:
        raise ValueError(f"cu_seqlens must start at 0, not {int(cu[0])}")
    if (np.diff(cu) < 0).any():
        k = int(np.argmax(np.diff(cu) < 0))
        raise ValueError(f"cu_seqlens must not decrease: cu[{k}] = {int(cu[k])} > cu[{k + 1}] = {int(cu[k + 1])}")
    if cu[-1] != total:
        raise ValueError(f"cu_seqlens must end at the number of tokens ({total}), not {int(cu[-1])}")
    return np.ascontiguousarray(cu.astype(np.int32))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("scone_amd: the f-gram lookup path needs an MI355X (no HIP device visible); "
                           "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def fit_gpu(tokens: torch.Tensor, text_offsets: torch.Tensor, max_n: int, min_freq: int, max_f_grams: int,
            device: Optional[torch.device] = None):
    """``scone_fit``: f-gram vocabulary of a tokenised corpus, built on the GPU.
    Returns ``(keys [S, max_n] uint32, lens [S] uint8, counts [S] uint32, n_distinct)`` as numpy arrays;
    row r is f-gram id r (the reference's ``Counter.most_common`` order)."""
    dev = torch.device(device) if device is not None else require_gpu()
    require_gpu()
    dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    tok = tokens.to(device=dev, dtype=torch.int32).contiguous()
    off = text_offsets.to(device=dev, dtype=torch.int64).contiguous()
    n_tok, n_texts = tok.numel(), off.numel() - 1
    cap = int(min(max_f_grams, max(1, n_tok * max_n)))
    keys = torch.zeros((cap, max_n), dtype=torch.int32, device=dev)
    lens = torch.zeros(cap, dtype=torch.uint8, device=dev)
    counts = torch.zeros(cap, dtype=torch.int32, device=dev)
    n_out, n_distinct = C.c_uint64(0), C.c_uint64(0)
    with torch.cuda.device(dev):
        rc = L.lib().scone_fit(dev.index, _ptr(tok), n_tok, _ptr(off), n_texts, int(max_n), int(max(min_freq, 0)),
                               int(max_f_grams), _ptr(keys), _ptr(lens), _ptr(counts), cap, C.byref(n_out),
                               C.byref(n_distinct), _stream())
    if rc != L.OK:
        _raise(rc, "scone_fit failed (negative or too large token ids, or out of memory)")
    n = n_out.value
    return (keys[:n].cpu().numpy().view(np.uint32), lens[:n].cpu().numpy(), counts[:n].cpu().numpy().view(np.uint32),
            n_distinct.value)


def fit_occurrences(text_lengths, max_n: int) -> int:
    """n-gram occurrences of a run of texts of these lengths: ``sum_L sum_{n=1..min(max_n, L)} (L - n + 1)``, the number of
    insertions the reference's ``Counter.update(extract_all_n_grams(text))`` makes (n_gram_extractor.py:59-70).  The
    ``seq_base`` of a shard is this sum over all texts in front of it.  Runs without a GPU."""
    lens = np.asarray(text_lengths, dtype=np.int64).reshape(-1)
    total = 0
    for n in range(1, int(max_n) + 1):
        total += int(np.clip(lens - n + 1, 0, None).sum())
    return total


def fit_partition(keys, lens, max_n: int, n_parts: int) -> np.ndarray:
    """``scone_fit_partition``: the key-hash partition ``uint32 [n]`` of ``keys [n, max_n]`` / ``lens [n]`` -- which part of
    ``n_parts`` counts each key under ``FitState.update(..., part=, n_parts=)``.  Runs without a GPU.  ``ValueError`` for a
    bad ``max_n`` / ``n_parts`` / length, ``IndexError`` for a token the key packing cannot hold."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    l = np.ascontiguousarray(lens, dtype=np.uint8).reshape(-1)
    if k.shape != (l.shape[0], int(max_n)):
        raise ValueError("fit_partition: keys must be [n, max_n]")
    if not 0 <= int(n_parts) < 2**32:
        raise ValueError("fit_partition: n_parts must fit 32 unsigned bits")
    out = np.zeros(l.shape[0], dtype=np.uint32)
    rc = L.lib().scone_fit_partition(k.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), l.shape[0], int(max_n),
                                     int(n_parts), out.ctypes.data_as(C.c_void_p))
    if rc != L.OK:
        _raise(rc, "scone_fit_partition failed")
    return out


_SEQ_CONTINUE = 2**64 - 1  # scone_fit_update: seq_base = UINT64_MAX continues at next_seq


class FitState:
    """``scone_fit_state``: a device-resident n-gram counter that is fed in chunks of whole texts, grows with the distinct
    n-grams seen, and can be finalised any number of times, exported and merged (include/scone_hip.h, "vocabulary
    construction").  A context manager; ``close()`` frees the device memory.  Raises like :func:`fit_gpu`'s callers
    expect: ``ValueError`` for ``SCONE_ERANGE`` (a token out of range) and ``SCONE_EINVAL``, ``RuntimeError`` otherwise."""

    def __init__(self, max_n: int, device: Optional[torch.device] = None, initial_slots: int = 0) -> None:
        self._st = None
        lib = L.lib()
        dev = torch.device(device) if device is not None else require_gpu()
        require_gpu()
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.max_n = int(max_n)
        st = C.c_void_p()
        self._check(lib.scone_fit_create(self.device.index, self.max_n, int(initial_slots), C.byref(st)), "scone_fit_create")
        self._st = st

    @staticmethod
    def _check(rc: int, who: str) -> None:
        if rc == L.OK:
            return
        text = f"{who} failed [{L.lib().scone_strerror(rc).decode()}]"
        if rc == L.ERANGE:
            raise ValueError(text + ": negative or too large token ids, or an output buffer too small")
        if rc == L.EINVAL:
            raise SconeInvalidArgument(text)
        raise SconeError(text)

    def close(self) -> None:
        if self._st is not None:
            L.lib().scone_fit_destroy(self._st)
            self._st = None

    def __enter__(self) -> "FitState":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._st is None:
            raise SconeError("FitState is closed")
        return self._st

    def _dev(self, a, dtype: torch.dtype, what: str) -> torch.Tensor:
        t = torch.as_tensor(a)
        if t.dtype != dtype:
            if t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"FitState: {what} must hold integers")
            if dtype == torch.int32 and t.numel() and (int(t.min()) < 0 or int(t.max()) > 2**31 - 2):
                raise ValueError("FitState: token ids must be in [0, 2**31 - 2]")
        return t.to(device=self.device, dtype=dtype).contiguous()

    def update(self, tokens, text_offsets, seq_base: Optional[int] = None, part: Optional[int] = None,
               n_parts: Optional[int] = None) -> None:
        """Count one chunk of whole texts: ``tokens`` flat, ``text_offsets[n_texts + 1]`` from 0 to ``len(tokens)``.
        ``seq_base=None`` numbers the chunk's occurrences after the previous chunk's; an integer is the global number of
        its first occurrence (see :func:`fit_occurrences`).  A refused chunk (``ValueError``) changes nothing.  int32
        tokens go to the device unchecked (the kernel validates them); wider integers are range-checked here.
        ``part`` / ``n_parts`` (both or neither): count only the keys of that key-hash partition
        (``scone_fit_update_part``, :func:`fit_partition`); every occurrence is still numbered and adds to
        ``n_occurrences`` and ``next_seq``."""
        if (part is None) != (n_parts is None):
            raise ValueError("FitState.update: give both part and n_parts, or neither")
        if part is not None and not (0 <= int(part) < 2**32 and 0 <= int(n_parts) < 2**32):
            raise ValueError("FitState.update: part and n_parts must fit 32 unsigned bits")
        tok = self._dev(tokens, torch.int32, "tokens").reshape(-1)
        off = self._dev(text_offsets, torch.int64, "text_offsets").reshape(-1)
        n_texts = off.numel() - 1
        if n_texts < 0:
            raise ValueError("FitState.update: text_offsets must hold n_texts + 1 offsets")
        base = _SEQ_CONTINUE if seq_base is None else int(seq_base)
        if not 0 <= base <= _SEQ_CONTINUE:
            raise ValueError("FitState.update: seq_base must fit 64 unsigned bits")
        with torch.cuda.device(self.device):
            if part is None:
                rc = L.lib().scone_fit_update(self._handle(), _ptr(tok), tok.numel(), _ptr(off), n_texts, base, _stream())
            else:
                rc = L.lib().scone_fit_update_part(self._handle(), _ptr(tok), tok.numel(), _ptr(off), n_texts, base, int(part),
                                                   int(n_parts), _stream())
        self._check(rc, "scone_fit_update" if part is None else "scone_fit_update_part")

    def stats(self) -> dict:
        """``n_distinct``, ``n_occurrences`` (counted by ``update``), ``slots`` (x 32 B of device memory), ``n_grows``,
        ``next_seq``."""
        v = [C.c_uint64(0) for _ in range(5)]
        self._check(L.lib().scone_fit_stats(self._handle(), *[C.byref(x) for x in v]), "scone_fit_stats")
        return dict(zip(("n_distinct", "n_occurrences", "slots", "n_grows", "next_seq"), (x.value for x in v)))

    def finalize(self, min_freq: int, max_f_grams: int, out_cap: Optional[int] = None, with_first: bool = False):
        """The f-gram list of everything counted so far: ``(keys [S, max_n] uint32, lens [S] uint8, counts [S] uint64,
        n_distinct)`` as numpy arrays, row r = f-gram id r (``Counter.most_common`` order).  Does not consume the state.
        ``with_first=True`` (``scone_fit_finalize_seq``) appends ``first [S] uint64``, every row's first sequence number:
        ``(keys, lens, counts, n_distinct, first)``, whose arrays are what :meth:`merge` takes."""
        n_distinct = self.stats()["n_distinct"]
        cap = int(min(max(int(max_f_grams), 0), n_distinct))
        if out_cap is not None:
            cap = min(cap, int(out_cap))
        keys = torch.zeros((max(cap, 1), self.max_n), dtype=torch.int32, device=self.device)
        lens = torch.zeros(max(cap, 1), dtype=torch.uint8, device=self.device)
        counts = torch.zeros(max(cap, 1), dtype=torch.int64, device=self.device)
        n_out = C.c_uint64(0)
        min_freq = int(min(max(int(min_freq), 0), 2**32 - 1))
        max_f_grams = int(min(max(int(max_f_grams), 0), 2**64 - 1))
        with torch.cuda.device(self.device):
            if with_first:
                first = torch.zeros(max(cap, 1), dtype=torch.int64, device=self.device)
                rc = L.lib().scone_fit_finalize_seq(self._handle(), min_freq, max_f_grams, _ptr(keys), _ptr(lens), _ptr(counts),
                                                    _ptr(first), cap, C.byref(n_out), _stream())
            else:
                rc = L.lib().scone_fit_finalize(self._handle(), min_freq, max_f_grams, _ptr(keys), _ptr(lens), _ptr(counts),
                                                cap, C.byref(n_out), _stream())
        self._check(rc, "scone_fit_finalize_seq" if with_first else "scone_fit_finalize")
        n = n_out.value
        res = (keys[:n].cpu().numpy().view(np.uint32), lens[:n].cpu().numpy(), counts[:n].cpu().numpy().view(np.uint64),
               n_distinct)
        return res + (first[:n].cpu().numpy().view(np.uint64),) if with_first else res

    def export(self):
        """Every distinct entry, in no particular order: ``(keys [D, max_n] uint32, lens [D] uint8, counts [D] uint64,
        first [D] uint64)`` as numpy arrays -- what :meth:`merge` takes (shards, checkpoints)."""
        cap = self.stats()["n_distinct"]
        keys = torch.zeros((max(cap, 1), self.max_n), dtype=torch.int32, device=self.device)
        lens = torch.zeros(max(cap, 1), dtype=torch.uint8, device=self.device)
        counts = torch.zeros(max(cap, 1), dtype=torch.int64, device=self.device)
        first = torch.zeros(max(cap, 1), dtype=torch.int64, device=self.device)
        n_out = C.c_uint64(0)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_fit_export(self._handle(), _ptr(keys), _ptr(lens), _ptr(counts), _ptr(first), cap,
                                          C.byref(n_out), _stream())
        self._check(rc, "scone_fit_export")
        n = n_out.value
        return (keys[:n].cpu().numpy().view(np.uint32), lens[:n].cpu().numpy(), counts[:n].cpu().numpy().view(np.uint64),
                first[:n].cpu().numpy().view(np.uint64))

    def merge(self, keys, lens, counts, first) -> None:
        """Add exported entries: ``count += counts[i]``, ``first = min(first, first[i])``.  ``next_seq`` is not touched."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        n = int(np.asarray(lens).shape[0])
        if k.shape != (n, self.max_n):
            raise ValueError("FitState.merge: keys must be [n, max_n]")
        arrs = [torch.from_numpy(k.view(np.int32)),
                torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint8)),
                torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint64).view(np.int64)),
                torch.from_numpy(np.ascontiguousarray(first, dtype=np.uint64).view(np.int64))]
        if arrs[2].numel() != n or arrs[3].numel() != n:
            raise ValueError("FitState.merge: lens, counts and first must have one entry per key")
        d = [a.to(self.device).contiguous() for a in arrs]
        with torch.cuda.device(self.device):
            rc = L.lib().scone_fit_merge(self._handle(), _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), n, _stream())
        self._check(rc, "scone_fit_merge")


def backward_chunk() -> int:
    """``scone_backward_chunk``: the chunk length ``C`` of the backward's summation order (part of its contract).  Runs
    without a GPU."""
    return int(L.lib().scone_backward_chunk())


_OPT = {"sgd": L.OPT_SGD, "adagrad": L.OPT_ADAGRAD, "adam": L.OPT_ADAM}


def _opt_cfg(kind, lr, betas, eps, weight_decay, grad_scale, step) -> "L.OptCfg":
    if isinstance(kind, str):
        if kind.lower() not in _OPT:
            raise ValueError(f"unknown optimizer kind {kind!r} (sgd, adagrad, adam)")
        kind = _OPT[kind.lower()]
    return L.OptCfg(C.sizeof(L.OptCfg), int(kind), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                    float(grad_scale), int(step))


def opt_scalars(kind, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, step=1) -> dict:
    """``scone_opt_scalars_of``: the fp32 scalars ``scone_opt_step`` computes with (``alpha, b1, b2, c1, c2, eps, decay,
    gscale``, each an ``np.float32``), from hyper-parameters given in double.  Runs without a GPU; ``ValueError`` for what
    the library refuses (a bad kind, ``step < 1`` for Adam, a value that is not finite)."""
    out = L.OptScalars()
    rc = L.lib().scone_opt_scalars_of(C.byref(_opt_cfg(kind, lr, betas, eps, weight_decay, grad_scale, step)), C.byref(out))
    if rc != L.OK:
        _raise(rc, "scone_opt_scalars_of: bad kind, step < 1 for Adam, or a hyper-parameter that is not finite")
    return {name: np.float32(getattr(out, name)) for name, _ in L.OptScalars._fields_}


_LEAN = {"sgd": L.LEAN_SGD, "rowwise_adagrad": L.LEAN_ROWWISE_ADAGRAD}
_ROUND = {"nearest": L.ROUND_NEAREST, "stochastic": L.ROUND_STOCHASTIC}
APPLY_LEAN_MAX_DIM = 4096     # the widest row scone_backward_apply_lean fuses (a wave's gradient row lives in its share of LDS)


def _lean_cfg(kind, lr, eps, weight_decay, grad_scale, rounding, seed, step) -> "L.LeanCfg":
    if isinstance(kind, str):
        if kind.lower() not in _LEAN:
            raise ValueError(f"unknown lean optimizer kind {kind!r} (sgd, rowwise_adagrad)")
        kind = _LEAN[kind.lower()]
    if isinstance(rounding, str):
        if rounding.lower() not in _ROUND:
            raise ValueError(f"unknown rounding {rounding!r} (nearest, stochastic)")
        rounding = _ROUND[rounding.lower()]
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 unsigned bits")
    return L.LeanCfg(C.sizeof(L.LeanCfg), int(kind), int(rounding), 0, float(lr), float(eps), float(weight_decay), float(grad_scale),
                     int(seed), int(step))


def lean_scalars(kind, lr, eps=1e-10, weight_decay=0.0, grad_scale=1.0) -> dict:
    """``scone_lean_scalars_of``: the fp32 scalars ``scone_opt_step_lean`` computes with (``alpha = lr``, ``eps``, ``decay = lr *
    weight_decay``, ``gscale``; the other fields of ``scone_opt_scalars`` are 0), each an ``np.float32``.  Runs without a GPU;
    ``ValueError`` for what the library refuses."""
    out = L.OptScalars()
    rc = L.lib().scone_lean_scalars_of(C.byref(_lean_cfg(kind, lr, eps, weight_decay, grad_scale, "nearest", 0, 1)), C.byref(out))
    if rc != L.OK:
        _raise(rc, "scone_lean_scalars_of: bad kind or a hyper-parameter that is not finite")
    return {name: np.float32(getattr(out, name)) for name, _ in L.OptScalars._fields_}


def lean_rand16(seed: int, step: int, row_id: int, col: int) -> int:
    """``scone_lean_rand16``: the 16 random bits of stochastic rounding for element ``col`` of GLOBAL row ``row_id`` (the host
    copy of the device function).  Runs without a GPU."""
    return int(L.lib().scone_lean_rand16(int(seed), int(step), int(row_id), int(col)))


def opt_hyper_scalars(kind, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, step=1) -> dict:
    """``scone_opt_hyper_scalars_of``: the host copy of what ``scone_opt_hyper_advance`` derives on the device at ``t = step`` --
    :func:`opt_scalars` in every field but Adam's ``alpha``, which uses the header's integer power instead of libm's ``pow`` (at
    most one fp32 ulp apart).  Runs without a GPU; ``ValueError`` for what the library refuses."""
    out = L.OptScalars()
    rc = L.lib().scone_opt_hyper_scalars_of(C.byref(_opt_cfg(kind, lr, betas, eps, weight_decay, grad_scale, step)), C.byref(out))
    if rc != L.OK:
        _raise(rc, "scone_opt_hyper_scalars_of: bad kind, step < 1 for Adam, or a hyper-parameter that is not finite")
    return {name: np.float32(getattr(out, name)) for name, _ in L.OptScalars._fields_}


def _no_scalars_beside_hyper(who: str, given: dict) -> None:
    """``hyper=`` replaces the by-value scalars: giving both is a ``ValueError``."""
    both = [name for name, v in given.items() if v is not None]
    if both:
        raise ValueError(f"{who}: hyper= holds the hyper-parameters on the device; {', '.join(name + '=' for name in both)} beside it "
                         "would be ignored -- write the block instead (hyper.lr.fill_(...), hyper.grad_scale.copy_(...))")


# the by-value scalars of the two steps: (their defaults -- lr has none --, what a cfg that carries only the kind holds beside hyper=)
_OPT_SCALARS = (dict(lr=None, step=1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0),
                dict(lr=0.0, step=1, betas=(0.0, 0.0), eps=0.0, weight_decay=0.0, grad_scale=1.0))
_LEAN_SCALARS = (dict(lr=None, eps=1e-10, weight_decay=0.0, grad_scale=1.0, seed=0, step=1),
                 dict(lr=0.0, eps=0.0, weight_decay=0.0, grad_scale=1.0, seed=0, step=1))


def _step_scalars(who: str, scalars, given: dict, n=None, hyper=None) -> dict:
    """The by-value scalars of a step, ``None`` replaced by the default -- or, with ``hyper=`` (which needs ``n=`` and takes no
    scalar beside it), the placeholders of a cfg that is read for its kind only."""
    defaults, kind_only = scalars
    if hyper is not None:
        _no_scalars_beside_hyper(who, given)
        if n is None:
            raise ValueError(f"{who}: hyper= needs n= (a 1-element int64 device tensor that holds the row count)")
        return kind_only
    if given["lr"] is None:
        raise ValueError(f"{who}: lr is required (or hyper=)")
    return {name: defaults[name] if v is None else v for name, v in given.items()}


class OptHyper:
    """``scone_opt_hyper``: the 104 device bytes that hold an optimizer's hyper-parameters and its step count
    (include/scone_hip.h, "optimizer hyper-parameters on the device"); :meth:`SconeTable.opt_hyper` makes one.  ``lr``,
    ``beta1``, ``beta2``, ``eps``, ``weight_decay``, ``grad_scale`` (float64), ``step`` and ``seed`` (int64: the seed's 64 bits)
    are 0-dim tensors that VIEW the block: ``hyper.lr.copy_(device_scalar)`` or ``hyper.lr.fill_(x)`` between steps -- or between
    replays of a captured step -- is stream-ordered device work and changes what the next
    :meth:`SconeTable.opt_hyper_advance` derives.  ``applied`` and ``bad`` (int32 views) are what the last advance left.
    :meth:`read` synchronises."""

    _INPUTS = ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")

    def __init__(self, device: torch.device) -> None:
        self.buf = torch.zeros(C.sizeof(L.SconeOptHyper) // 8, dtype=torch.float64, device=device)   # 104 bytes, 8-byte aligned
        for name in self._INPUTS:
            setattr(self, name, self.buf[getattr(L.SconeOptHyper, name).offset // 8])
        as_int = self.buf.view(torch.int64)
        self.seed = as_int[L.SconeOptHyper.seed.offset // 8]
        self.step = as_int[L.SconeOptHyper.step.offset // 8]
        as_i32 = self.buf.view(torch.int32)
        self.applied = as_i32[L.SconeOptHyper.applied.offset // 4]
        self.bad = as_i32[L.SconeOptHyper.bad.offset // 4]

    def read(self) -> dict:
        """Every field on the host: the six doubles, ``seed``, ``step``, ``sc`` (a dict of eight ``np.float32``), ``applied``
        and ``bad``.  Synchronises."""
        rec = L.SconeOptHyper.from_buffer_copy(self.buf.cpu().numpy().tobytes())
        out = {name: float(getattr(rec, name)) for name in self._INPUTS}
        out.update(seed=int(rec.seed), step=int(rec.step), applied=int(rec.applied), bad=int(rec.bad),
                   sc={name: np.float32(getattr(rec.sc, name)) for name, _ in L.OptScalars._fields_})
        return out


class GradCtl:
    """``scone_grad_ctl``: the 24 device bytes :meth:`SconeTable.grad_ctl` fills and ``opt_step(..., ctl=)`` /
    ``opt_step_lean(..., ctl=)`` read (include/scone_hip.h, "gradient norm, clipping and skipped steps").  ``coef`` (fp32) and
    ``skip`` (int32: 0 or 1) are 0-dim views of the block on the device -- no synchronisation; ``coef`` is what the caller's dense
    gradients are multiplied by (``torch._foreach_mul_(dense_grads, ctl.coef)``).  :meth:`read` synchronises."""

    _DTYPE = np.dtype([("sqnorm", "<f8"), ("norm", "<f4"), ("coef", "<f4"), ("skip", "<u4"), ("reserved", "<u4")])

    def __init__(self, device: torch.device) -> None:
        self.buf = torch.empty(3, dtype=torch.float64, device=device)      # 24 bytes, 8-byte aligned; scone_grad_ctl_set writes all

    def _field(self, name: str, dtype: torch.dtype) -> torch.Tensor:
        at = getattr(L.SconeGradCtl, name).offset
        return self.buf.view(torch.uint8)[at:at + 4].view(dtype)[0]

    @property
    def coef(self) -> torch.Tensor:
        return self._field("coef", torch.float32)

    @property
    def skip(self) -> torch.Tensor:
        return self._field("skip", torch.int32)

    def read(self) -> dict:
        """The five fields on the host (``sqnorm`` float64, ``norm`` / ``coef`` float32, ``skip`` / ``reserved`` int).
        Synchronises."""
        rec = self.buf.cpu().numpy().view(self._DTYPE)[0]
        return {"sqnorm": np.float64(rec["sqnorm"]), "norm": np.float32(rec["norm"]), "coef": np.float32(rec["coef"]),
                "skip": int(rec["skip"]), "reserved": int(rec["reserved"])}


class GradMergeMap:
    """What ``scone_grad_merge_map`` returns for two id lists ``a`` and ``b`` (include/scone_hip.h, "gradient accumulation"):
    ``ids`` int64 ``[n_out]``, the ascending union; ``src_a`` / ``src_b`` int32 ``[n_out]``, the index in ``a`` / ``b`` of
    every output row, ``-1`` (the library's ``0xFFFFFFFF``) where the list does not have it; ``pos_a`` ``[n_a]`` / ``pos_b``
    ``[n_b]``, the output row of every input row; ``d_n_out``, the count on the device; ``n_out``, the count on the host
    (``None`` from an unsynchronised call, whose arrays keep their capacity ``n_a + n_b``).  Made by
    :meth:`SconeTable.grad_merge_map`."""

    __slots__ = ("ids", "src_a", "src_b", "pos_a", "pos_b", "d_n_out", "n_out")

    def __init__(self, ids, src_a, src_b, pos_a, pos_b, d_n_out, n_out) -> None:
        self.ids, self.src_a, self.src_b, self.pos_a, self.pos_b = ids, src_a, src_b, pos_a, pos_b
        self.d_n_out, self.n_out = d_n_out, n_out


class BackwardPlan:
    """``scone_bwd_plan``: the sorted reference stream of one batch on one :class:`SconeTable` (include/scone_hip.h,
    "backward").  ``n_rows`` distinct rows have at least one of the ``n_refs`` references.  :meth:`rows` may be called any
    number of times, with either ``reduce`` and any ``grad_out`` dtype; it is stream-ordered and allocates nothing but its
    outputs.  A context manager; ``close()`` frees the device memory.  Made by :meth:`SconeTable.backward_plan` /
    :meth:`SconeTable.backward_plan_csr`."""

    def __init__(self, table: "SconeTable", plan, ntok: int, n_rows: int, n_refs: int) -> None:
        self._table, self._p = table, plan
        self.ntok, self.n_rows, self.n_refs = int(ntok), int(n_rows), int(n_refs)
        self._row_ids = None                      # row_ids(), once asked for: a plan does not change
        self._row_ids_stream, self._row_ids_ready = None, None    # where they were computed, and the event recorded behind that

    def close(self) -> None:
        if self._p is not None:
            L.lib().scone_backward_plan_destroy(self._p)
            self._p = None

    def __enter__(self) -> "BackwardPlan":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _plan(self):
        if self._p is None:
            raise SconeError("BackwardPlan is closed")
        if self._table._h is None:
            raise SconeError("BackwardPlan: its table is closed")
        return self._p

    def row_ids(self) -> torch.Tensor:
        """``scone_backward_row_ids``: the plan's ``U`` row ids, int64 ascending -- :meth:`rows`'s first result without
        computing a row.  Computed once, on the stream that is current then, and kept: treat the tensor as read-only.  A call
        under another current stream -- `rows(accumulate=)` makes one -- has that stream wait for an event recorded behind the
        launch (no host synchronisation; nothing on the stream that computed them)."""
        plan, t = self._plan(), self._table
        stream = torch.cuda.current_stream(t.device)
        if self._row_ids is None:
            ids = torch.empty(self.n_rows, dtype=torch.int64, device=t.device)
            t._check(L.lib().scone_backward_row_ids(t._h, plan, _ptr(ids) if self.n_rows else None, self.n_rows, stream.cuda_stream),
                     "scone_backward_row_ids")
            self._row_ids = ids
            if self.n_rows:                       # a plan serves every stream: a later caller on another one waits for this
                self._row_ids_stream = stream.cuda_stream
                self._row_ids_ready = torch.cuda.Event()
                self._row_ids_ready.record(stream)
        elif self._row_ids_ready is not None and stream.cuda_stream != self._row_ids_stream:
            stream.wait_event(self._row_ids_ready)                # nothing on the stream that made them
            self._row_ids.record_stream(stream)
        return self._row_ids

    def _rows_accumulate(self, grad_out: torch.Tensor, reduce: str, old) -> Tuple[torch.Tensor, torch.Tensor]:
        plan, t = self._plan(), self._table
        old_ids, old_rows = t._sparse_operand("rows(accumulate=)", *old)
        m = t.grad_merge_map(old_ids, self.row_ids())
        out = torch.empty((m.n_out, t.dim), dtype=torch.float32, device=t.device)
        with torch.cuda.device(t.device):
            stream = torch.cuda.current_stream(t.device)
            rc = L.lib().scone_backward_rows_acc(t._h, plan, _ptr(grad_out) if self.n_rows else None, _DT[grad_out.dtype],
                                                 _REDUCE[reduce], _ptr(m.src_a), _ptr(m.src_b), _ptr(m.pos_b), m.n_out,
                                                 _ptr(old_rows) if old_rows.shape[0] else None, _ptr(out) if m.n_out else None,
                                                 stream.cuda_stream)
        t._check(rc, "scone_backward_rows_acc")
        for x in (grad_out, old_rows, m.src_a, m.src_b, m.pos_b):
            if x.numel():
                x.record_stream(stream)
        return m.ids, out

    def rows(self, grad_out: torch.Tensor, reduce: str = "mean",
             out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, *,
             accumulate: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``scone_backward_rows``: ``(row_ids [U] int64 ascending, grad_rows [U, d] fp32)``, the payload of a coalesced
        ``torch.sparse_coo_tensor``.  ``grad_out``: ``[ntok, d]`` (or ``[B, T, d]``) fp32 / fp16 / bf16 on the table's device.
        ``out = (row_ids, grad_rows)``: the caller's buffers of at least ``n_rows`` rows; views of their first ``U`` rows
        are returned.

        ``accumulate = (old_ids, old_rows)``, a sparse row gradient that is already there (int64 ascending and distinct, fp32
        ``[n, d]``, on the table's device): ``scone_backward_rows_acc`` (include/scone_hip.h, "gradient accumulation").  The
        merged ``(ids, rows)`` is returned -- the bits of :meth:`rows` followed by :meth:`SconeTable.grad_merge` ``(old, new)``
        -- and the fp32 ``[U, d]`` gradient of this plan is never stored.  One 8-byte synchronise for the size of the union;
        ``out`` is not taken on this road."""
        plan, t = self._plan(), self._table
        if grad_out.dtype not in _DT:
            raise ValueError(f"grad_out must be fp32, fp16 or bf16, not {grad_out.dtype}")
        if grad_out.numel() != self.ntok * t.dim or (grad_out.dim() and grad_out.shape[-1] != t.dim and grad_out.numel()):
            raise ValueError(f"grad_out must hold [{self.ntok}, {t.dim}] elements, got {tuple(grad_out.shape)}")
        if not (grad_out.is_cuda and grad_out.device == t.device and grad_out.is_contiguous()):
            grad_out = grad_out.to(device=t.device).contiguous()
        if accumulate is not None:
            if out is not None:
                raise ValueError("rows: out= and accumulate= do not go together (the size of the union is not known beforehand)")
            if reduce not in _REDUCE:
                raise ValueError(f"unknown reduce {reduce!r}")
            return self._rows_accumulate(grad_out, reduce, accumulate)
        if out is None:
            ids = torch.empty(self.n_rows, dtype=torch.int64, device=t.device)
            rows = torch.empty((self.n_rows, t.dim), dtype=torch.float32, device=t.device)
        else:
            ids, rows = out
            assert ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int64 and ids.dim() == 1
            assert rows.is_cuda and rows.is_contiguous() and rows.dtype == torch.float32 and rows.dim() == 2
            assert rows.shape[1] == t.dim          # (too few rows: IndexError from the library, nothing written)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        rc = L.lib().scone_backward_rows(t._h, plan, grad_out.data_ptr(), _DT[grad_out.dtype], _REDUCE[reduce], ids.data_ptr(),
                                         rows.data_ptr(), min(ids.numel(), rows.shape[0]), stream)
        t._check(rc, "scone_backward_rows")
        if self.n_rows:
            grad_out.record_stream(torch.cuda.current_stream(t.device))    # it may be a temporary of the caller
        return ids[:self.n_rows], rows[:self.n_rows]

    def apply_lean(self, grad_out: torch.Tensor, reduce: str = "mean", *, kind, lr: float,
                   row_state: Optional[torch.Tensor] = None, eps: float = 1e-10, weight_decay: float = 0.0,
                   grad_scale: float = 1.0, rounding="nearest", seed: int = 0, step: int = 1) -> int:
        """``scone_backward_apply_lean``: the backward applied IN PLACE (include/scone_hip.h, "backward applied in place").  The
        served fp32 / bf16 rows and ``row_state`` end with exactly the bits that :meth:`rows` followed by
        :meth:`SconeTable.opt_step_lean` (``master=None``) leaves, but the fp32 ``[U, d]`` gradient is never stored.  The
        arguments are those two calls'.  Stream-ordered, at most two kernel launches, no allocation.  A table wider than
        ``APPLY_LEAN_MAX_DIM`` takes the two calls (the library does not fuse it).  Returns ``n_rows``."""
        plan, t = self._plan(), self._table
        cfg = _lean_cfg(kind, rounding=rounding, **_step_scalars("apply_lean", _LEAN_SCALARS, dict(
            lr=lr, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, seed=seed, step=step)))
        if t.fmt not in (L.FMT_F32, L.FMT_BF16):
            raise ValueError(f"apply_lean: in place needs an fp32 or bf16 table, this one has format code {t.fmt}")
        if cfg.rounding == L.ROUND_STOCHASTIC and t.fmt != L.FMT_BF16:
            raise ValueError("apply_lean: stochastic rounding is for bf16 rows (on an fp32 table there is nothing to round)")
        t._state_operand("apply_lean", "row_state", row_state, (t.row_end - t.row_begin,), cfg.kind == L.LEAN_ROWWISE_ADAGRAD)
        if grad_out.dtype not in _DT:
            raise ValueError(f"grad_out must be fp32, fp16 or bf16, not {grad_out.dtype}")
        if grad_out.numel() != self.ntok * t.dim or (grad_out.dim() and grad_out.shape[-1] != t.dim and grad_out.numel()):
            raise ValueError(f"grad_out must hold [{self.ntok}, {t.dim}] elements, got {tuple(grad_out.shape)}")
        if reduce not in _REDUCE:
            raise ValueError(f"unknown reduce {reduce!r}")
        if t.dim > APPLY_LEAN_MAX_DIM:                           # the two-call road, the same bits
            ids, rows = self.rows(grad_out, reduce)
            t.opt_step_lean(ids, rows, kind=kind, lr=lr, row_state=row_state, eps=eps, weight_decay=weight_decay,
                            grad_scale=grad_scale, rounding=rounding, seed=seed, step=step)
            return self.n_rows
        if not (grad_out.is_cuda and grad_out.device == t.device and grad_out.is_contiguous()):
            grad_out = grad_out.to(device=t.device).contiguous()
        with torch.cuda.device(t.device):
            stream = torch.cuda.current_stream(t.device)
            rc = L.lib().scone_backward_apply_lean(t._h, plan, grad_out.data_ptr(), _DT[grad_out.dtype], _REDUCE[reduce],
                                                   C.byref(cfg), _ptr(row_state), stream.cuda_stream)
        t._check(rc, "scone_backward_apply_lean")
        if self.n_rows:
            grad_out.record_stream(stream)                       # it may be a temporary of the caller
        return self.n_rows

    def counts(self) -> torch.Tensor:
        """``scone_backward_counts``: ``K_p``, the full hit count of every position, int32 ``[ntok]``."""
        plan, t = self._plan(), self._table
        k = torch.empty(self.ntok, dtype=torch.int32, device=t.device)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        t._check(L.lib().scone_backward_counts(t._h, plan, k.data_ptr(), stream), "scone_backward_counts")
        return k


def _device_count(who: str, n, device: torch.device) -> torch.Tensor:
    """``n=`` of the ``_dn`` calls: ONE int64 on the table's device (what :meth:`BackwardContext.rows` returns third)."""
    if not (isinstance(n, torch.Tensor) and n.dtype == torch.int64 and n.numel() == 1 and n.device == device and n.is_contiguous()):
        raise ValueError(f"{who}: n must be a 1-element int64 tensor on {device} (BackwardContext.rows returns it)")
    return n


class BackwardContext:
    """``scone_bwd_ctx``: the backward without a host synchronisation (include/scone_hip.h, "backward and optimizer step without
    a host synchronisation").  Holds, allocated once, every buffer a plan of up to ``max_tokens`` positions can need;
    :meth:`plan` and :meth:`rows` neither synchronise nor allocate device memory of the library's, so a whole
    ``plan; rows; opt_step(n=)`` chain can be enqueued while the device is busy, and captured in a ``torch.cuda.graph``.  The
    counts of the current plan live on the device; :meth:`counts` is the synchronising read.  One plan at a time: a new
    :meth:`plan` overwrites the previous one (stream order protects work already enqueued on the same stream).  A context
    manager; ``close()`` frees the device memory.  Made by :meth:`SconeTable.backward_context`."""

    def __init__(self, table: "SconeTable", max_tokens: int) -> None:
        self._table, self._c = table, None
        self.max_tokens = int(max_tokens)
        if self.max_tokens < 0:
            raise ValueError("backward_context: max_tokens must be >= 0")
        ctx = C.c_void_p()
        with torch.cuda.device(table.device):
            rc = L.lib().scone_backward_ctx_create(table._h, self.max_tokens, C.byref(ctx))
        table._check(rc, "scone_backward_ctx_create")
        self._c = ctx
        self.ntok = 0                             # positions of the current plan (host-known)
        nbytes = C.c_uint64(0)
        table._check(L.lib().scone_backward_ctx_bytes(ctx, C.byref(nbytes)), "scone_backward_ctx_bytes")
        self.nbytes = int(nbytes.value)           # device memory held

    def close(self) -> None:
        if self._c is not None:
            L.lib().scone_backward_ctx_destroy(self._c)
            self._c = None

    def __enter__(self) -> "BackwardContext":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ctx(self):
        if self._c is None:
            raise SconeError("BackwardContext is closed")
        if self._table._h is None:
            raise SconeError("BackwardContext: its table is closed")
        return self._c

    def plan(self, tok: torch.Tensor, cu_seqlens=None) -> "BackwardContext":
        """``scone_backward_plan_dn`` / ``scone_backward_plan_varlen_dn``: plan the batch :meth:`SconeTable.embed`
        (``tok [B, T]``) or :meth:`SconeTable.embed_varlen` (``tok [total]`` with ``cu_seqlens``) looks up -- the plan
        :meth:`SconeTable.backward_plan` returns, left in the context.  No synchronisation when ``tok`` (and a device
        ``cu_seqlens``) are int32, contiguous and on the table's device already; under capture pass such tensors.
        ``IndexError``: more positions than ``max_tokens``."""
        ctx, t = self._ctx(), self._table
        if cu_seqlens is None:
            tok = t._tok(tok)
            B, T = tok.shape
            if B * T > self.max_tokens:
                raise IndexError(f"BackwardContext.plan: {B * T} positions, the context holds {self.max_tokens}")
            with torch.cuda.device(t.device):
                stream = torch.cuda.current_stream(t.device).cuda_stream
                rc = L.lib().scone_backward_plan_dn(t._h, ctx, _ptr(tok) if B * T else None, B, T, stream)
            t._check(rc, "scone_backward_plan_dn")
            self.ntok, self._keep = B * T, (tok,)
            return self
        if tok.dim() != 1:
            raise ValueError("a packed batch takes its token ids as a 1-D tensor [total]")
        tok = tok.to(device=t.device, dtype=torch.int32).contiguous()
        total = tok.shape[0]
        if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
            if not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                    and cu_seqlens.numel() >= 1):
                raise ValueError("a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
            cu = cu_seqlens
        else:
            cu = torch.from_numpy(check_cu_seqlens(cu_seqlens, total)).to(t.device)
        ntok = total if cu.numel() > 1 else 0
        if ntok > self.max_tokens:
            raise IndexError(f"BackwardContext.plan: {ntok} positions, the context holds {self.max_tokens}")
        with torch.cuda.device(t.device):
            stream = torch.cuda.current_stream(t.device).cuda_stream
            rc = L.lib().scone_backward_plan_varlen_dn(t._h, ctx, _ptr(tok) if total else None, _ptr(cu), cu.numel() - 1, total, stream)
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"scone_backward_plan_varlen_dn: {L.lib().scone_last_error(t._h).decode()} "
                                       f"[{L.lib().scone_strerror(rc).decode()}]")
        t._check(rc, "scone_backward_plan_varlen_dn")
        self.ntok, self._keep = ntok, (tok, cu)
        return self

    def rows_cap(self) -> int:
        """The most rows the current plan can have on the host's knowledge: ``min(ntok * candidates, owned rows)``."""
        t = self._table
        cand = 1 if t.lookup_mode == "longest_suffix" else t.max_n * (t.max_n + 1) // 2
        return min(self.ntok * cand, t.row_end - t.row_begin)

    def rows(self, grad_out: torch.Tensor, reduce: str = "mean", out=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``scone_backward_rows_dn``: ``(ids_buf, rows_buf, n)`` -- the first ``n`` entries of ``ids_buf`` (int64) and rows of
        ``rows_buf`` (fp32 ``[cap, d]``) are, bit for bit, what :meth:`BackwardPlan.rows` returns for the same batch; ``n`` is a
        1-element int64 tensor ON THE DEVICE (``U``), the ``n=`` of :meth:`SconeTable.opt_step`, :meth:`SconeTable.opt_step_lean`
        and :meth:`SconeTable.grad_sqnorm`.  ``out = (ids_buf, rows_buf)`` or ``(ids_buf, rows_buf, n)``: the caller's buffers
        (``None``: fresh ones of :meth:`rows_cap` rows).  Entries past ``n`` are not touched.  A plan of more rows than the
        buffers hold writes nothing, sets ``n = 0`` and raises status bit 4 (:meth:`SconeTable.status`).  No synchronisation."""
        ctx, t = self._ctx(), self._table
        if grad_out.dtype not in _DT:
            raise ValueError(f"grad_out must be fp32, fp16 or bf16, not {grad_out.dtype}")
        if grad_out.numel() != self.ntok * t.dim or (grad_out.dim() and grad_out.shape[-1] != t.dim and grad_out.numel()):
            raise ValueError(f"grad_out must hold [{self.ntok}, {t.dim}] elements, got {tuple(grad_out.shape)}")
        if reduce not in _REDUCE:
            raise ValueError(f"unknown reduce {reduce!r}")
        if not (grad_out.is_cuda and grad_out.device == t.device and grad_out.is_contiguous()):
            grad_out = grad_out.to(device=t.device).contiguous()
        n = None
        if out is None:
            cap = self.rows_cap()
            ids = torch.empty(cap, dtype=torch.int64, device=t.device)
            rows = torch.empty((cap, t.dim), dtype=torch.float32, device=t.device)
        else:
            ids, rows = out[0], out[1]
            n = out[2] if len(out) > 2 else None
            if not (ids.is_cuda and ids.device == t.device and ids.is_contiguous() and ids.dtype == torch.int64 and ids.dim() == 1):
                raise ValueError(f"BackwardContext.rows: out[0] must be a contiguous int64 [cap] tensor on {t.device}")
            if not (rows.is_cuda and rows.device == t.device and rows.is_contiguous() and rows.dtype == torch.float32
                    and rows.dim() == 2 and rows.shape[1] == t.dim):
                raise ValueError(f"BackwardContext.rows: out[1] must be a contiguous fp32 [cap, {t.dim}] tensor on {t.device}")
        n = torch.empty(1, dtype=torch.int64, device=t.device) if n is None else _device_count("BackwardContext.rows", n, t.device)
        cap = min(ids.numel(), rows.shape[0])
        with torch.cuda.device(t.device):
            stream = torch.cuda.current_stream(t.device).cuda_stream
            rc = L.lib().scone_backward_rows_dn(t._h, ctx, _ptr(grad_out) if grad_out.numel() else None, _DT[grad_out.dtype],
                                                _REDUCE[reduce], _ptr(ids) if cap else None, _ptr(rows) if cap else None, cap,
                                                _ptr(n), stream)
        t._check(rc, "scone_backward_rows_dn")
        return ids, rows, n

    def counts(self) -> Tuple[int, int]:
        """``scone_backward_ctx_counts``: ``(n_rows, n_refs)`` of the current plan.  SYNCHRONISES the current stream."""
        ctx, t = self._ctx(), self._table
        n_rows, n_refs = C.c_uint64(0), C.c_uint64(0)
        with torch.cuda.device(t.device):
            rc = L.lib().scone_backward_ctx_counts(ctx, C.byref(n_rows), C.byref(n_refs), torch.cuda.current_stream(t.device).cuda_stream)
        t._check(rc, "scone_backward_ctx_counts")
        return int(n_rows.value), int(n_refs.value)


class SconeTable:
    """Device-resident f-gram index (+ optional table shard)."""

    def __init__(self, max_n: int, n_rows: int, dim: int = 0, table_format="fp32", placement: str = "hbm",
                 device: Optional[torch.device] = None, row_begin: int = 0, row_end: Optional[int] = None,
                 index_capacity: int = 0, hot_rows: int = 0, lookup_mode: str = "cover",
                 stage_tokens: int = 0, cache_rows: int = 0) -> None:
        self._h = None
        lib = L.lib()
        dev = torch.device(device) if device is not None else require_gpu()
        if dev.type != "cuda":
            raise RuntimeError("scone_amd: SconeTable lives on a HIP device; got " + str(dev))
        require_gpu()
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.max_n, self.n_rows, self.dim = int(max_n), int(n_rows), int(dim)
        self.fmt = format_code(table_format)
        self.row_begin = int(row_begin)
        self.row_end = int(n_rows if row_end is None else row_end)
        self.lookup_mode = str(lookup_mode)
        cfg = L.SconeCfg(C.sizeof(L.SconeCfg), self.device.index, self.max_n, self.dim, self.fmt,
                         _PLACE[placement], self.n_rows, self.row_begin, self.row_end, int(index_capacity),
                         int(hot_rows), _MODE[lookup_mode], int(stage_tokens), int(cache_rows))
        h = C.c_void_p()
        rc = lib.scone_create(C.byref(cfg), C.byref(h))
        if rc != L.OK:
            _raise(rc, "scone_create: " + lib.scone_last_error(None).decode())
        self._h = h
        self._embed_fn = lib.scone_embed

    # -- plumbing ---------------------------------------------------------------
    def _check(self, rc: int, who: str) -> None:
        if rc != L.OK:
            _raise(rc, f"{who}: " + L.lib().scone_last_error(self._h).decode())

    def close(self) -> None:
        if self._h is not None:
            L.lib().scone_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def status(self) -> int:
        bits = C.c_uint32(0)
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_status(self._h, C.byref(bits), _stream()), "scone_status")
        return bits.value

    def stage_counters(self) -> dict:
        """The cache of cold rows of a pinned-host table with ``stage_tokens > 0``: ``cache_rows`` (slots), ``rows_copied``
        (host -> HBM since the cache was created: every miss crosses PCIe once), ``chunks``, ``chunk_tokens`` (synchronises)."""
        v = [C.c_uint64(0) for _ in range(4)]
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_stage_counters(self._h, *[C.byref(x) for x in v]), "scone_stage_counters")
        return dict(zip(("cache_rows", "rows_copied", "chunks", "chunk_tokens"), (x.value for x in v)))

    # -- index ------------------------------------------------------------------
    def index_build(self, keys: np.ndarray, lens: np.ndarray, id0: int = 0) -> None:
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.uint8)
        n = int(lens.shape[0])
        if n == 0:
            return
        if keys.shape != (n, self.max_n):
            raise ValueError(f"keys must be [{n}, {self.max_n}] uint32, got {keys.shape}")
        rc = L.lib().scone_index_build(self._h, keys.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
                                       n, int(id0))
        self._check(rc, "scone_index_build")

    def index_build_device(self, keys: torch.Tensor, lens: torch.Tensor, id0: int = 0) -> None:
        assert keys.is_cuda and lens.is_cuda and keys.is_contiguous() and lens.is_contiguous()
        assert keys.dtype in (torch.int32, torch.uint32) and lens.dtype == torch.uint8
        n = int(lens.shape[0])
        with torch.cuda.device(self.device):
            rc = L.lib().scone_index_build_device(self._h, _ptr(keys), _ptr(lens), n, int(id0), _stream())
        self._check(rc, "scone_index_build_device")

    def index_stats(self) -> Tuple[int, int, int]:
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(L.lib().scone_index_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "scone_index_stats")
        return a.value, b.value, c.value

    def index_blob_sizes(self) -> Tuple[int, int, int]:
        """Bytes of the three blobs of the built index: hash slots, unigram table, presence bitmap."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(L.lib().scone_index_blob_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)), "scone_index_blob_sizes")
        return a.value, b.value, c.value

    def index_export(self, out=None):
        """The built index as host arrays ``(slots uint8, uni int32, bloom uint8, n_keys, capacity)``.  ``out = (slots, uni,
        bloom)``: write into these arrays (e.g. sections of a memory-mapped file) instead of allocating."""
        a, b, c = (C.c_uint64(x) for x in self.index_blob_sizes())
        if out is None:
            slots = np.empty(a.value, dtype=np.uint8)
            uni = np.empty(b.value // 4, dtype=np.int32)
            bloom = np.empty(c.value, dtype=np.uint8)
        else:
            slots, uni, bloom = out
            assert (slots.nbytes, uni.nbytes, bloom.nbytes) == (a.value, b.value, c.value)
            assert all(x.flags["C_CONTIGUOUS"] and x.flags["WRITEABLE"] for x in out)
        n = C.c_uint64(0)
        rc = L.lib().scone_index_export(self._h, slots.ctypes.data_as(C.c_void_p), uni.ctypes.data_as(C.c_void_p),
                                        bloom.ctypes.data_as(C.c_void_p), C.byref(n))
        self._check(rc, "scone_index_export")
        return slots, uni, bloom, n.value, a.value // 16

    def index_import(self, slots: np.ndarray, uni: np.ndarray, bloom: np.ndarray, n_keys: int) -> None:
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(L.lib().scone_index_blob_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)), "scone_index_blob_sizes")
        slots, uni, bloom = (np.ascontiguousarray(x) for x in (slots, uni, bloom))
        if (slots.nbytes, uni.nbytes, bloom.nbytes) != (a.value, b.value, c.value):
            raise ValueError("index blobs do not fit this handle (create it with the same max_n and index_capacity)")
        rc = L.lib().scone_index_import(self._h, slots.ctypes.data_as(C.c_void_p), uni.ctypes.data_as(C.c_void_p),
                                        bloom.ctypes.data_as(C.c_void_p), int(n_keys))
        self._check(rc, "scone_index_import")

    # -- table ------------------------------------------------------------------
    def upload(self, rows, scales=None, row0: int = 0) -> None:
        """Raw rows already in the table format (numpy host arrays or device tensors).  MXFP4: payload bytes ``[n, d/2]`` and
        E8M0 scale bytes ``[n, d/32]`` in logical block order; ``torch.float4_e2m1fn_x2`` / ``torch.float8_e8m0fnu`` tensors
        (an existing MX checkpoint) are taken as their bytes."""
        if self.fmt == L.FMT_MXFP4:
            rows, scales = (x.view(torch.uint8) if isinstance(x, torch.Tensor) and x.dtype != torch.uint8 and x.element_size() == 1
                            else x for x in (rows, scales))
            for x, width in ((rows, self.payload_bytes()), (scales, self.scales_per_row())):
                if x is None or tuple(x.shape[1:]) != (width,) or str(x.dtype).rsplit(".", 1)[-1] != "uint8":
                    raise ValueError(f"mxfp4 upload takes uint8 rows [n, {self.payload_bytes()}] and uint8 scales [n, {self.scales_per_row()}]")
            if isinstance(rows, torch.Tensor) and not rows.is_cuda:
                rows, scales = rows.numpy(), (scales.numpy() if isinstance(scales, torch.Tensor) else scales)
        is_dev = isinstance(rows, torch.Tensor)
        if is_dev:
            assert rows.is_cuda and rows.is_contiguous()
            nrows, rp = rows.shape[0], _ptr(rows)
            sp = _ptr(scales) if scales is not None else None
        else:
            rows = np.ascontiguousarray(rows)
            nrows, rp = rows.shape[0], rows.ctypes.data_as(C.c_void_p)
            if scales is not None:
                scales = np.ascontiguousarray(scales, dtype=self.scales_dtype())
            sp = scales.ctypes.data_as(C.c_void_p) if scales is not None else None
        with torch.cuda.device(self.device):
            rc = L.lib().scone_table_upload(self._h, rp, sp, int(row0), int(nrows), int(is_dev), _stream())
        self._check(rc, "scone_table_upload")

    def payload_bytes(self) -> int:
        return {L.FMT_F32: 4 * self.dim, L.FMT_F16: 2 * self.dim, L.FMT_I8: self.dim, L.FMT_I4: self.dim // 2,
                L.FMT_BF16: 2 * self.dim, L.FMT_MXFP4: self.dim // 2}[self.fmt]

    def scales_per_row(self) -> int:
        return {L.FMT_F32: 0, L.FMT_F16: 0, L.FMT_I8: 1, L.FMT_I4: self.dim // I4_GROUP, L.FMT_BF16: 0,
                L.FMT_MXFP4: self.dim // MX_BLOCK}[self.fmt]

    def scales_dtype(self):
        """numpy dtype of a scale: fp16 (INT8 / INT4), one E8M0 byte (MXFP4)."""
        return np.dtype(np.uint8) if self.fmt == L.FMT_MXFP4 else np.dtype(np.float16)

    def download(self, row0: int, nrows: int, rows: Optional[np.ndarray] = None,
                 scales: Optional[np.ndarray] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Raw payload rows ``uint8 [nrows, payload_bytes]`` and scales (fp16; MXFP4: E8M0 bytes, logical order) of global rows ``row0 ..`` -- into ``rows`` /
        ``scales`` when given (contiguous host arrays of those shapes, e.g. slices of a memory-mapped file)."""
        spr = self.scales_per_row()
        if rows is None:
            rows = np.empty((nrows, self.payload_bytes()), dtype=np.uint8)
        if scales is None and spr:
            scales = np.empty((nrows, spr), dtype=self.scales_dtype())
        assert rows.shape == (nrows, self.payload_bytes()) and rows.dtype == np.uint8 and rows.flags["C_CONTIGUOUS"]
        assert not spr or (scales.shape == (nrows, spr) and scales.dtype == self.scales_dtype() and scales.flags["C_CONTIGUOUS"])
        if not spr:
            scales = None
        with torch.cuda.device(self.device):
            rc = L.lib().scone_table_download(self._h, rows.ctypes.data_as(C.c_void_p),
                                              scales.ctypes.data_as(C.c_void_p) if spr else None, int(row0), int(nrows),
                                              0, _stream())
        self._check(rc, "scone_table_download")
        return rows, scales

    def store_f32(self, rows: torch.Tensor, row0: int = 0, ids: Optional[torch.Tensor] = None) -> None:
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {tuple(rows.shape)}")
        with torch.cuda.device(self.device):
            if ids is None:
                rc = L.lib().scone_table_store_f32(self._h, _ptr(rows), int(row0), rows.shape[0], _stream())
            else:
                ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
                rc = L.lib().scone_table_store_f32_ids(self._h, _ptr(rows), _ptr(ids), rows.shape[0], _stream())
            # `rows`/`ids` may be temporaries: keep them alive until the kernel has read them
            torch.cuda.current_stream().synchronize()
        self._check(rc, "scone_table_store_f32")

    def fill_synthetic(self, seed: int, base_scale: float) -> None:
        with torch.cuda.device(self.device):
            rc = L.lib().scone_table_fill_synthetic(self._h, int(seed) & 0xFFFFFFFF, float(base_scale), _stream())
        self._check(rc, "scone_table_fill_synthetic")

    def gather_rows(self, ids: torch.Tensor) -> torch.Tensor:
        ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty((ids.numel(), self.dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_table_gather_rows(self._h, _ptr(ids), ids.numel(), _ptr(out), _stream())
        self._check(rc, "scone_table_gather_rows")
        return out

    # -- hot path ---------------------------------------------------------------
    def _tok(self, tok: torch.Tensor) -> torch.Tensor:
        if tok.dim() == 1:
            tok = tok.unsqueeze(0)
        if tok.dim() != 2:
            raise ValueError("token ids must be [T] or [B, T]")
        return tok.to(device=self.device, dtype=torch.int32).contiguous()

    def match(self, tok: torch.Tensor) -> torch.Tensor:
        """hits[max_n, B, T] int32: id of the window tok[b, i:i+n] or -1."""
        tok = self._tok(tok)
        B, T = tok.shape
        hits = torch.empty((self.max_n, B, T), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_match(self._h, _ptr(tok), B, T, _ptr(hits), _stream())
        self._check(rc, "scone_match")
        return hits

    def match_csr(self, tok: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-position id lists (reference order, duplicates kept) as CSR (offsets[B*T+1], ids)."""
        tok = self._tok(tok)
        B, T = tok.shape
        ncand = self.max_n * (self.max_n + 1) // 2
        offsets = torch.empty(B * T + 1, dtype=torch.int32, device=self.device)
        ids = torch.empty(max(B * T * ncand, 1), dtype=torch.int32, device=self.device)
        total = C.c_int64(0)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_match_csr(self._h, _ptr(tok), B, T, _ptr(offsets), _ptr(ids), ids.numel(),
                                         C.byref(total), _stream())
        self._check(rc, "scone_match_csr")
        return offsets, ids[:total.value]

    def gather_reduce(self, offsets: torch.Tensor, ids: torch.Tensor, reduce: str = "mean",
                      base: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        offsets = offsets.to(device=self.device, dtype=torch.int32).contiguous()
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        ntok = offsets.numel() - 1
        out = torch.empty((ntok, self.dim), dtype=out_dtype, device=self.device)
        if base is not None:
            base = base.to(device=self.device, dtype=out_dtype).contiguous()
            assert base.shape == out.shape
        with torch.cuda.device(self.device):
            rc = L.lib().scone_gather_reduce(self._h, _ptr(offsets), _ptr(ids), ntok, _ptr(base), _REDUCE[reduce],
                                             _ptr(out), _DT[out_dtype], _stream())
        self._check(rc, "scone_gather_reduce")
        return out

    def embed(self, tok: torch.Tensor, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
              position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
              out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Fused match + gather + dequantise + reduce (+ wte[tok] + wpe[pos]) -> [B, T, d]."""
        if not (tok.dim() == 2 and tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
            tok = self._tok(tok)          # decode-size calls are host-bound: skip conversions that are no-ops
        B, T = tok.shape
        if out_dtype is None:
            out_dtype = wte.dtype if wte is not None else (wpe.dtype if wpe is not None else torch.float32)
        for name, w in (("wte", wte), ("wpe", wpe)):
            if w is not None:
                if not (w.is_cuda and w.is_contiguous() and w.dtype == out_dtype and w.dim() == 2
                        and w.shape[1] == self.dim):
                    raise ValueError(f"{name} must be a contiguous [*, {self.dim}] {out_dtype} tensor on {self.device}")
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).expand(B, T).contiguous()
        if out is None:
            out = torch.empty((B, T, self.dim), dtype=out_dtype, device=self.device)
        else:
            assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and out.numel() == B * T * self.dim
        # the library selects its device itself (hipSetDevice); torch's current stream of THAT device is the launch stream
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._embed_fn(self._h, tok.data_ptr(), B, T, None if wte is None else wte.data_ptr(),
                            0 if wte is None else wte.shape[0], None if wpe is None else wpe.data_ptr(),
                            0 if wpe is None else wpe.shape[0], None if position_ids is None else position_ids.data_ptr(),
                            _REDUCE[reduce], out.data_ptr(), _DT[out_dtype], stream)
        if rc != L.OK:
            self._check(rc, "scone_embed")
        return out

    def embed_varlen(self, tok: torch.Tensor, cu_seqlens, wte: Optional[torch.Tensor] = None,
                     wpe: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
                     out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_embed_varlen``: the fused lookup of a PACKED batch -> ``[total, d]``.  ``tok [total]`` holds the sequences back
        to back, sequence ``s`` is ``tok[cu_seqlens[s]:cu_seqlens[s + 1]]``; every token gets what :meth:`embed` gives it when
        its sequence is passed alone (no window crosses a boundary; the default position is the place inside the sequence).
        ``cu_seqlens`` on the host (list / numpy / CPU tensor) is validated (:func:`check_cu_seqlens`, ``ValueError``); an
        int32 device tensor is trusted -- no synchronisation either way."""
        if tok.dim() != 1:
            raise ValueError("embed_varlen takes the packed token ids as a 1-D tensor [total]")
        if not (tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
            tok = tok.to(device=self.device, dtype=torch.int32).contiguous()
        total = tok.shape[0]
        if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
            if not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                    and cu_seqlens.numel() >= 1):
                raise ValueError("a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
            cu = cu_seqlens
        else:
            cu = torch.from_numpy(check_cu_seqlens(cu_seqlens, total)).to(self.device)
        n_seqs = cu.numel() - 1
        if out_dtype is None:
            out_dtype = wte.dtype if wte is not None else (wpe.dtype if wpe is not None else torch.float32)
        for name, w in (("wte", wte), ("wpe", wpe)):
            if w is not None:
                if not (w.is_cuda and w.is_contiguous() and w.dtype == out_dtype and w.dim() == 2
                        and w.shape[1] == self.dim):
                    raise ValueError(f"{name} must be a contiguous [*, {self.dim}] {out_dtype} tensor on {self.device}")
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if position_ids.numel() != total:
                raise ValueError(f"position_ids must hold one position per packed token ({total})")
        if out is None:
            out = torch.empty((total, self.dim), dtype=out_dtype, device=self.device)
        else:
            assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and out.numel() == total * self.dim
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = L.lib().scone_embed_varlen(self._h, tok.data_ptr(), cu.data_ptr(), n_seqs, total,
                                        None if wte is None else wte.data_ptr(), 0 if wte is None else wte.shape[0],
                                        None if wpe is None else wpe.data_ptr(), 0 if wpe is None else wpe.shape[0],
                                        None if position_ids is None else position_ids.data_ptr(), _REDUCE[reduce],
                                        out.data_ptr(), _DT[out_dtype], stream)
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"scone_embed_varlen: {L.lib().scone_last_error(self._h).decode()} "
                                       f"[{L.lib().scone_strerror(rc).decode()}]")
        if rc != L.OK:
            self._check(rc, "scone_embed_varlen")
        return out

    def _base_args(self, who: str, ntok: int, base: torch.Tensor, wpe: Optional[torch.Tensor],
                   out_dtype: Optional[torch.dtype], out: Optional[torch.Tensor], shape) -> Tuple[torch.dtype, torch.Tensor]:
        """Validation shared by :meth:`embed_base` and :meth:`embed_base_varlen`: ``(out_dtype, out)``."""
        if not isinstance(base, torch.Tensor):
            raise ValueError(f"{who}: base must be a tensor")
        if out_dtype is None:
            out_dtype = base.dtype
        if out_dtype not in _DT:
            raise ValueError(f"{who}: out_dtype must be float32, float16 or bfloat16")
        if not (base.is_cuda and base.is_contiguous() and base.dtype == out_dtype and base.dim() >= 2
                and base.shape[-1] == self.dim and base.numel() == ntok * self.dim):
            raise ValueError(f"{who}: base must be a contiguous {out_dtype} tensor of {ntok} rows of {self.dim} on {self.device}")
        if wpe is not None and not (wpe.is_cuda and wpe.is_contiguous() and wpe.dtype == out_dtype and wpe.dim() == 2
                                    and wpe.shape[1] == self.dim):
            raise ValueError(f"wpe must be a contiguous [*, {self.dim}] {out_dtype} tensor on {self.device}")
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=self.device)
        else:
            assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and out.numel() == ntok * self.dim
        return out_dtype, out

    def embed_base(self, tok: torch.Tensor, base: torch.Tensor, *, wpe: Optional[torch.Tensor] = None,
                   position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
                   out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_embed_base``: :meth:`embed` onto a DENSE base -> ``[B, T, d]``,
        ``out[b, t] = (base[b, t] + reduce_k row_k) + wpe[pos[b, t]]``.  ``base`` (``[B, T, d]`` or ``[B * T, d]``, contiguous,
        on the device, in the output dtype) takes the place of ``wte[tok]``; token ids serve the match only (no vocabulary).
        On a ``longest_suffix`` table a matched f-gram replaces the base row.  ``out=base`` is the in-place call and is passed
        through untouched; an ``out`` that overlaps ``base`` in any other way is refused (``ValueError``)."""
        if not (tok.dim() == 2 and tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
            tok = self._tok(tok)
        B, T = tok.shape
        out_dtype, out = self._base_args("embed_base", B * T, base, wpe, out_dtype, out, (B, T, self.dim))
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).expand(B, T).contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = L.lib().scone_embed_base(self._h, tok.data_ptr(), B, T, base.data_ptr(), None if wpe is None else wpe.data_ptr(),
                                      0 if wpe is None else wpe.shape[0],
                                      None if position_ids is None else position_ids.data_ptr(), _REDUCE[reduce],
                                      out.data_ptr(), _DT[out_dtype], stream)
        if rc != L.OK:
            self._check(rc, "scone_embed_base")
        return out

    def embed_base_varlen(self, tok: torch.Tensor, cu_seqlens, base: torch.Tensor, *, wpe: Optional[torch.Tensor] = None,
                          position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
                          out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_embed_base_varlen``: :meth:`embed_varlen` onto a dense ``base [total, d]`` -> ``[total, d]`` (see
        :meth:`embed_base`; ``cu_seqlens`` as in :meth:`embed_varlen`)."""
        if tok.dim() != 1:
            raise ValueError("embed_base_varlen takes the packed token ids as a 1-D tensor [total]")
        if not (tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
            tok = tok.to(device=self.device, dtype=torch.int32).contiguous()
        total = tok.shape[0]
        if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
            if not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                    and cu_seqlens.numel() >= 1):
                raise ValueError("a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
            cu = cu_seqlens
        else:
            cu = torch.from_numpy(check_cu_seqlens(cu_seqlens, total)).to(self.device)
        n_seqs = cu.numel() - 1
        out_dtype, out = self._base_args("embed_base_varlen", total, base, wpe, out_dtype, out, (total, self.dim))
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if position_ids.numel() != total:
                raise ValueError(f"position_ids must hold one position per packed token ({total})")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = L.lib().scone_embed_base_varlen(self._h, tok.data_ptr(), cu.data_ptr(), n_seqs, total, base.data_ptr(),
                                             None if wpe is None else wpe.data_ptr(), 0 if wpe is None else wpe.shape[0],
                                             None if position_ids is None else position_ids.data_ptr(), _REDUCE[reduce],
                                             out.data_ptr(), _DT[out_dtype], stream)
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"scone_embed_base_varlen: {L.lib().scone_last_error(self._h).decode()} "
                                       f"[{L.lib().scone_strerror(rc).decode()}]")
        if rc != L.OK:
            self._check(rc, "scone_embed_base_varlen")
        return out

    def embed_rows(self, tok: torch.Tensor, row_ids: torch.Tensor, rows: torch.Tensor, *, n: Optional[torch.Tensor] = None,
                   cu_seqlens=None, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                   base: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, reduce: str = "mean",
                   out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_embed_rows`` / ``scone_embed_rows_varlen``: the fused lookup over a batch's LIVE rows -> ``[B, T, d]``
        (``tok [B, T]``) or ``[total, d]`` (``tok [total]`` with ``cu_seqlens=``).  The rows come from ``rows [U, d]`` (fp32 /
        fp16 / bf16, on the device) keyed by ``row_ids [U]`` (int64, ascending and distinct: :meth:`BackwardPlan.row_ids`), not
        from the table, which is never read; the output has the bits :meth:`embed` / :meth:`embed_base` / the packed forms
        give on a table of ``rows.dtype`` that holds ``rows[u]`` in row ``row_ids[u]``.  A hit whose id is not listed adds a
        row of zeros (the divisor stays the full hit count) and raises bit 1 of :meth:`status`.  ``n``: an int64 device scalar,
        ``min(n, U)`` rows are live (read on the stream).  ``wte`` and ``base`` are exclusive; ``out=base`` is the in-place
        call; ``pos`` are explicit position ids.  Every argument check raises :class:`SconeInvalidArgument` before any device
        work; a ``rows`` that is not contiguous or not 16-byte aligned is copied.  Stream-ordered, two launches."""
        who = "embed_rows"
        if not isinstance(tok, torch.Tensor) or not isinstance(row_ids, torch.Tensor) or not isinstance(rows, torch.Tensor):
            raise SconeInvalidArgument(f"{who}: tok, row_ids and rows must be tensors")
        packed = cu_seqlens is not None
        if packed:
            if tok.dim() != 1:
                raise SconeInvalidArgument(f"{who}: with cu_seqlens= the packed token ids are a 1-D tensor [total]")
            ntok, shape = tok.shape[0], (tok.shape[0], self.dim)
            if not (isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda):
                try:
                    cu_seqlens = check_cu_seqlens(cu_seqlens, ntok)
                except ValueError as e:
                    raise SconeInvalidArgument(f"{who}: {e}") from None
            elif not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                      and cu_seqlens.numel() >= 1):
                raise SconeInvalidArgument(f"{who}: a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
        else:
            if tok.dim() == 1:
                tok = tok.unsqueeze(0)
            if tok.dim() != 2:
                raise SconeInvalidArgument(f"{who}: token ids must be [T] or [B, T]")
            ntok, shape = tok.numel(), (tok.shape[0], tok.shape[1], self.dim)
        if row_ids.dtype != torch.int64 or row_ids.dim() != 1:
            raise SconeInvalidArgument(f"{who}: row_ids must be a 1-D int64 tensor, got {row_ids.dtype} {tuple(row_ids.shape)}")
        if rows.dtype not in _DT:
            raise SconeInvalidArgument(f"{who}: rows must be float32, float16 or bfloat16, not {rows.dtype}")
        if rows.dim() != 2 or rows.shape[1] != self.dim or rows.shape[0] != row_ids.shape[0]:
            raise SconeInvalidArgument(f"{who}: rows must be [{row_ids.shape[0]}, {self.dim}] (one row per row id), "
                                       f"got {tuple(rows.shape)}")
        if rows.shape[0] > L.LIVE_ROWS_MAX:
            raise SconeInvalidArgument(f"{who}: at most 2^31 - 1 live rows")
        if self.dim % 8 != 0:
            raise SconeInvalidArgument(f"{who}: needs d % 8 == 0")
        if n is not None and not (isinstance(n, torch.Tensor) and n.dtype == torch.int64 and n.numel() == 1):
            raise SconeInvalidArgument(f"{who}: n must be an int64 tensor of one element (the live count on the device)")
        if reduce not in _REDUCE:
            raise SconeInvalidArgument(f"{who}: unknown reduce {reduce!r}")
        if wte is not None and base is not None:
            raise SconeInvalidArgument(f"{who}: wte and base are exclusive")
        if out_dtype is None:
            out_dtype = next((t.dtype for t in (base, wte, wpe, out) if t is not None), torch.float32)
        if out_dtype not in _DT:
            raise SconeInvalidArgument(f"{who}: out_dtype must be float32, float16 or bfloat16")
        if base is not None and not (isinstance(base, torch.Tensor) and base.dim() >= 2 and base.shape[-1] == self.dim
                                     and base.numel() == ntok * self.dim and (not packed or base.dim() == 2)):
            raise SconeInvalidArgument(f"{who}: base must hold {ntok} rows of {self.dim}" + (f": [{ntok}, {self.dim}]" if packed else "")
                                       + f", got {tuple(base.shape) if isinstance(base, torch.Tensor) else type(base).__name__}")
        for name, w in (("base", base), ("wte", wte), ("wpe", wpe)):
            if w is not None and not (w.is_cuda and w.is_contiguous() and w.dtype == out_dtype and w.dim() >= 2
                                      and w.shape[-1] == self.dim):
                raise SconeInvalidArgument(f"{who}: {name} must be a contiguous [*, {self.dim}] {out_dtype} tensor on the device")
        if pos is not None and not (isinstance(pos, torch.Tensor) and not pos.dtype.is_floating_point):
            raise SconeInvalidArgument(f"{who}: pos must be an integer tensor")
        if pos is not None and packed and pos.numel() != ntok:
            raise SconeInvalidArgument(f"{who}: pos must hold one position per packed token ({ntok})")
        if out is not None and not (out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and out.numel() == ntok * self.dim):
            raise SconeInvalidArgument(f"{who}: out must be a contiguous {out_dtype} tensor of {ntok} rows of {self.dim} on the device")
        # ---- device work from here
        if not (tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
            tok = tok.to(device=self.device, dtype=torch.int32).contiguous()
        row_ids = row_ids.to(device=self.device).contiguous()
        rows = rows.to(device=self.device)
        if not rows.is_contiguous() or rows.data_ptr() % 16 != 0:
            rows = rows.contiguous() if not rows.is_contiguous() else rows.clone()
        if n is not None:
            n = n.to(device=self.device).reshape(1)
        if pos is not None:
            pos = pos.to(device=self.device, dtype=torch.int32)
            pos = (pos.reshape(-1) if packed else pos.expand(tok.shape)).contiguous()
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=self.device)
        live = L.SconeLiveRows(C.sizeof(L.SconeLiveRows), _DT[rows.dtype], row_ids.data_ptr() or None, rows.data_ptr() or None,
                               rows.shape[0], None if n is None else n.data_ptr())
        tail = (None if wte is None else wte.data_ptr(), 0 if wte is None else wte.shape[0],
                None if base is None else base.data_ptr(), None if wpe is None else wpe.data_ptr(),
                0 if wpe is None else wpe.shape[0], None if pos is None else pos.data_ptr(), _REDUCE[reduce], out.data_ptr(),
                _DT[out_dtype], torch.cuda.current_stream(self.device).cuda_stream)
        if packed:
            cu = cu_seqlens if isinstance(cu_seqlens, torch.Tensor) else torch.from_numpy(cu_seqlens).to(self.device)
            name = "scone_embed_rows_varlen"
            rc = L.lib().scone_embed_rows_varlen(self._h, C.byref(live), tok.data_ptr(), cu.data_ptr(), cu.numel() - 1, ntok, *tail)
        else:
            name = "scone_embed_rows"
            rc = L.lib().scone_embed_rows(self._h, C.byref(live), tok.data_ptr(), tok.shape[0], tok.shape[1], *tail)
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"{name}: {L.lib().scone_last_error(self._h).decode()} [{L.lib().scone_strerror(rc).decode()}]")
        if rc != L.OK:
            self._check(rc, name)
        stream = torch.cuda.current_stream(self.device)
        for x in (rows, row_ids, tok, n, pos):            # they may be temporaries made here
            if x is not None and x.numel():
                x.record_stream(stream)
        return out

    def embed_select(self, tok: torch.Tensor, sel, *, cu_seqlens=None, wte: Optional[torch.Tensor] = None,
                     base: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                     position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
                     out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_embed_select``: the fused lookup at CHOSEN positions only -> ``[n_sel, d]``.  ``out[j]`` holds exactly what
        :meth:`embed` (``tok [B, T]``) or :meth:`embed_varlen` (``tok [total]`` with ``cu_seqlens=``) writes to its flattened
        row ``sel[j]``, matched against the whole context -- one launch, for a decoding step's last tokens, a verify step's last
        k, a prefill chunk.  ``sel`` (any order, repeats allowed) indexes the flattened tokens; ``base [n_sel, d]`` and
        ``position_ids [n_sel]`` are per SELECTED row; ``wte`` and ``base`` are exclusive; ``out=base`` is the in-place call.
        A ``sel`` entry outside ``[0, total)`` leaves its row unwritten and raises bit 0 of :meth:`status`.  Refusals of the
        library come back as :class:`SconeInvalidArgument`."""
        if cu_seqlens is None:
            if not (tok.dim() == 2 and tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
                tok = self._tok(tok)
            total, T = tok.numel(), tok.shape[1]
            cu, n_seqs = None, 0
        else:
            if tok.dim() != 1:
                raise ValueError("embed_select with cu_seqlens takes the packed token ids as a 1-D tensor [total]")
            if not (tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()):
                tok = tok.to(device=self.device, dtype=torch.int32).contiguous()
            total, T = tok.shape[0], 0
            if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
                if not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                        and cu_seqlens.numel() >= 1):
                    raise ValueError("a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
                cu = cu_seqlens
            else:
                cu = torch.from_numpy(check_cu_seqlens(cu_seqlens, total)).to(self.device)
            n_seqs = cu.numel() - 1
        if not isinstance(sel, torch.Tensor):
            sel = torch.from_numpy(np.ascontiguousarray(np.asarray(sel, dtype=np.int64).astype(np.int32)))
        if sel.dim() != 1:
            raise ValueError("embed_select: sel must be a 1-D list of flattened token positions")
        if not (sel.dtype == torch.int32 and sel.is_cuda and sel.is_contiguous()):
            sel = sel.to(device=self.device, dtype=torch.int32).contiguous()
        n_sel = sel.shape[0]
        if wte is not None and base is not None:
            raise SconeInvalidArgument("embed_select: wte and base are exclusive")
        if base is not None:
            out_dtype, out = self._base_args("embed_select", n_sel, base, wpe, out_dtype, out, (n_sel, self.dim))
        else:
            if out_dtype is None:
                out_dtype = wte.dtype if wte is not None else (wpe.dtype if wpe is not None else torch.float32)
            if out_dtype not in _DT:
                raise ValueError("embed_select: out_dtype must be float32, float16 or bfloat16")
            for name, w in (("wte", wte), ("wpe", wpe)):
                if w is not None:
                    if not (w.is_cuda and w.is_contiguous() and w.dtype == out_dtype and w.dim() == 2
                            and w.shape[1] == self.dim):
                        raise ValueError(f"{name} must be a contiguous [*, {self.dim}] {out_dtype} tensor on {self.device}")
            if out is None:
                out = torch.empty((n_sel, self.dim), dtype=out_dtype, device=self.device)
            else:
                assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and out.numel() == n_sel * self.dim
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if position_ids.numel() != n_sel:
                raise ValueError(f"position_ids must hold one position per selected row ({n_sel})")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = L.lib().scone_embed_select(self._h, tok.data_ptr(), total, T, None if cu is None else cu.data_ptr(), n_seqs,
                                        sel.data_ptr(), n_sel, None if wte is None else wte.data_ptr(),
                                        0 if wte is None else wte.shape[0], None if base is None else base.data_ptr(),
                                        None if wpe is None else wpe.data_ptr(), 0 if wpe is None else wpe.shape[0],
                                        None if position_ids is None else position_ids.data_ptr(), _REDUCE[reduce],
                                        out.data_ptr(), _DT[out_dtype], stream)
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"scone_embed_select: {L.lib().scone_last_error(self._h).decode()} "
                                       f"[{L.lib().scone_strerror(rc).decode()}]")
        if rc != L.OK:
            self._check(rc, "scone_embed_select")
        return out

    # -- backward ---------------------------------------------------------------
    def _make_plan(self, rc: int, who: str, plan, ntok: int, n_rows, n_refs) -> BackwardPlan:
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"{who}: {L.lib().scone_last_error(self._h).decode()} "
                                       f"[{L.lib().scone_strerror(rc).decode()}]")
        self._check(rc, who)
        return BackwardPlan(self, plan, ntok, n_rows.value, n_refs.value)

    def backward_plan(self, tok: torch.Tensor, cu_seqlens=None) -> BackwardPlan:
        """``scone_backward_plan`` / ``scone_backward_plan_varlen``: the plan of the table gradient of the batch :meth:`embed`
        (``tok [B, T]``) or :meth:`embed_varlen` (``tok [total]`` with ``cu_seqlens``, validated as there) looks up.
        Synchronises the current stream once."""
        plan, n_rows, n_refs = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if cu_seqlens is None:
            tok = self._tok(tok)
            B, T = tok.shape
            rc = L.lib().scone_backward_plan(self._h, tok.data_ptr(), B, T, C.byref(plan), C.byref(n_rows), C.byref(n_refs), stream)
            return self._make_plan(rc, "scone_backward_plan", plan, B * T, n_rows, n_refs)
        if tok.dim() != 1:
            raise ValueError("a packed batch takes its token ids as a 1-D tensor [total]")
        tok = tok.to(device=self.device, dtype=torch.int32).contiguous()
        total = tok.shape[0]
        if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
            if not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                    and cu_seqlens.numel() >= 1):
                raise ValueError("a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
            cu = cu_seqlens
        else:
            cu = torch.from_numpy(check_cu_seqlens(cu_seqlens, total)).to(self.device)
        rc = L.lib().scone_backward_plan_varlen(self._h, tok.data_ptr(), cu.data_ptr(), cu.numel() - 1, total, C.byref(plan),
                                                C.byref(n_rows), C.byref(n_refs), stream)
        return self._make_plan(rc, "scone_backward_plan_varlen", plan, total if cu.numel() > 1 else 0, n_rows, n_refs)

    def backward_context(self, max_tokens: int) -> BackwardContext:
        """``scone_backward_ctx_create``: a :class:`BackwardContext` for batches of up to ``max_tokens`` positions -- the
        backward whose plan and counts stay on the device (no synchronisation, no allocation per step; capturable).
        Allocates (and so synchronises) once, here; ``.nbytes`` reports the device memory held."""
        return BackwardContext(self, max_tokens)

    def rows_overflowed(self) -> bool:
        """Reads and CLEARS the sticky status bits (as :meth:`status`; synchronises) and tells whether bit 4 was set: a
        :meth:`BackwardContext.rows` found more rows than its buffers hold, wrote none and left ``n = 0``."""
        return bool(self.status() & L.ST_ROWS_OVERFLOW)

    def backward_plan_csr(self, offsets: torch.Tensor, ids: torch.Tensor) -> BackwardPlan:
        """``scone_backward_plan_csr``: the plan of the caller's id lists (``offsets [ntok + 1]``, ``ids``), the counterpart
        of :meth:`gather_reduce`.  Host ``offsets`` are checked here: ``offsets[-1]`` (the library reads no id at or beyond it)
        must lie in ``[0, ids.numel()]``.  Device ``offsets`` are trusted, as a device ``cu_seqlens`` is."""
        if not offsets.is_cuda and offsets.numel():
            total = int(offsets.reshape(-1)[-1])
            if total < 0 or total > ids.numel():
                raise ValueError(f"backward_plan_csr: offsets[-1] = {total} is outside [0, ids.numel() = {ids.numel()}]")
        offsets = offsets.to(device=self.device, dtype=torch.int32).contiguous()
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        ntok = max(offsets.numel() - 1, 0)
        plan, n_rows, n_refs = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = L.lib().scone_backward_plan_csr(self._h, offsets.data_ptr() if offsets.numel() else None,
                                             ids.data_ptr() if ids.numel() else None, ntok, C.byref(plan), C.byref(n_rows),
                                             C.byref(n_refs), stream)
        return self._make_plan(rc, "scone_backward_plan_csr", plan, ntok, n_rows, n_refs)

    # -- backward of the dense side (wte / wpe) -----------------------------------
    def backward_plan_index(self, idx: torch.Tensor, n_ids: int, skip: Optional[torch.Tensor] = None) -> BackwardPlan:
        """``scone_backward_plan_index``: the plan of a dense embedding's gradient -- position ``p`` refers to row ``idx[p]`` of
        an id space of ``n_ids`` rows (``wte``: the tokens and the vocabulary; ``wpe``: the position ids and ``n_pos``), which
        has nothing to do with the table's.  ``skip`` (int32, as long as ``idx``): positions with ``skip != 0`` have no
        reference; so have ids outside ``[0, n_ids)``, silently.  :meth:`BackwardPlan.rows` then returns the ids with a
        reference and their fp32 gradient rows, summed in the backward's fixed order.  Synchronises the current stream once."""
        idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        ntok = idx.numel()
        if skip is not None:
            skip = torch.as_tensor(skip).to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
            if skip.numel() != ntok:
                raise ValueError(f"backward_plan_index: skip must have the {ntok} elements of idx, got {skip.numel()}")
        plan, n_rows, n_refs = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = L.lib().scone_backward_plan_index(self._h, _ptr(idx) if ntok else None, ntok, int(n_ids),
                                                   _ptr(skip) if skip is not None and ntok else None, C.byref(plan),
                                                   C.byref(n_rows), C.byref(n_refs), stream)
        return self._make_plan(rc, "scone_backward_plan_index", plan, ntok, n_rows, n_refs)

    def default_positions(self, B: Optional[int] = None, T: Optional[int] = None, *, cu_seqlens=None,
                          total: Optional[int] = None) -> torch.Tensor:
        """``scone_backward_default_positions``: the position the lookup gives every ``p`` when it is called without
        ``position_ids``, int32 -- ``[B * T]`` (``p % T``) for ``default_positions(B, T)``, ``[total]`` (``p - cu[s]``) for
        ``default_positions(cu_seqlens=, total=)``.  No synchronisation with a device ``cu_seqlens``."""
        if cu_seqlens is None:
            if B is None or T is None:
                raise ValueError("default_positions: give (B, T) or cu_seqlens= and total=")
            n, cu, n_seqs, T = int(B) * int(T), None, int(B), int(T)
        else:
            if total is None:
                raise ValueError("default_positions: a packed batch needs total=")
            n, T = int(total), 0
            if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
                if not (cu_seqlens.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
                        and cu_seqlens.numel() >= 1):
                    raise ValueError("a device cu_seqlens must be a contiguous 1-D int32 tensor [n_seqs + 1]")
                cu = cu_seqlens
            else:
                cu = torch.from_numpy(check_cu_seqlens(cu_seqlens, n)).to(self.device)
            n_seqs = cu.numel() - 1
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = L.lib().scone_backward_default_positions(self._h, _ptr(cu), n_seqs, T, n, _ptr(out) if n else None,
                                                          stream.cuda_stream)
        if rc == L.EINVAL:
            raise SconeInvalidArgument(f"scone_backward_default_positions: {L.lib().scone_last_error(self._h).decode()} "
                                       f"[{L.lib().scone_strerror(rc).decode()}]")
        self._check(rc, "scone_backward_default_positions")
        if cu is not None and n:
            cu.record_stream(stream)
        return out

    def backward_wpe(self, grad_out: torch.Tensor, n_pos: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_backward_wpe``: the gradient of ``wpe`` for a rectangle looked up with default positions -- fp32
        ``[min(T, n_pos), d]``, row ``t`` the sum of ``grad_out[b, t, :]`` over ``b`` ascending in the backward's fixed order
        (the bits of :meth:`backward_plan_index` on :meth:`default_positions`).  ``grad_out``: ``[B, T, d]`` fp32 / fp16 / bf16.
        No plan, no sort, no synchronisation; the scratch of a batch of more than ``backward_chunk()`` sequences is kept on the
        table and grows only when a larger batch comes."""
        if grad_out.dim() != 3 or grad_out.shape[-1] != self.dim:
            raise ValueError(f"grad_out must be [B, T, {self.dim}], got {tuple(grad_out.shape)}")
        if grad_out.dtype not in _DT:
            raise ValueError(f"grad_out must be fp32, fp16 or bf16, not {grad_out.dtype}")
        if int(n_pos) <= 0:
            raise ValueError("backward_wpe: n_pos must be positive")
        if not (grad_out.is_cuda and grad_out.device == self.device and grad_out.is_contiguous()):
            grad_out = grad_out.to(device=self.device).contiguous()
        B, T = int(grad_out.shape[0]), int(grad_out.shape[1])
        rows = min(T, int(n_pos)) if B else 0
        if out is None:
            out = torch.empty((rows, self.dim), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.device == self.device and out.is_contiguous() and out.dtype == torch.float32
                  and tuple(out.shape) == (rows, self.dim)):
            raise ValueError(f"out must be a contiguous fp32 [{rows}, {self.dim}] tensor on {self.device}")
        need = L.backward_wpe_scratch(B, T, self.dim)
        scratch = getattr(self, "_wpe_scratch", None)
        if need and (scratch is None or scratch.numel() < need):
            scratch = self._wpe_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = L.lib().scone_backward_wpe(self._h, _ptr(grad_out) if B * T else None, _DT[grad_out.dtype], B, T, int(n_pos),
                                            _ptr(out) if rows else None, _ptr(scratch) if need else None, stream.cuda_stream)
        self._check(rc, "scone_backward_wpe")
        if B * T:
            grad_out.record_stream(stream)                       # it may be a temporary of the caller
            if need:
                scratch.record_stream(stream)
        return out

    def _sparse_operand(self, who: str, ids: torch.Tensor, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(ids, rows)`` of a sparse row gradient, checked and made contiguous on the table's device."""
        if ids.dim() != 1 or ids.dtype != torch.int64:
            raise ValueError(f"{who}: row ids must be int64 [n], got {ids.dtype} {tuple(ids.shape)}")
        if rows.dim() != 2 or rows.shape != (ids.shape[0], self.dim) or rows.dtype != torch.float32:
            raise ValueError(f"{who}: rows must be fp32 [{ids.shape[0]}, {self.dim}], got {rows.dtype} {tuple(rows.shape)}")
        return ids.to(device=self.device).contiguous(), rows.to(device=self.device).contiguous()

    def _step_operands(self, who: str, row_ids: torch.Tensor, grad_rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(row_ids, grad_rows)`` of an optimizer step: :meth:`_sparse_operand`'s conditions, refused in the steps' own words."""
        if row_ids.dim() != 1 or grad_rows.dim() != 2 or grad_rows.shape[0] != row_ids.numel() or grad_rows.shape[1] != self.dim:
            raise ValueError(f"{who}: row_ids [U] and grad_rows [U, {self.dim}], got {tuple(row_ids.shape)} and "
                             f"{tuple(grad_rows.shape)}")
        if row_ids.dtype != torch.int64 or grad_rows.dtype != torch.float32:
            raise ValueError(f"{who}: row_ids must be int64 and grad_rows fp32")
        return row_ids.to(device=self.device).contiguous(), grad_rows.to(device=self.device).contiguous()

    def _state_operand(self, who: str, name: str, t: Optional[torch.Tensor], shape: tuple, needed: bool) -> None:
        """A master or state tensor of an optimizer step: absent only if the kind does not need it, else contiguous fp32 of
        ``shape`` on the table's device (it is updated in place, so it is never copied or moved)."""
        if t is None:
            if needed:
                raise ValueError(f"{who}: this kind needs {name}")
        elif not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == shape and t.device == self.device
                  and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous fp32 {list(shape)} tensor on {self.device} (it is updated in place)")

    def _step_call(self, base: str, cfg, dh_prefix: tuple, row_ids: torch.Tensor, grad_rows: torch.Tensor, states: tuple,
                   ctl: Optional["GradCtl"], n: Optional[torch.Tensor], hyper: Optional[OptHyper]) -> None:
        """One optimizer step through the form of ``base`` (``scone_opt_step`` / ``scone_opt_step_lean``) that ``(ctl, n, hyper)``
        select: ``_dh`` with ``hyper`` (``dh_prefix``, the kind -- and rounding -- by value, stands where the others take the cfg),
        ``_dn`` with ``n``, ``_ctl`` with ``ctl`` alone, else the plain call.  ``states``: the master and state tensors, in the
        entry point's order.  The operands are recorded on the stream (they may be temporaries of the caller) in the forms without
        ``n``; with ``n`` they are buffers the caller keeps across steps."""
        U = row_ids.numel()
        if n is not None:
            n = _device_count(base[len("scone_"):], n, self.device)
        head = dh_prefix if hyper is not None else (C.byref(cfg),)
        rows = (_ptr(row_ids), _ptr(grad_rows), *(() if n is None else (_ptr(n),)), U, *(_ptr(t) for t in states))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if hyper is not None:
                name, tail = base + "_dh", (_ptr(hyper.buf), None if ctl is None else _ptr(ctl.buf))
            elif n is not None:
                name, tail = base + "_dn", (None if ctl is None else _ptr(ctl.buf),)
            elif ctl is not None:
                name, tail = base + "_ctl", (_ptr(ctl.buf),)
            else:
                name, tail = base, ()
            rc = getattr(L.lib(), name)(self._h, *head, *rows, *tail, stream.cuda_stream)
        self._check(rc, name)
        if n is None and U:
            row_ids.record_stream(stream)
            grad_rows.record_stream(stream)

    def grad_merge_map(self, ids_a: torch.Tensor, ids_b: torch.Tensor, sync: bool = True) -> GradMergeMap:
        """``scone_grad_merge_map``: the union of two ascending lists of distinct int64 row ids and the maps between the three
        row numberings (include/scone_hip.h, "gradient accumulation"), a :class:`GradMergeMap`.  ``sync=True`` synchronises
        the current stream once (8 bytes) and trims the results to ``n_out``; ``sync=False`` does not synchronise and leaves
        them at their capacity ``n_a + n_b`` with ``n_out = None`` (the count is the device tensor ``d_n_out``)."""
        for x in (ids_a, ids_b):
            if x.dim() != 1 or x.dtype != torch.int64:
                raise ValueError(f"grad_merge_map: row ids must be int64 [n], got {x.dtype} {tuple(x.shape)}")
        ids_a, ids_b = ids_a.to(device=self.device).contiguous(), ids_b.to(device=self.device).contiguous()
        n_a, n_b = ids_a.numel(), ids_b.numel()
        dev = self.device
        ids = torch.empty(n_a + n_b, dtype=torch.int64, device=dev)
        words = torch.empty(3 * (n_a + n_b) + 2, dtype=torch.int32, device=dev)       # src_a | src_b | pos_a | pos_b | n_out
        src_a, src_b = words[:n_a + n_b], words[n_a + n_b:2 * (n_a + n_b)]
        pos_a, pos_b = words[2 * (n_a + n_b):2 * (n_a + n_b) + n_a], words[2 * (n_a + n_b) + n_a:3 * (n_a + n_b)]
        d_n_out = torch.empty(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.grad_merge_scratch(n_a, n_b), dtype=torch.uint8, device=dev)
        h_n_out = C.c_uint64(0)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            rc = L.lib().scone_grad_merge_map(self._h, _ptr(ids_a) if n_a else None, n_a, _ptr(ids_b) if n_b else None, n_b,
                                              _ptr(ids), _ptr(src_a), _ptr(src_b), _ptr(pos_a), _ptr(pos_b), _ptr(scratch),
                                              _ptr(d_n_out), C.byref(h_n_out) if sync else None, stream.cuda_stream)
        self._check(rc, "scone_grad_merge_map")
        for x in (ids_a, ids_b, scratch):
            if x.numel():
                x.record_stream(stream)
        if not sync:
            return GradMergeMap(ids, src_a, src_b, pos_a, pos_b, d_n_out, None)
        n = int(h_n_out.value)
        return GradMergeMap(ids[:n], src_a[:n], src_b[:n], pos_a, pos_b, d_n_out, n)

    def grad_merge_rows(self, m: GradMergeMap, rows_a: torch.Tensor, rows_b: torch.Tensor,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``scone_grad_merge_rows``: the rows of the merged gradient, fp32 ``[n_out, d]`` -- a row one operand has is that row,
        bit for bit; a row both have is ``a + b``, one fp32 add.  ``m``: a synchronised :class:`GradMergeMap` of the two id
        lists.  One launch on the current stream."""
        if m.n_out is None:
            raise ValueError("grad_merge_rows: the map must know n_out (grad_merge_map(sync=True))")
        for x in (rows_a, rows_b):
            if x.dim() != 2 or x.shape[1] != self.dim or x.dtype != torch.float32 or not (x.is_cuda and x.device == self.device
                                                                                          and x.is_contiguous()):
                raise ValueError(f"grad_merge_rows: rows must be contiguous fp32 [n, {self.dim}] on {self.device}")
        if rows_a.shape[0] != m.pos_a.numel() or rows_b.shape[0] != m.pos_b.numel():
            raise ValueError("grad_merge_rows: the rows are not those of the map's lists")
        if out is None:
            out = torch.empty((m.n_out, self.dim), dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.dim() == 2 and out.shape[1] == self.dim and out.shape[0] >= m.n_out
                  and out.device == self.device and out.is_contiguous()):
            raise ValueError(f"grad_merge_rows: out must be a contiguous fp32 [>= {m.n_out}, {self.dim}] tensor on {self.device}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = L.lib().scone_grad_merge_rows(self._h, _ptr(m.src_a), _ptr(m.src_b), m.n_out,
                                               _ptr(rows_a) if rows_a.shape[0] else None,
                                               _ptr(rows_b) if rows_b.shape[0] else None, _ptr(out) if out.shape[0] else None,
                                               stream.cuda_stream)
        self._check(rc, "scone_grad_merge_rows")
        for x in (rows_a, rows_b, m.src_a, m.src_b):
            if x.numel():
                x.record_stream(stream)
        return out[:m.n_out]

    def grad_merge(self, ids_a: torch.Tensor, rows_a: torch.Tensor, ids_b: torch.Tensor,
                   rows_b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The sum of two sparse row gradients ``(ids, rows)`` -- int64 ascending and distinct, fp32 ``[n, d]``, what
        :meth:`BackwardPlan.rows` returns -- as one more: ``scone_grad_merge_map`` (one 8-byte synchronise for the size of the
        union), then ``scone_grad_merge_rows``.  Gradient accumulation over micro-batches without ``coalesce()``."""
        ids_a, rows_a = self._sparse_operand("grad_merge", ids_a, rows_a)
        ids_b, rows_b = self._sparse_operand("grad_merge", ids_b, rows_b)
        m = self.grad_merge_map(ids_a, ids_b)
        return m.ids, self.grad_merge_rows(m, rows_a, rows_b)

    def grad_sqnorm(self, grad_rows: torch.Tensor, scratch: Optional[torch.Tensor] = None, *, n: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``scone_grad_sqnorm``: the squared norm of ``grad_rows`` (fp32 ``[U, d]``, what :meth:`BackwardPlan.rows` returns),
        summed in double in the fixed order of include/scone_hip.h, "gradient norm, clipping and skipped steps".  Returns
        ``(sq, row_sq)``: a 0-dim float64 device tensor and the per-row squared norms, a float64 ``[U]`` view of the call's
        scratch.  ``scratch``: a contiguous float64 device tensor of at least ``_lib.grad_sqnorm_scratch(U)`` elements to use
        instead of a fresh one (the tile sums follow the row sums in it).  At most three launches on the current stream; no
        synchronisation.  ``n`` (a 1-element int64 device tensor, :meth:`BackwardContext.rows`' third result):
        ``scone_grad_sqnorm_dn`` -- the norm of the first ``min(n, U)`` rows, ``U`` now the capacity; the same bits.  ``out``: a
        0-dim float64 device tensor to write ``sq`` to instead of a fresh one."""
        if grad_rows.dim() != 2 or grad_rows.shape[1] != self.dim or grad_rows.dtype != torch.float32:
            raise ValueError(f"grad_sqnorm: grad_rows must be fp32 [U, {self.dim}], got {grad_rows.dtype} {tuple(grad_rows.shape)}")
        grad_rows = grad_rows.to(device=self.device).contiguous()
        n_dev, n = n, grad_rows.shape[0]
        need = L.grad_sqnorm_scratch(n)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        elif not (isinstance(scratch, torch.Tensor) and scratch.dtype == torch.float64 and scratch.dim() == 1 and scratch.numel() >= need
                  and scratch.device == self.device and scratch.is_contiguous()):
            raise ValueError(f"grad_sqnorm: scratch must be a contiguous float64 tensor of at least {need} elements on {self.device}")
        if out is None:
            sq = torch.empty((), dtype=torch.float64, device=self.device)
        elif isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.numel() == 1 and out.device == self.device:
            sq = out
        else:
            raise ValueError(f"grad_sqnorm: out must be a one-element float64 tensor on {self.device}")
        if n_dev is not None:
            n_dev = _device_count("grad_sqnorm", n_dev, self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if n_dev is None:
                rc = L.lib().scone_grad_sqnorm(self._h, _ptr(grad_rows) if n else None, n, _ptr(scratch) if need else None, _ptr(sq),
                                               stream.cuda_stream)
            else:
                rc = L.lib().scone_grad_sqnorm_dn(self._h, _ptr(grad_rows) if n else None, _ptr(n_dev), n,
                                                  _ptr(scratch) if need else None, _ptr(sq), stream.cuda_stream)
        self._check(rc, "scone_grad_sqnorm" if n_dev is None else "scone_grad_sqnorm_dn")
        if n and n_dev is None:
            grad_rows.record_stream(stream)                        # it may be a temporary of the caller
        return sq, scratch[:n]

    def opt_hyper(self, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0,
                  seed: int = 0, step: int = 0, out: Optional[OptHyper] = None) -> OptHyper:
        """``scone_opt_hyper_init``: an :class:`OptHyper` on the table's device holding these hyper-parameters, ``seed`` (stochastic
        rounding) and ``step``, the number of steps ALREADY applied (0 for a fresh optimizer).  One launch on the current stream;
        no synchronisation.  ``out``: a block to re-initialise instead of a fresh one."""
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must fit 64 unsigned bits")
        cfg = _opt_cfg(L.OPT_SGD, lr, betas, eps, weight_decay, grad_scale, step)
        hyper = OptHyper(self.device) if out is None else out
        with torch.cuda.device(self.device):
            rc = L.lib().scone_opt_hyper_init(self._h, C.byref(cfg), int(seed), _ptr(hyper.buf),
                                              torch.cuda.current_stream(self.device).cuda_stream)
        self._check(rc, "scone_opt_hyper_init")
        return hyper

    def opt_hyper_advance(self, hyper: OptHyper, kind, ctl: Optional["GradCtl"] = None) -> None:
        """``scone_opt_hyper_advance``: count one optimizer step in ``hyper`` and derive the fp32 scalars of ``kind`` (``"sgd"``,
        ``"adagrad"``, ``"adam"``; the lean kinds advance as ``"sgd"``) on the device -- once per step, before the
        ``opt_step(..., hyper=)`` / ``opt_step_lean(..., hyper=)`` calls of every table or shard that shares the block.  With
        ``ctl`` whose ``skip`` is set nothing is counted and the steps behind it change nothing; a hyper-parameter that is not
        finite sets ``hyper.bad`` instead.  One launch on the current stream; no synchronisation."""
        if isinstance(kind, str):
            k = kind.lower()
            if k not in _OPT and k not in _LEAN:
                raise ValueError(f"unknown optimizer kind {kind!r} (sgd, adagrad, adam, rowwise_adagrad)")
            kind = _OPT.get(k, L.OPT_SGD)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_opt_hyper_advance(self._h, int(kind), _ptr(hyper.buf), None if ctl is None else _ptr(ctl.buf),
                                                 torch.cuda.current_stream(self.device).cuda_stream)
        self._check(rc, "scone_opt_hyper_advance")

    def grad_ctl(self, terms, grad_scale: Optional[float] = None, max_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 out: Optional[GradCtl] = None, hyper: Optional[OptHyper] = None) -> GradCtl:
        """``scone_grad_ctl_set``: a :class:`GradCtl` from squared-norm ``terms`` that stay on the device -- a sequence of 0-dim
        tensors (``grad_sqnorm``'s ``sq``, the dense parameters' squared norm, other shards') and floats, or one 1-D tensor; they
        are added in the order given, in double.  ``grad_scale`` is the un-scaling factor the step will use (the norm is that of
        the un-scaled gradient); ``max_norm=None`` does not clip; ``skip_nonfinite`` sets the block's ``skip`` when the sum is inf
        or NaN.  One launch on the current stream; no synchronisation.  ``out``: a :class:`GradCtl` to fill instead of a fresh one
        (a captured step keeps one).  ``hyper`` (an :class:`OptHyper`): ``scone_grad_ctl_set_dh`` -- ``grad_scale`` is read from the
        block on the device (the same bits; a scale that is not finite there sets ``skip``); ``grad_scale=`` beside it is a
        ``ValueError``."""
        if hyper is not None:
            _no_scalars_beside_hyper("grad_ctl", {"grad_scale": grad_scale})
        elif grad_scale is None:
            grad_scale = 1.0
        if not isinstance(terms, torch.Tensor):
            terms = list(terms)
        if isinstance(terms, torch.Tensor):
            vec = terms.reshape(-1).to(device=self.device, dtype=torch.float64)
        elif len(terms) == 1 and isinstance(terms[0], torch.Tensor) and terms[0].dtype == torch.float64 and terms[0].device == self.device:
            vec = terms[0].detach().reshape(1)                     # the usual case, the table's norm alone: no copy
        elif terms:
            vec = torch.stack([t.detach().to(device=self.device, dtype=torch.float64).reshape(()) if isinstance(t, torch.Tensor)
                               else torch.tensor(float(t), dtype=torch.float64, device=self.device) for t in terms])
        else:
            vec = torch.zeros(0, dtype=torch.float64, device=self.device)
        vec = vec.contiguous()
        ctl = GradCtl(self.device) if out is None else out
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if hyper is None:
                rc = L.lib().scone_grad_ctl_set(self._h, _ptr(vec) if vec.numel() else None, vec.numel(), float(grad_scale),
                                                float("inf") if max_norm is None else float(max_norm), int(bool(skip_nonfinite)),
                                                _ptr(ctl.buf), stream.cuda_stream)
            else:
                rc = L.lib().scone_grad_ctl_set_dh(self._h, _ptr(vec) if vec.numel() else None, vec.numel(), _ptr(hyper.buf),
                                                   float("inf") if max_norm is None else float(max_norm),
                                                   int(bool(skip_nonfinite)), _ptr(ctl.buf), stream.cuda_stream)
        self._check(rc, "scone_grad_ctl_set" if hyper is None else "scone_grad_ctl_set_dh")
        if vec.numel() and out is None:                            # (out=: the caller keeps the block, and its terms with it)
            vec.record_stream(stream)
        return ctl

    def opt_step(self, row_ids: torch.Tensor, grad_rows: torch.Tensor, master: torch.Tensor, *, kind, lr: Optional[float] = None,
                 step: Optional[int] = None, state1: Optional[torch.Tensor] = None, state2: Optional[torch.Tensor] = None,
                 betas=None, eps: Optional[float] = None, weight_decay: Optional[float] = None,
                 grad_scale: Optional[float] = None, ctl: Optional["GradCtl"] = None, n: Optional[torch.Tensor] = None,
                 hyper: Optional[OptHyper] = None) -> None:
        """``scone_opt_step``: the fused sparse optimizer step (include/scone_hip.h, "optimizer step").  ``row_ids`` ``[U]``
        int64 ascending and distinct and ``grad_rows`` ``[U, d]`` fp32 are what :meth:`BackwardPlan.rows` returns.  ``master``,
        ``state1`` (Adam's m) and ``state2`` (Adam's v / Adagrad's sum of squares) are fp32 ``[row_end - row_begin, d]``,
        contiguous, on the table's device: the rows this handle owns, updated in place; the served table receives the updated
        rows in its own format.  ``kind``: ``"sgd"``, ``"adagrad"`` or ``"adam"``.  One kernel launch on the current stream; no
        synchronisation.  ``ctl`` (a :class:`GradCtl`): ``scone_opt_step_ctl`` -- the kernel multiplies ``grad_scale`` by the block's
        ``coef`` and changes nothing at all when its ``skip`` is set.  ``n`` (a 1-element int64 device tensor,
        :meth:`BackwardContext.rows`' third result): ``scone_opt_step_dn`` -- the step over the first ``min(n, U)`` listed rows,
        ``U`` now the capacity of the two buffers; the count is read on the device.  Under capture a replay repeats Adam's
        ``step`` as captured.  ``hyper`` (an :class:`OptHyper`, with ``n``): ``scone_opt_step_dh`` -- the scalars are those
        :meth:`opt_hyper_advance` left in the block, read on the device; the step changes nothing if that advance did not apply.
        ``lr`` (required without ``hyper``), ``step`` (1), ``betas`` ((0.9, 0.999)), ``eps`` (1e-8), ``weight_decay`` (0) and
        ``grad_scale`` (1) are the by-value scalars: any of them beside ``hyper=`` is a ``ValueError``."""
        cfg = _opt_cfg(kind, **_step_scalars("opt_step", _OPT_SCALARS, dict(
            lr=lr, step=step, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale), n, hyper))
        shape = (self.row_end - self.row_begin, self.dim)
        self._state_operand("opt_step", "master", master, shape, True)
        self._state_operand("opt_step", "state1", state1, shape, cfg.kind == L.OPT_ADAM)
        self._state_operand("opt_step", "state2", state2, shape, cfg.kind in (L.OPT_ADAM, L.OPT_ADAGRAD))
        row_ids, grad_rows = self._step_operands("opt_step", row_ids, grad_rows)
        self._step_call("scone_opt_step", cfg, (cfg.kind,), row_ids, grad_rows, (master, state1, state2), ctl, n, hyper)

    def opt_step_lean(self, row_ids: torch.Tensor, grad_rows: torch.Tensor, *, kind, lr: Optional[float] = None,
                      master: Optional[torch.Tensor] = None, row_state: Optional[torch.Tensor] = None, eps: Optional[float] = None,
                      weight_decay: Optional[float] = None, grad_scale: Optional[float] = None, rounding="nearest",
                      seed: Optional[int] = None, step: Optional[int] = None, ctl: Optional["GradCtl"] = None,
                      n: Optional[torch.Tensor] = None, hyper: Optional[OptHyper] = None) -> None:
        """``scone_opt_step_lean``: the lean optimizer step (include/scone_hip.h, "lean optimizer step").  ``kind``: ``"sgd"`` or
        ``"rowwise_adagrad"`` (ONE fp32 accumulator per row: ``row_state``, fp32 ``[row_end - row_begin]``, contiguous, on the
        table's device, updated in place).  ``master`` given (fp32 ``[row_end - row_begin, d]``): it is updated in place and
        the served rows are re-stored in the table's format, as :meth:`opt_step` does.  ``master=None``: IN PLACE -- the served
        fp32 / bf16 rows are the weights; bf16 rows are rounded to ``"nearest"`` or ``"stochastic"`` (random bits keyed by
        ``seed``, ``step``, the global row id and the column).  One kernel launch on the current stream; no synchronisation.
        ``ctl`` (a :class:`GradCtl`): ``scone_opt_step_lean_ctl``, as for :meth:`opt_step`.  ``n`` (a 1-element int64 device
        tensor): ``scone_opt_step_lean_dn``, as for :meth:`opt_step`; under capture a replay repeats the stochastic rounding's
        ``step`` as captured.  ``hyper`` (an :class:`OptHyper`, with ``n``): ``scone_opt_step_lean_dh`` -- the scalars, and the
        random bits' ``seed`` and ``step``, are read from the block on the device, as for :meth:`opt_step`.  ``lr`` (required
        without ``hyper``), ``eps`` (1e-10), ``weight_decay`` (0), ``grad_scale`` (1), ``seed`` (0) and ``step`` (1) are the by-value
        scalars: any of them beside ``hyper=`` is a ``ValueError``."""
        cfg = _lean_cfg(kind, rounding=rounding, **_step_scalars("opt_step_lean", _LEAN_SCALARS, dict(
            lr=lr, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, seed=seed, step=step), n, hyper))
        owned = self.row_end - self.row_begin
        if master is None and self.fmt not in (L.FMT_F32, L.FMT_BF16):
            raise ValueError("opt_step_lean: in place (master=None) needs an fp32 or bf16 table, this one has format code "
                             f"{self.fmt}")
        if cfg.rounding == L.ROUND_STOCHASTIC and (master is not None or self.fmt != L.FMT_BF16):
            raise ValueError("opt_step_lean: stochastic rounding is for in-place bf16 rows (with a master or on an fp32 table "
                             "there is nothing to round)")
        self._state_operand("opt_step_lean", "master", master, (owned, self.dim), False)
        self._state_operand("opt_step_lean", "row_state", row_state, (owned,), cfg.kind == L.LEAN_ROWWISE_ADAGRAD)
        row_ids, grad_rows = self._step_operands("opt_step_lean", row_ids, grad_rows)
        self._step_call("scone_opt_step_lean", cfg, (cfg.kind, cfg.rounding), row_ids, grad_rows, (master, row_state), ctl, n, hyper)

    def embed_prefetch(self, tok: torch.Tensor, tokens_ready: bool = False) -> None:
        """``scone_embed_prefetch``: start the pinned-host prefetch pipeline for ``tok`` (int32 ``[B, T]`` on the device: pass the
        very tensor the later :meth:`embed` gets) behind the current stream -- or, ``tokens_ready=True``, right away (the tokens
        are complete; the prefetch then runs beside a lookup queued just before).  A no-op for other tables."""
        assert tok.dim() == 2 and tok.dtype == torch.int32 and tok.is_cuda and tok.is_contiguous()
        B, T = tok.shape
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(L.lib().scone_embed_prefetch(self._h, tok.data_ptr(), B, T, int(bool(tokens_ready)), stream), "scone_embed_prefetch")
        self._prefetch_keepalive = tok

    def reserve(self, max_tokens: int) -> None:
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_reserve(self._h, int(max_tokens)), "scone_reserve")

    def set_cu_reserve(self, n_reserved: int) -> None:
        """Leave ``n_reserved`` compute units (a multiple of 8; 0 = off) free of this handle's large-batch lookup kernels, for
        the transport kernels of other streams (``scone_set_cu_reserve``)."""
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_set_cu_reserve(self._h, int(n_reserved)), "scone_set_cu_reserve")

    def lookup_stream(self) -> Optional["torch.cuda.Stream"]:
        """The handle's CU-masked stream as a torch stream (None without a reserve): a loop queued on it -- ``with
        torch.cuda.stream(table.lookup_stream()):`` -- has its lookups launched there directly, without the two cross-stream
        events of the transparent form.  The handle uses it until the next :meth:`set_cu_reserve`; the stream object itself is
        never destroyed by the library (PyTorch's allocator keeps the streams a tensor was recorded on), only retired and re-used."""
        p = C.c_void_p()
        self._check(L.lib().scone_lookup_stream(self._h, C.byref(p)), "scone_lookup_stream")
        return torch.cuda.ExternalStream(p.value, device=self.device) if p.value else None

    def streams_overlap(self, a: "torch.cuda.Stream", b: "torch.cuda.Stream") -> bool:
        """Do kernels queued on ``b`` start while a kernel queued before them on ``a`` is still running (i.e. do the two streams
        sit on different hardware queues)?  Synchronises both streams (``scone_streams_overlap``)."""
        v = C.c_int32(0)
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_streams_overlap(self._h, a.cuda_stream, b.cuda_stream, C.byref(v)), "scone_streams_overlap")
        return bool(v.value)

    def pick_side_stream(self, candidates: int = 6) -> "torch.cuda.Stream":
        """A new stream whose kernels run BESIDE those of the current stream: the first of ``candidates`` fresh streams that
        passes :meth:`streams_overlap` against the current stream (HIP spreads streams over four hardware queues; a side
        stream that shares the current stream's queue overlaps with nothing).  The first candidate if none passes."""
        cur = torch.cuda.current_stream(self.device)
        made = [torch.cuda.Stream(device=self.device) for _ in range(max(1, candidates))]
        for s in made:
            if self.streams_overlap(cur, s):
                return s
        return made[0]

    def cu_reserve(self) -> Tuple[int, int]:
        """(compute units reserved, compute units of the device)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(L.lib().scone_get_cu_reserve(self._h, C.byref(a), C.byref(b)), "scone_get_cu_reserve")
        return a.value, b.value

    def profile_enable(self, enable: bool = True) -> None:
        self._check(L.lib().scone_profile_enable(self._h, int(enable)), "scone_profile_enable")

    def profile_read(self, reset: bool = True) -> Tuple[int, float]:
        """(launches, total milliseconds) of the gather/reduce kernel since the last reset."""
        n, ms = C.c_uint64(0), C.c_double(0.0)
        self._check(L.lib().scone_profile_read(self._h, C.byref(n), C.byref(ms), int(reset)), "scone_profile_read")
        return n.value, ms.value

    def profile_samples(self) -> np.ndarray:
        """Milliseconds of every timed launch since the last reset (launch order)."""
        n = C.c_uint64(0)
        self._check(L.lib().scone_profile_samples(self._h, None, 0, C.byref(n)), "scone_profile_samples")
        out = np.zeros(n.value, dtype=np.float32)
        if n.value:
            self._check(L.lib().scone_profile_samples(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n.value,
                                                      C.byref(n)), "scone_profile_samples")
        return out[:n.value]

    def embed_partial(self, tok: torch.Tensor,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """fp32 sums over the rows this shard owns ``[B*T, d]`` and the full hit counts ``[B*T]`` (``scone_embed_partial``);
        ``out=(sums, counts)`` writes into the caller's buffers."""
        tok = self._tok(tok)
        B, T = tok.shape
        if out is None:
            partial = torch.empty((B * T, self.dim), dtype=torch.float32, device=self.device)
            counts = torch.empty(B * T, dtype=torch.int32, device=self.device)
        else:
            partial, counts = out
            assert partial.is_cuda and partial.is_contiguous() and partial.dtype == torch.float32 and partial.shape == (B * T, self.dim)
            assert counts.is_cuda and counts.is_contiguous() and counts.dtype == torch.int32 and counts.shape == (B * T,)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_embed_partial(self._h, _ptr(tok), B, T, _ptr(partial), _ptr(counts), _stream())
        self._check(rc, "scone_embed_partial")
        return partial, counts

    # -- row exchange between shards (scone_shard_*) ---------------------------------
    def shard_set_head(self, n_head: int) -> None:
        """Keep global rows ``[0, n_head)`` on this shard as well (replicated head: never sent between shards)."""
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_shard_set_head(self._h, int(n_head)), "scone_shard_set_head")
        self.n_head = min(int(n_head), self.n_rows)

    def shard_head_store_f32(self, rows: torch.Tensor, row0: int = 0) -> None:
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {tuple(rows.shape)}")
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_head_store_f32(self._h, _ptr(rows), int(row0), rows.shape[0], _stream())
            torch.cuda.current_stream().synchronize()          # `rows` may be a temporary
        self._check(rc, "scone_shard_head_store_f32")

    def shard_record_bytes(self) -> int:
        n = C.c_uint64(0)
        self._check(L.lib().scone_shard_record_bytes(self._h, C.byref(n)), "scone_shard_record_bytes")
        return n.value

    # -- all-gather form: one record per distinct row (scone_shard_gather_*) -------------
    def shard_gather_plan(self, tok: torch.Tensor) -> int:
        """Number of records this shard contributes: the distinct rows it owns (outside the replicated head) that
        the batch references (synchronises)."""
        tok = self._tok(tok)
        B, T = tok.shape
        n = C.c_uint64(0)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_plan(self._h, _ptr(tok), B, T, C.byref(n), _stream())
        self._check(rc, "scone_shard_gather_plan")
        self._shard_keepalive = (tok,)
        return n.value

    def shard_gather_pack(self, n_records: int) -> torch.Tensor:
        """uint8 ``[n_records, record_bytes]``: ``[row payload | scales | row id]`` per claimed row."""
        buf = torch.empty((int(n_records), self.shard_record_bytes()), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_pack(self._h, _ptr(buf), _stream())
        self._check(rc, "scone_shard_gather_pack")
        return buf

    def shard_select_slot(self, slot: int) -> None:
        """Plan slot 0 .. 3 for the scone_shard_gather_* calls that follow (host-side switch): the receiver-side state of a
        planned batch exists once per slot, so batches b + 1, b + 2 can be planned and exchanged while batch b is being reduced."""
        self._check(L.lib().scone_shard_select_slot(self._h, int(slot)), "scone_shard_select_slot")

    def shard_gather_plan_chunks(self, tok: torch.Tensor, n_chunks: int, dedup_across_chunks: bool = True) -> list:
        """Chunked plan: ``ends[c]`` = records this shard contributes to chunks ``0..c`` of the batch (chunk c = sequences
        ``[c * ceil(B / n_chunks), ...)``).  ``dedup_across_chunks=True`` (all-gather form): a row claimed by an earlier chunk
        is not claimed again; ``False`` (slice exchange, ``n_chunks = world``): every chunk lists each distinct row it
        references (synchronises)."""
        tok = self._tok(tok)
        B, T = tok.shape
        ends = (C.c_uint64 * 64)()
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_plan_chunks(self._h, _ptr(tok), B, T, int(n_chunks), int(bool(dedup_across_chunks)),
                                                        ends, _stream())
        self._check(rc, "scone_shard_gather_plan_chunks")
        self._shard_keepalive = (tok,)
        return [int(e) for e in ends[:n_chunks]]

    def ell_width(self) -> int:
        """int32 words of one token's list record (8 for max_n <= 3, 16 for max_n = 4)."""
        n = C.c_uint32(0)
        self._check(L.lib().scone_ell_width(self._h, C.byref(n)), "scone_ell_width")
        return n.value

    def shard_gather_match(self, tok: torch.Tensor, seq_begin: int, seq_end: int, out_ell: torch.Tensor) -> None:
        """List records of sequences ``[seq_begin, seq_end)`` of the batch (matched against ALL rows) into
        ``out_ell[:(seq_end - seq_begin) * T]`` (int32 ``[., ell_width()]``): this rank's share of a plan whose match is
        sharded over the ranks."""
        tok = self._tok(tok)
        B, T = tok.shape
        n = (seq_end - seq_begin) * T
        assert out_ell.is_cuda and out_ell.is_contiguous() and out_ell.dtype == torch.int32 and out_ell.numel() >= n * self.ell_width()
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_match(self._h, _ptr(tok), B, T, int(seq_begin), int(seq_end), _ptr(out_ell), _stream())
        self._check(rc, "scone_shard_gather_match")
        self._shard_keepalive = (tok, out_ell)

    def shard_gather_plan_ell(self, ell: torch.Tensor, B: int, T: int, n_chunks: int, dedup_across_chunks: bool = True) -> list:
        """The claim passes of :meth:`shard_gather_plan_chunks` over list records the caller gathered (``ell`` int32
        ``[>= B * T, ell_width()]``, token order); ``ell`` is borrowed by the plan slot until the batch has been reduced
        (synchronises)."""
        assert ell.is_cuda and ell.is_contiguous() and ell.dtype == torch.int32 and ell.numel() >= B * T * self.ell_width()
        ends = (C.c_uint64 * 64)()
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_plan_ell(self._h, _ptr(ell), int(B), int(T), int(n_chunks),
                                                     int(bool(dedup_across_chunks)), ends, _stream())
        self._check(rc, "scone_shard_gather_plan_ell")
        self._shard_keepalive = (ell,)
        return [int(e) for e in ends[:n_chunks]]

    def shard_gather_pack_range(self, first: int, count: int, out: torch.Tensor) -> None:
        """Records ``[first, first + count)`` of the plan into ``out[:count]``; the rest of ``out`` becomes padding."""
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.shape[1] == self.shard_record_bytes()
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_pack_range(self._h, int(first), int(count), int(out.shape[0] - count), _ptr(out),
                                                       _stream())
        self._check(rc, "scone_shard_gather_pack_range")

    def shard_gather_add_records(self, records: torch.Tensor, record0: int, n_records: int) -> None:
        """Receiver: records ``[record0, record0 + n_records)`` of the gathered buffer ``records [n_total, record_bytes]``
        join the row map (``record0 == 0`` starts a new exchange)."""
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.uint8
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_add_records(self._h, _ptr(records), int(record0), int(n_records),
                                                        records.shape[0], _stream())
        self._check(rc, "scone_shard_gather_add_records")

    def shard_gather_remap_range(self, seq_begin: int, seq_end: int) -> None:
        """Rewrite the lists of sequences ``[seq_begin, seq_end)`` of the planned batch to record numbers on the current
        stream (their rows must have been added); :meth:`shard_gather_embed_range` then only launches the lookup."""
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_remap_range(self._h, int(seq_begin), int(seq_end), _stream())
        self._check(rc, "scone_shard_gather_remap_range")

    def shard_gather_embed_range(self, tok: torch.Tensor, seq_begin: int, seq_end: int, records: torch.Tensor,
                                 out: torch.Tensor, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                                 position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
                                 out_is_slice: bool = False) -> None:
        """Sequences ``[seq_begin, seq_end)`` of the planned batch into their place in ``out [B*T, d]`` -- or, with
        ``out_is_slice``, into ``out [>= (seq_end - seq_begin) * T, d]`` whose first row is sequence ``seq_begin``."""
        tok = self._tok(tok)
        B, T = tok.shape
        n_out = (seq_end - seq_begin) * T if out_is_slice else B * T
        assert out.is_cuda and out.is_contiguous() and out.numel() >= n_out * self.dim
        if position_ids is not None:                      # (a host / int64 tensor handed to the kernel as it is would be read as garbage)
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).expand(B, T).contiguous()
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_embed_range(self._h, _ptr(tok), B, T, int(seq_begin), int(seq_end), _ptr(records),
                                                        records.shape[0], _ptr(wte), 0 if wte is None else wte.shape[0],
                                                        _ptr(wpe), 0 if wpe is None else wpe.shape[0], _ptr(position_ids),
                                                        _REDUCE[reduce], _ptr(out), int(seq_begin) * T if out_is_slice else 0,
                                                        _DT[out.dtype], _stream())
        self._shard_keepalive = (records, tok, position_ids, wte, wpe, out)
        self._check(rc, "scone_shard_gather_embed_range")

    # -- all-gather form with columns on the wire (scone_shard_cols_*) ---------------------------------
    @staticmethod
    def cols_frag_slots(count: int) -> int:
        """u64 slots of the sender's hash fragment for ``count`` rows (both ends derive it from the exchanged counts)."""
        n = C.c_uint64(0)
        L.lib().scone_shard_cols_frag_slots(int(count), C.byref(n))
        return n.value

    def shard_cols_pack(self, first: int, count: int, rows_out: torch.Tensor, scales_out: Optional[torch.Tensor],
                        frag_out: torch.Tensor) -> None:
        """Records ``[first, first + count)`` of the plan as columns: payload rows ``uint8 [count, payload_bytes]``, scales
        ``uint8 [count, scale bytes]`` (None for fp32 / fp16 tables) and the hash fragment ``int64 [slots]`` (cleared and
        filled: row id -> position)."""
        assert rows_out.is_cuda and rows_out.is_contiguous() and rows_out.numel() >= count * self.payload_bytes()
        assert frag_out.is_cuda and frag_out.is_contiguous() and frag_out.dtype == torch.int64
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_cols_pack(self._h, int(first), int(count), _ptr(rows_out), _ptr(scales_out), _ptr(frag_out),
                                               frag_out.numel(), _stream())
        self._check(rc, "scone_shard_cols_pack")

    def shard_gather_plan_async(self, tok: torch.Tensor) -> None:
        """The one-chunk plan without the host round trip: match + claim pass are enqueued, the count stays on the device
        (pack with :meth:`shard_cols_pack_cap`)."""
        tok = self._tok(tok)
        B, T = tok.shape
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_plan_async(self._h, _ptr(tok), B, T, _stream())
        self._check(rc, "scone_shard_gather_plan_async")
        self._shard_keepalive = (tok,)

    def shard_gather_plan_ell_async(self, ell: torch.Tensor, B: int, T: int) -> None:
        """:meth:`shard_gather_plan_ell` (one chunk) without the host round trip."""
        assert ell.is_cuda and ell.is_contiguous() and ell.dtype == torch.int32 and ell.numel() >= B * T * self.ell_width()
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_plan_ell_async(self._h, _ptr(ell), int(B), int(T), _stream())
        self._check(rc, "scone_shard_gather_plan_ell_async")
        self._shard_keepalive = (ell,)

    def shard_cols_pack_cap(self, cap_rows: int, rows_out: torch.Tensor, scales_out: Optional[torch.Tensor], frag_out: torch.Tensor,
                            header_out: torch.Tensor) -> None:
        """The pack of a sync-free plan: up to ``cap_rows`` claimed rows as columns, the count read on the device;
        ``header_out`` (int64 ``[2]``, device) = (rows claimed, 1 if more than ``cap_rows``)."""
        assert rows_out.is_cuda and rows_out.is_contiguous() and rows_out.numel() >= cap_rows * self.payload_bytes()
        assert frag_out.is_cuda and frag_out.is_contiguous() and frag_out.dtype == torch.int64
        assert header_out.is_cuda and header_out.is_contiguous() and header_out.dtype == torch.int64 and header_out.numel() >= 2
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_cols_pack_cap(self._h, int(cap_rows), _ptr(rows_out), _ptr(scales_out), _ptr(frag_out),
                                                   frag_out.numel(), _ptr(header_out), _stream())
        self._check(rc, "scone_shard_cols_pack_cap")

    def shard_cols_build_frag(self, ids: torch.Tensor, frag_out: torch.Tensor) -> None:
        """The fragment of an arbitrary id list (position = index in the list)."""
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        assert frag_out.is_cuda and frag_out.is_contiguous() and frag_out.dtype == torch.int64
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_cols_build_frag(self._h, _ptr(ids), ids.numel(), _ptr(frag_out), frag_out.numel(), _stream())
            torch.cuda.current_stream().synchronize()              # `ids` may be a temporary
        self._check(rc, "scone_shard_cols_build_frag")

    def scale_bytes(self) -> int:
        return (1 if self.fmt == L.FMT_MXFP4 else 2) * self.scales_per_row()      # E8M0 bytes; fp16 otherwise

    def shard_head_version(self) -> int:
        """Counter bumped by every change of the replicated head (buffers that start with the head's scales are refilled)."""
        v = C.c_uint64(0)
        self._check(L.lib().scone_shard_head_version(self._h, C.byref(v)), "scone_shard_head_version")
        return v.value

    def shard_head_scales_into(self, scales_full: torch.Tensor) -> None:
        """The replicated head's scales into the front of a ``[n_head + capacity, scale bytes]`` buffer."""
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_head_scales(self._h, _ptr(scales_full), _stream())
        self._check(rc, "scone_shard_head_scales")

    def shard_cols_embed(self, tok: torch.Tensor, seq_begin: int, seq_end: int, rows: torch.Tensor, n_total: int,
                         scales_full: Optional[torch.Tensor], frags: torch.Tensor, frag_off, frag_slots, rec_base,
                         out: torch.Tensor, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                         position_ids: Optional[torch.Tensor] = None, reduce: str = "mean", row_lo=None) -> None:
        """Sequences ``[seq_begin, seq_end)`` of the planned batch into their place in ``out [B*T, d]`` out of ``[replicated
        head | rows]`` (payload stride), lists resolved through the owners' fragments.  ``row_lo``: the owners' row ranges,
        ``len(frag_off) + 1`` ascending values from 0 to ``n_rows`` (None: the floor partition of ``distributed.shard_range``)."""
        tok = self._tok(tok)
        B, T = tok.shape
        W = len(frag_off)
        assert out.is_cuda and out.is_contiguous() and out.numel() >= B * T * self.dim
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).expand(B, T).contiguous()
        arr = lambda v: (C.c_uint64 * 65)(*[int(x) for x in v])
        if row_lo is not None and len(row_lo) != W + 1:
            raise ValueError("row_lo needs len(frag_off) + 1 entries")
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_cols_embed(self._h, _ptr(tok), B, T, int(seq_begin), int(seq_end), _ptr(rows), int(n_total),
                                                _ptr(scales_full), _ptr(frags), frags.numel(), arr(frag_off), arr(frag_slots),
                                                arr(rec_base), None if row_lo is None else arr(row_lo), W,
                                                _ptr(wte), 0 if wte is None else wte.shape[0], _ptr(wpe),
                                                0 if wpe is None else wpe.shape[0], _ptr(position_ids), _REDUCE[reduce], _ptr(out),
                                                0, _DT[out.dtype], _stream())
        self._shard_keepalive = (rows, scales_full, frags, tok, position_ids, wte, wpe, out)
        self._check(rc, "scone_shard_cols_embed")

    # -- peer-mapped buffers, interprocess events, copy-engine pushes (scone_ipc_*: the "sdma" transport) ------------
    def ipc_alloc(self, nbytes: int) -> Tuple[int, bytes]:
        """Device memory of this handle's device + its 64-byte interprocess handle: ``(pointer, handle)``."""
        p, hb = C.c_void_p(), C.create_string_buffer(64)
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_ipc_alloc(self._h, int(nbytes), C.byref(p), hb), "scone_ipc_alloc")
        return p.value, hb.raw

    def ipc_free(self, ptr: int) -> None:
        self._check(L.lib().scone_ipc_free(self._h, C.c_void_p(ptr)), "scone_ipc_free")

    def ipc_open(self, handle: bytes) -> int:
        p = C.c_void_p()
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_ipc_open(self._h, C.c_char_p(handle), C.byref(p)), "scone_ipc_open")
        return p.value

    def ipc_close(self, ptr: int) -> None:
        self._check(L.lib().scone_ipc_close(self._h, C.c_void_p(ptr)), "scone_ipc_close")

    def ipc_event_create(self) -> Tuple[int, bytes]:
        e, hb = C.c_void_p(), C.create_string_buffer(64)
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_ipc_event_create(self._h, C.byref(e), hb), "scone_ipc_event_create")
        return e.value, hb.raw

    def ipc_event_open(self, handle: bytes) -> int:
        e = C.c_void_p()
        with torch.cuda.device(self.device):
            self._check(L.lib().scone_ipc_event_open(self._h, C.c_char_p(handle), C.byref(e)), "scone_ipc_event_open")
        return e.value

    def ipc_event_destroy(self, event: int) -> None:
        self._check(L.lib().scone_ipc_event_destroy(self._h, C.c_void_p(event)), "scone_ipc_event_destroy")

    # (the stream is torch's current stream of THE TABLE'S device, whatever device is current in the caller)
    def ipc_event_record(self, event: int) -> None:
        with torch.cuda.device(self.device):
            rc = L.lib().scone_ipc_event_record(self._h, C.c_void_p(event), _stream())
        self._check(rc, "scone_ipc_event_record")

    def ipc_event_wait(self, event: int) -> None:
        with torch.cuda.device(self.device):
            rc = L.lib().scone_ipc_event_wait(self._h, C.c_void_p(event), _stream())
        self._check(rc, "scone_ipc_event_wait")

    def ipc_push(self, dst_ptr: int, src_ptr: int, nbytes: int, copy_engine: bool = True) -> None:
        """``nbytes`` from ``src_ptr`` (this device) to ``dst_ptr`` (possibly a peer's mapped buffer) on the current stream."""
        with torch.cuda.device(self.device):
            rc = L.lib().scone_ipc_push(self._h, C.c_void_p(dst_ptr), C.c_void_p(src_ptr), int(nbytes), int(bool(copy_engine)), _stream())
        self._check(rc, "scone_ipc_push")

    def ipc_tensor(self, ptr: int, nbytes: int) -> torch.Tensor:
        """A uint8 tensor over raw device memory of this handle's device (no ownership: keep the allocation alive)."""
        class _Raw:
            pass
        raw = _Raw()
        raw.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        with torch.cuda.device(self.device):
            return torch.as_tensor(raw, device=self.device)

    def shard_gather_embed(self, tok: torch.Tensor, records: torch.Tensor, wte: Optional[torch.Tensor] = None,
                           wpe: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                           reduce: str = "mean", out_dtype: torch.dtype = torch.float32,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The whole batch ``[B*T, d]`` out of ``[replicated head | records of every shard]``."""
        tok = self._tok(tok)
        B, T = tok.shape
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).expand(B, T).contiguous()
        if out is None:
            out = torch.empty((B * T, self.dim), dtype=out_dtype, device=self.device)
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.uint8
        with torch.cuda.device(self.device):
            rc = L.lib().scone_shard_gather_embed(self._h, _ptr(tok), B, T, _ptr(records), records.shape[0], _ptr(wte),
                                                  0 if wte is None else wte.shape[0], _ptr(wpe),
                                                  0 if wpe is None else wpe.shape[0], _ptr(position_ids), _REDUCE[reduce],
                                                  _ptr(out), _DT[out_dtype], _stream())
        self._shard_keepalive = (records, tok, position_ids, wte, wpe)       # read in place after the call returns
        self._check(rc, "scone_shard_gather_embed")
        return out

    def finalize(self, sums: torch.Tensor, counts: torch.Tensor, tok: torch.Tensor, tok_begin: int, tok_end: int,
                 wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                 position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
                 out_dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        tok = self._tok(tok)
        B, T = tok.shape
        n = tok_end - tok_begin
        sums = sums.to(device=self.device, dtype=torch.float32).contiguous()
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        assert sums.shape == (n, self.dim) and counts.shape == (n,)
        if position_ids is not None:
            position_ids = position_ids.to(device=self.device, dtype=torch.int32).expand(B, T).contiguous()
        if out is None:
            out = torch.empty((n, self.dim), dtype=out_dtype, device=self.device)
        else:
            assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and out.shape == (n, self.dim)
        with torch.cuda.device(self.device):
            rc = L.lib().scone_finalize(self._h, _ptr(sums), _ptr(counts), _ptr(tok), B, T, int(tok_begin),
                                        int(tok_end), _ptr(wte), 0 if wte is None else wte.shape[0], _ptr(wpe),
                                        0 if wpe is None else wpe.shape[0], _ptr(position_ids), _REDUCE[reduce],
                                        _ptr(out), _DT[out_dtype], _stream())
        self._check(rc, "scone_finalize")
        return out
