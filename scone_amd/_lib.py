"""ctypes binding of libscone_hip.so (include/scone_hip.h).

The library is the product path: there is no CPU fallback.  Importing this module
is cheap; :func:`lib` loads the shared object on first use and raises
``RuntimeError`` if it has not been built (``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C scone_amd/csrc -j8``).
"""

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCONE_HIP_LIB: alternative build of the same library (A/B kernel experiments)
LIB_PATH = os.environ.get("SCONE_HIP_LIB") or os.path.join(_HERE, "csrc", "libscone_hip.so")

ABI_VERSION = 2

FMT_F32, FMT_F16, FMT_I8, FMT_I4, FMT_BF16, FMT_MXFP4 = 0, 1, 2, 3, 4, 5
PLACE_HBM, PLACE_PINNED_HOST = 0, 1
REDUCE_MEAN, REDUCE_SUM = 0, 1
MODE_COVER, MODE_LONGEST_SUFFIX = 0, 1
DT_F32, DT_F16, DT_BF16 = 0, 1, 2

OK, ESTATE, EHIP, ENOMEM, ENODEV, EINVAL, ERANGE = 0, -1, -5, -12, -19, -22, -34

ST_BAD_TOKEN, ST_BAD_ID, ST_INDEX_FULL, ST_STAGE_OVERFLOW, ST_ROWS_OVERFLOW = 1, 2, 4, 8, 16


class SconeCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("max_n", C.c_int32),
        ("dim", C.c_int32),
        ("table_fmt", C.c_int32),
        ("placement", C.c_int32),
        ("n_rows", C.c_uint64),
        ("row_begin", C.c_uint64),
        ("row_end", C.c_uint64),
        ("index_capacity", C.c_uint64),
        ("hot_rows", C.c_uint64),
        ("lookup_mode", C.c_uint32),
        ("stage_tokens", C.c_uint32),
        ("cache_rows", C.c_uint64),
    ]


OPT_SGD, OPT_ADAGRAD, OPT_ADAM = 0, 1, 2


class OptCfg(C.Structure):
    """``scone_opt_cfg``: the hyper-parameters of one optimizer step, in double."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("kind", C.c_int32),
        ("lr", C.c_double),
        ("beta1", C.c_double),
        ("beta2", C.c_double),
        ("eps", C.c_double),
        ("weight_decay", C.c_double),
        ("grad_scale", C.c_double),
        ("step", C.c_int64),
    ]


class OptScalars(C.Structure):
    """``scone_opt_scalars``: the fp32 values the kernel computes with (``scone_opt_scalars_of``)."""
    _fields_ = [(name, C.c_float) for name in ("alpha", "b1", "b2", "c1", "c2", "eps", "decay", "gscale")]


LEAN_SGD, LEAN_ROWWISE_ADAGRAD = 0, 1
ROUND_NEAREST, ROUND_STOCHASTIC = 0, 1


class LeanCfg(C.Structure):
    """``scone_lean_cfg``: the hyper-parameters of one lean optimizer step; ``seed`` / ``step`` feed the random bits only."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("kind", C.c_int32),
        ("rounding", C.c_int32),
        ("reserved", C.c_int32),
        ("lr", C.c_double),
        ("eps", C.c_double),
        ("weight_decay", C.c_double),
        ("grad_scale", C.c_double),
        ("seed", C.c_uint64),
        ("step", C.c_int64),
    ]


class SconeGradCtl(C.Structure):
    """``scone_grad_ctl``: the 24 device bytes ``scone_grad_ctl_set`` writes and the ``_ctl`` optimizer steps read."""
    _fields_ = [
        ("sqnorm", C.c_double),
        ("norm", C.c_float),
        ("coef", C.c_float),
        ("skip", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SconeOptHyper(C.Structure):
    """``scone_opt_hyper``: the 104 device bytes ``scone_opt_hyper_init`` writes, ``scone_opt_hyper_advance`` advances and the
    ``_dh`` steps read (include/scone_hip.h, "optimizer hyper-parameters on the device")."""
    _fields_ = [
        ("lr", C.c_double),
        ("beta1", C.c_double),
        ("beta2", C.c_double),
        ("eps", C.c_double),
        ("weight_decay", C.c_double),
        ("grad_scale", C.c_double),
        ("seed", C.c_uint64),
        ("step", C.c_int64),
        ("sc", OptScalars),
        ("applied", C.c_uint32),
        ("bad", C.c_uint32),
    ]


class SconeLiveRows(C.Structure):
    """``scone_live_rows``: a batch's live f-gram rows as ``scone_embed_rows`` takes them (include/scone_hip.h, "the fused
    lookup over a batch's LIVE rows")."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dtype", C.c_int32),
        ("d_row_ids", C.c_void_p),
        ("d_rows", C.c_void_p),
        ("n", C.c_uint64),
        ("d_n", C.c_void_p),
    ]


LIVE_ROWS_MAX = 2**31 - 1   # the most rows a scone_live_rows may list

_P = C.c_void_p
_I32, _I64, _U32, _U64 = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64


def grad_sqnorm_scratch(n: int) -> int:
    """``scone_grad_sqnorm_scratch``: the doubles ``scone_grad_sqnorm`` needs as scratch for ``n`` rows.  Runs without a GPU."""
    out = _U64(0)
    if lib().scone_grad_sqnorm_scratch(int(n), C.byref(out)) != OK:
        raise ValueError("scone_grad_sqnorm_scratch refused its arguments")
    return int(out.value)


def grad_merge_scratch(n_a: int, n_b: int) -> int:
    """``scone_grad_merge_scratch``: the bytes ``scone_grad_merge_map`` needs as scratch.  Runs without a GPU."""
    out = _U64(0)
    if lib().scone_grad_merge_scratch(int(n_a), int(n_b), C.byref(out)) != OK:
        raise ValueError("scone_grad_merge_scratch refused its arguments")
    return int(out.value)


def backward_ctx_partial_slots(max_refs: int) -> int:
    """``scone_backward_ctx_partial_slots``: the most partial slots a plan of ``max_refs`` references can have,
    ``floor(2 R / (C + 1))``.  Runs without a GPU."""
    out = _U64(0)
    if lib().scone_backward_ctx_partial_slots(int(max_refs), C.byref(out)) != OK:
        raise ValueError("scone_backward_ctx_partial_slots refused its arguments (max_refs must be below 2^32)")
    return int(out.value)


def backward_wpe_scratch(B: int, T: int, d: int) -> int:
    """``scone_backward_wpe_scratch``: the bytes of scratch ``scone_backward_wpe`` needs for a rectangle ``[B, T]`` at ``d``.
    Runs without a GPU."""
    out = _U64(0)
    if lib().scone_backward_wpe_scratch(int(B), int(T), int(d), C.byref(out)) != OK:
        raise ValueError("scone_backward_wpe_scratch refused its arguments")
    return int(out.value)


# name -> (restype, argtypes); must list every symbol include/scone_hip.h declares
SIGNATURES = {
    "scone_abi_version": (C.c_int, []),
    "scone_strerror": (C.c_char_p, [C.c_int]),
    "scone_create": (C.c_int, [C.POINTER(SconeCfg), C.POINTER(_P)]),
    "scone_destroy": (None, [_P]),
    "scone_last_error": (C.c_char_p, [_P]),
    "scone_status": (C.c_int, [_P, C.POINTER(_U32), _P]),
    "scone_stage_counters": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64)]),
    "scone_index_build": (C.c_int, [_P, _P, _P, _U64, _U64]),
    "scone_index_build_device": (C.c_int, [_P, _P, _P, _U64, _U64, _P]),
    "scone_index_stats": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64)]),
    "scone_index_blob_sizes": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64)]),
    "scone_index_export": (C.c_int, [_P, _P, _P, _P, C.POINTER(_U64)]),
    "scone_index_import": (C.c_int, [_P, _P, _P, _P, _U64]),
    "scone_fit": (C.c_int, [_I32, _P, _I64, _P, _I64, _I32, _U32, _U64, _P, _P, _P, _U64, C.POINTER(_U64),
                            C.POINTER(_U64), _P]),
    "scone_fit_create": (C.c_int, [_I32, _I32, _U64, C.POINTER(_P)]),
    "scone_fit_destroy": (None, [_P]),
    "scone_fit_update": (C.c_int, [_P, _P, _I64, _P, _I64, _U64, _P]),
    "scone_fit_stats": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64)]),
    "scone_fit_finalize": (C.c_int, [_P, _U32, _U64, _P, _P, _P, _U64, C.POINTER(_U64), _P]),
    "scone_fit_export": (C.c_int, [_P, _P, _P, _P, _P, _U64, C.POINTER(_U64), _P]),
    "scone_fit_merge": (C.c_int, [_P, _P, _P, _P, _P, _U64, _P]),
    "scone_fit_partition": (C.c_int, [_P, _P, _U64, _I32, _U32, _P]),
    "scone_fit_update_part": (C.c_int, [_P, _P, _I64, _P, _I64, _U64, _U32, _U32, _P]),
    "scone_fit_finalize_seq": (C.c_int, [_P, _U32, _U64, _P, _P, _P, _P, _U64, C.POINTER(_U64), _P]),
    "scone_table_upload": (C.c_int, [_P, _P, _P, _U64, _U64, C.c_int, _P]),
    "scone_table_download": (C.c_int, [_P, _P, _P, _U64, _U64, C.c_int, _P]),
    "scone_table_store_f32": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "scone_table_store_f32_ids": (C.c_int, [_P, _P, _P, _U64, _P]),
    "scone_table_fill_synthetic": (C.c_int, [_P, _U32, C.c_float, _P]),
    "scone_table_gather_rows": (C.c_int, [_P, _P, _U64, _P, _P]),
    "scone_match": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "scone_match_csr": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _I64, C.POINTER(_I64), _P]),
    "scone_gather_reduce": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed": (C.c_int, [_P, _P, _I32, _I32, _P, _I64, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed_varlen": (C.c_int, [_P, _P, _P, _I32, _I64, _P, _I64, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed_base": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed_base_varlen": (C.c_int, [_P, _P, _P, _I32, _I64, _P, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed_select": (C.c_int, [_P, _P, _I64, _I32, _P, _I32, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed_rows": (C.c_int, [_P, C.POINTER(SconeLiveRows), _P, _I32, _I32, _P, _I64, _P, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_embed_rows_varlen": (C.c_int, [_P, C.POINTER(SconeLiveRows), _P, _P, _I32, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _P,
                                          _I32, _P]),
    "scone_embed_prefetch": (C.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "scone_reserve": (C.c_int, [_P, _I64]),
    "scone_set_cu_reserve": (C.c_int, [_P, _I32]),
    "scone_get_cu_reserve": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_I32)]),
    "scone_lookup_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "scone_streams_overlap": (C.c_int, [_P, _P, _P, C.POINTER(_I32)]),
    "scone_profile_enable": (C.c_int, [_P, C.c_int]),
    "scone_profile_read": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(C.c_double), C.c_int]),
    "scone_profile_samples": (C.c_int, [_P, C.POINTER(C.c_float), _U64, C.POINTER(_U64)]),
    "scone_embed_partial": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _P]),
    "scone_shard_gather_plan": (C.c_int, [_P, _P, _I32, _I32, C.POINTER(_U64), _P]),
    "scone_shard_gather_pack": (C.c_int, [_P, _P, _P]),
    "scone_shard_gather_embed": (C.c_int, [_P, _P, _I32, _I32, _P, _U64, _P, _I64, _P, _I64, _P, _I32, _P, _I32, _P]),
    "scone_shard_select_slot": (C.c_int, [_P, _I32]),
    "scone_shard_gather_plan_chunks": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, C.POINTER(_U64), _P]),
    "scone_ell_width": (C.c_int, [_P, C.POINTER(_U32)]),
    "scone_shard_gather_match": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "scone_shard_gather_plan_ell": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, C.POINTER(_U64), _P]),
    "scone_shard_gather_pack_range": (C.c_int, [_P, _U64, _U64, _U64, _P, _P]),
    "scone_shard_gather_add_records": (C.c_int, [_P, _P, _U64, _U64, _U64, _P]),
    "scone_shard_gather_remap_range": (C.c_int, [_P, _I32, _I32, _P]),
    "scone_shard_gather_embed_range": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, _U64, _P, _I64, _P, _I64, _P, _I32, _P,
                                                 _I64, _I32, _P]),
    "scone_shard_gather_plan_async": (C.c_int, [_P, _P, _I32, _I32, _P]),
    "scone_shard_gather_plan_ell_async": (C.c_int, [_P, _P, _I32, _I32, _P]),
    "scone_shard_cols_pack_cap": (C.c_int, [_P, _U64, _P, _P, _P, _U64, _P, _P]),
    "scone_shard_cols_frag_slots": (C.c_int, [_U64, C.POINTER(_U64)]),
    "scone_shard_cols_pack": (C.c_int, [_P, _U64, _U64, _P, _P, _P, _U64, _P]),
    "scone_shard_cols_build_frag": (C.c_int, [_P, _P, _U64, _P, _U64, _P]),
    "scone_shard_head_scales": (C.c_int, [_P, _P, _P]),
    "scone_shard_head_version": (C.c_int, [_P, C.POINTER(_U64)]),
    "scone_shard_cols_embed": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, _U64, _P, _P, _U64, C.POINTER(_U64), C.POINTER(_U64),
                                         C.POINTER(_U64), C.POINTER(_U64), _I32, _P, _I64, _P, _I64, _P, _I32, _P, _I64, _I32, _P]),
    "scone_shard_set_head": (C.c_int, [_P, _U64]),
    "scone_shard_head_store_f32": (C.c_int, [_P, _P, _U64, _U64, _P]),
    "scone_shard_record_bytes": (C.c_int, [_P, C.POINTER(_U64)]),
    "scone_ipc_alloc": (C.c_int, [_P, _U64, C.POINTER(_P), _P]),
    "scone_ipc_free": (C.c_int, [_P, _P]),
    "scone_ipc_open": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "scone_ipc_close": (C.c_int, [_P, _P]),
    "scone_ipc_event_create": (C.c_int, [_P, C.POINTER(_P), _P]),
    "scone_ipc_event_open": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "scone_ipc_event_destroy": (C.c_int, [_P, _P]),
    "scone_ipc_event_record": (C.c_int, [_P, _P, _P]),
    "scone_ipc_event_wait": (C.c_int, [_P, _P, _P]),
    "scone_ipc_push": (C.c_int, [_P, _P, _P, _U64, _I32, _P]),
    "scone_finalize": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I64, _I64, _P, _I64, _P, _I64, _P, _I32, _P,
                                 _I32, _P]),
    "scone_backward_chunk": (C.c_int, []),
    "scone_backward_plan": (C.c_int, [_P, _P, _I32, _I32, C.POINTER(_P), C.POINTER(_U64), C.POINTER(_U64), _P]),
    "scone_backward_plan_varlen": (C.c_int, [_P, _P, _P, _I32, _I64, C.POINTER(_P), C.POINTER(_U64), C.POINTER(_U64), _P]),
    "scone_backward_plan_csr": (C.c_int, [_P, _P, _P, _I64, C.POINTER(_P), C.POINTER(_U64), C.POINTER(_U64), _P]),
    "scone_backward_rows": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _U64, _P]),
    "scone_backward_counts": (C.c_int, [_P, _P, _P, _P]),
    "scone_backward_plan_destroy": (None, [_P]),
    "scone_opt_scalars_of": (C.c_int, [C.POINTER(OptCfg), C.POINTER(OptScalars)]),
    "scone_opt_step": (C.c_int, [_P, C.POINTER(OptCfg), _P, _P, _U64, _P, _P, _P, _P]),
    "scone_lean_scalars_of": (C.c_int, [C.POINTER(LeanCfg), C.POINTER(OptScalars)]),
    "scone_lean_rand16": (_U32, [_U64, _I64, _U64, _U32]),
    "scone_opt_step_lean": (C.c_int, [_P, C.POINTER(LeanCfg), _P, _P, _U64, _P, _P, _P]),
    "scone_backward_apply_lean": (C.c_int, [_P, _P, _P, _I32, _I32, C.POINTER(LeanCfg), _P, _P]),
    "scone_grad_sqnorm_scratch": (C.c_int, [_U64, C.POINTER(_U64)]),
    "scone_grad_sqnorm": (C.c_int, [_P, _P, _U64, _P, _P, _P]),
    "scone_grad_ctl_set": (C.c_int, [_P, _P, _I32, C.c_double, C.c_double, _I32, _P, _P]),
    "scone_opt_step_ctl": (C.c_int, [_P, C.POINTER(OptCfg), _P, _P, _U64, _P, _P, _P, _P, _P]),
    "scone_opt_step_lean_ctl": (C.c_int, [_P, C.POINTER(LeanCfg), _P, _P, _U64, _P, _P, _P, _P]),
    "scone_grad_merge_scratch": (C.c_int, [_U64, _U64, C.POINTER(_U64)]),
    "scone_grad_merge_map": (C.c_int, [_P, _P, _U64, _P, _U64, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_U64), _P]),
    "scone_grad_merge_rows": (C.c_int, [_P, _P, _P, _U64, _P, _P, _P, _P]),
    "scone_backward_row_ids": (C.c_int, [_P, _P, _P, _U64, _P]),
    "scone_backward_rows_acc": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P, _U64, _P, _P, _P]),
    "scone_backward_ctx_partial_slots": (C.c_int, [_U64, C.POINTER(_U64)]),
    "scone_backward_ctx_create": (C.c_int, [_P, _I64, C.POINTER(_P)]),
    "scone_backward_ctx_bytes": (C.c_int, [_P, C.POINTER(_U64)]),
    "scone_backward_ctx_destroy": (None, [_P]),
    "scone_backward_plan_dn": (C.c_int, [_P, _P, _P, _I32, _I32, _P]),
    "scone_backward_plan_varlen_dn": (C.c_int, [_P, _P, _P, _P, _I32, _I64, _P]),
    "scone_backward_ctx_counts": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_U64), _P]),
    "scone_backward_rows_dn": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _U64, _P, _P]),
    "scone_opt_step_dn": (C.c_int, [_P, C.POINTER(OptCfg), _P, _P, _P, _U64, _P, _P, _P, _P, _P]),
    "scone_opt_step_lean_dn": (C.c_int, [_P, C.POINTER(LeanCfg), _P, _P, _P, _U64, _P, _P, _P, _P]),
    "scone_grad_sqnorm_dn": (C.c_int, [_P, _P, _P, _U64, _P, _P, _P]),
    "scone_opt_hyper_scalars_of": (C.c_int, [C.POINTER(OptCfg), C.POINTER(OptScalars)]),
    "scone_opt_hyper_init": (C.c_int, [_P, C.POINTER(OptCfg), _U64, _P, _P]),
    "scone_opt_hyper_advance": (C.c_int, [_P, _I32, _P, _P, _P]),
    "scone_opt_step_dh": (C.c_int, [_P, _I32, _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "scone_opt_step_lean_dh": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _U64, _P, _P, _P, _P, _P]),
    "scone_grad_ctl_set_dh": (C.c_int, [_P, _P, _I32, _P, C.c_double, _I32, _P, _P]),
    "scone_backward_plan_index": (C.c_int, [_P, _P, _I64, _I64, _P, C.POINTER(_P), C.POINTER(_U64), C.POINTER(_U64), _P]),
    "scone_backward_default_positions": (C.c_int, [_P, _P, _I32, _I32, _I64, _P, _P]),
    "scone_backward_wpe_scratch": (C.c_int, [_I32, _I32, _I32, C.POINTER(_U64)]),
    "scone_backward_wpe": (C.c_int, [_P, _P, _I32, _I32, _I32, _I64, _P, _P, _P]),
}

_lock = threading.Lock()
_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the C-ABI library; fail loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"scone_amd: HIP extension not built ({LIB_PATH} is missing). "
                "Build it with `make -C scone_amd/csrc -j8` or __graft_entry__.build(); "
                "there is no CPU fallback for the lookup path.")
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as e:
            raise RuntimeError(f"scone_amd: cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.scone_abi_version() != ABI_VERSION:
            raise RuntimeError("scone_amd: libscone_hip.so ABI version mismatch; rebuild it")
        _lib = handle
        return _lib
