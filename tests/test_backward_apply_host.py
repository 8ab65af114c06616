"""The backward applied in place, without a GPU: the argument types of `scone_backward_apply_lean` in the header and in the
ctypes binding, and the Python surface -- `BackwardPlan.apply_lean`, `FGramOptimizer(fused_backward=...)` -- whose defaults must
leave every existing call as it was."""

import ctypes as C
import inspect
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scone_hip.h")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/scone_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_binding_agree_on_the_argument_types():
    from scone_amd import _lib
    args = _declaration("scone_backward_apply_lean")
    assert args == ["scone_handle *h", "scone_bwd_plan *plan", "const void *d_grad_out", "int32_t grad_dtype", "int32_t reduce",
                    "const scone_lean_cfg *cfg", "float *d_row_state", "scone_stream_t stream"]
    restype, argtypes = _lib.SIGNATURES["scone_backward_apply_lean"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_lib.LeanCfg), C.c_void_p, C.c_void_p]
    fn = _lib.lib().scone_backward_apply_lean                     # the symbol is exported, with these types bound
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert _lib.lib().scone_abi_version() == _lib.ABI_VERSION, "appended: the ABI version is unchanged"


def test_a_null_handle_is_refused_without_a_gpu():
    from scone_amd import _lib
    assert _lib.lib().scone_backward_apply_lean(None, None, None, 0, 0, None, None, None) == _lib.EINVAL


def test_python_surface_and_defaults():
    from scone_amd import FGramOptimizer
    from scone_amd.hip_backend import APPLY_LEAN_MAX_DIM, BackwardPlan
    sig = inspect.signature(BackwardPlan.apply_lean)
    names = list(sig.parameters)
    assert names[:3] == ["self", "grad_out", "reduce"]
    keyword_only = [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert keyword_only == ["kind", "lr", "row_state", "eps", "weight_decay", "grad_scale", "rounding", "seed", "step"]
    assert sig.parameters["row_state"].default is None and sig.parameters["rounding"].default == "nearest"
    assert sig.parameters["grad_scale"].default == 1.0 and sig.parameters["weight_decay"].default == 0.0
    assert APPLY_LEAN_MAX_DIM == 4096
    fused = inspect.signature(FGramOptimizer.__init__).parameters["fused_backward"]
    assert fused.default is False, "the default road is the two calls"
    assert "two updates" in FGramOptimizer.__doc__.lower()
