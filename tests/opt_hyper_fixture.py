"""Host model of the optimizer hyper-parameter block (include/scone_hip.h, "optimizer hyper-parameters on the device"), written
from the header's text and independent of the library: the integer power, the eight fp32 scalars and what one
``scone_opt_hyper_advance`` does to the block.

Python floats are IEEE doubles and ``*``, ``-``, ``/`` and ``math.sqrt`` on them are correctly rounded single operations, which is
what the header states for every step; ``np.float32(x)`` of a double is the one rounding to fp32."""

import math

import numpy as np

SGD, ADAGRAD, ADAM = 0, 1, 2
KINDS = {"sgd": SGD, "adagrad": ADAGRAD, "adam": ADAM}
INPUTS = ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")
FIELDS = ("alpha", "b1", "b2", "c1", "c2", "eps", "decay", "gscale")
INT64_MAX = 2 ** 63 - 1


def ipow(b: float, t: int) -> float:
    """r = 1.0; while (t) { if (t & 1) r = r * b; t >>= 1; if (t) b = b * b; }"""
    r = 1.0
    while t:
        if t & 1:
            r = r * b
        t >>= 1
        if t:
            b = b * b
    return r


def f32(x: float) -> np.float32:
    with np.errstate(over="ignore"):
        return np.float32(x)


def scalars(kind, lr, beta1, beta2, eps, weight_decay, grad_scale, t) -> dict:
    """The eight fp32 scalars at step t."""
    kind = KINDS.get(kind, kind)
    alpha = lr
    if kind == ADAM:
        num = lr * math.sqrt(1.0 - ipow(beta2, t))
        den = 1.0 - ipow(beta1, t)
        alpha = num / den if den != 0.0 else math.copysign(math.inf, num) if num != 0.0 else math.nan
    return {"alpha": f32(alpha), "b1": f32(beta1), "b2": f32(beta2), "c1": f32(1.0 - beta1), "c2": f32(1.0 - beta2), "eps": f32(eps),
            "decay": f32(lr * weight_decay), "gscale": f32(grad_scale)}


def init(lr, beta1, beta2, eps, weight_decay, grad_scale, seed, step) -> dict:
    """The block after scone_opt_hyper_init."""
    return {"lr": float(lr), "beta1": float(beta1), "beta2": float(beta2), "eps": float(eps), "weight_decay": float(weight_decay),
            "grad_scale": float(grad_scale), "seed": int(seed), "step": int(step),
            "sc": {name: np.float32(0.0) for name in FIELDS}, "applied": 0, "bad": 0}


def advance(block: dict, kind, skip: bool = False) -> dict:
    """The block after one scone_opt_hyper_advance (skip: d_ctl given and its skip set)."""
    out = dict(block)
    if skip:
        out["applied"] = 0
        return out
    if not all(math.isfinite(block[name]) for name in INPUTS) or block["step"] == INT64_MAX:
        out["applied"], out["bad"] = 0, 1
        return out
    out["step"] = block["step"] + 1
    out["sc"] = scalars(kind, *(block[name] for name in INPUTS), out["step"])
    out["applied"], out["bad"] = 1, 0
    return out


def same_block(got: dict, want: dict) -> bool:
    """Two blocks (OptHyper.read() / this module's dicts) equal bit for bit."""
    for name in INPUTS:
        if np.float64(got[name]).view(np.int64) != np.float64(want[name]).view(np.int64):
            return False
    if any(int(got[k]) != int(want[k]) for k in ("seed", "step", "applied", "bad")):
        return False
    return all(np.float32(got["sc"][k]).view(np.uint32) == np.float32(want["sc"][k]).view(np.uint32) for k in FIELDS)
