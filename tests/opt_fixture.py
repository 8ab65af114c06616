"""The optimizer step (include/scone_hip.h, "optimizer step") in plain numpy.

`step_f32` is the contract: np.float32 scalars and arrays, ONE numpy operation per rounding, the scalars taken as arguments
(the tests read them from `scone_opt_scalars_of`; `scalars_f64` is their definition in numpy double).  `step_f64` is the same
formulas in float64 with unrounded scalars: what both fp32 evaluations (this one and torch's) are measured against.
`apply` walks an id list by the call's id rules.  `fma=True` evaluates every `a * b + c` shape the way a fused multiply-add
would (the exact product, one rounding); `ftz=True` flushes subnormal operands and results to zero: the two variants the edge
test must tell from the contract.
"""

import numpy as np

SGD, ADAGRAD, ADAM = 0, 1, 2
KINDS = {"sgd": SGD, "adagrad": ADAGRAD, "adam": ADAM}
NAMES = ("alpha", "b1", "b2", "c1", "c2", "eps", "decay", "gscale")
F32 = np.float32
_TINY = np.float32(2.0 ** -126)


def kind_code(kind):
    return KINDS[kind] if isinstance(kind, str) else int(kind)


def scalars_f64(kind, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, step=1):
    """The scalars in numpy double, not yet rounded."""
    b1, b2 = np.float64(betas[0]), np.float64(betas[1])
    lr = np.float64(lr)
    alpha = lr
    if kind_code(kind) == ADAM:
        t = np.float64(step)
        alpha = lr * np.sqrt(1.0 - np.power(b2, t)) / (1.0 - np.power(b1, t))
    return dict(alpha=alpha, b1=b1, b2=b2, c1=1.0 - b1, c2=1.0 - b2, eps=np.float64(eps), decay=lr * np.float64(weight_decay),
                gscale=np.float64(grad_scale))


def scalars_f32(*args, **kwargs):
    return {k: F32(v) for k, v in scalars_f64(*args, **kwargs).items()}


def _ftz(x):
    x = np.asarray(x, dtype=F32)
    return np.where(np.abs(x) < _TINY, np.copysign(F32(0), x), x).astype(F32)


class _Ops:
    """fp32 arithmetic, one rounding per call; `fma` / `ftz` select the two wrong machines."""

    def __init__(self, fma=False, ftz=False):
        self.fma, self.ftz = fma, ftz

    def _in(self, x):
        x = np.asarray(x, dtype=F32)
        return _ftz(x) if self.ftz else x

    def _out(self, x):
        x = np.asarray(x).astype(F32)
        return _ftz(x) if self.ftz else x

    def mul(self, a, b):
        return self._out(self._in(a) * self._in(b))

    def add(self, a, b):
        return self._out(self._in(a) + self._in(b))

    def sub(self, a, b):
        return self._out(self._in(a) - self._in(b))

    def div(self, a, b):
        return self._out(self._in(a) / self._in(b))

    def sqrt(self, a):
        return self._out(np.sqrt(self._in(a)))

    def mul_add(self, a, b, c, sign=1.0):
        """c + sign * (a * b): two roundings -- or one, where a fused multiply-add would be used."""
        if not self.fma:
            p = self.mul(a, b)
            return self.add(c, p) if sign > 0 else self.sub(c, p)
        exact = self._in(a).astype(np.float64) * self._in(b).astype(np.float64)      # 48 bits: exact in double
        return self._out(self._in(c).astype(np.float64) + sign * exact)


def step_f32(kind, sc, g, w, m=None, v=None, fma=False, ftz=False):
    """(w', m', v') of whole arrays; m / v are returned unchanged where the kind does not use them."""
    kind = kind_code(kind)
    o = _Ops(fma, ftz)
    sc = {k: F32(sc[k]) for k in NAMES}
    g, w = np.asarray(g, dtype=F32), np.asarray(w, dtype=F32)
    with np.errstate(all="ignore"):
        g1 = g if sc["gscale"] == F32(1) else o.mul(g, sc["gscale"])
        w1 = w if sc["decay"] == F32(0) else o.mul_add(sc["decay"], w, w, sign=-1.0)
        if kind == SGD:
            return o.mul_add(sc["alpha"], g1, w1, sign=-1.0), m, v
        if kind == ADAGRAD:
            v2 = o.mul_add(g1, g1, np.asarray(v, dtype=F32))
            den = o.add(o.sqrt(v2), sc["eps"])
            return o.sub(w1, o.div(o.mul(sc["alpha"], g1), den)), m, v2
        m2 = o.mul_add(sc["b1"], np.asarray(m, dtype=F32), o.mul(sc["c1"], g1))
        v2 = o.mul_add(sc["b2"], np.asarray(v, dtype=F32), o.mul(sc["c2"], o.mul(g1, g1)))
        den = o.add(o.sqrt(v2), sc["eps"])
        return o.sub(w1, o.div(o.mul(sc["alpha"], m2), den)), m2, v2


def step_f64(kind, sc64, g, w, m=None, v=None):
    """The same formulas in float64 with the unrounded scalars of `scalars_f64`."""
    kind = kind_code(kind)
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        g1 = g * sc64["gscale"]
        w1 = w - sc64["decay"] * w
        if kind == SGD:
            return w1 - sc64["alpha"] * g1, m, v
        if kind == ADAGRAD:
            v2 = np.asarray(v, dtype=np.float64) + g1 * g1
            return w1 - (sc64["alpha"] * g1) / (np.sqrt(v2) + sc64["eps"]), m, v2
        m2 = sc64["b1"] * np.asarray(m, dtype=np.float64) + sc64["c1"] * g1
        v2 = sc64["b2"] * np.asarray(v, dtype=np.float64) + sc64["c2"] * (g1 * g1)
        return w1 - (sc64["alpha"] * m2) / (np.sqrt(v2) + sc64["eps"]), m2, v2


def valid_entries(ids, row_begin, row_end):
    """Which entries of the list the call applies: inside [row_begin, row_end) and above their predecessor IN THE LIST."""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= row_begin) & (ids < row_end)
    if len(ids) > 1:
        ok[1:] &= ids[1:] > ids[:-1]
    return ok


def apply(kind, sc, ids, grad_rows, master, state1=None, state2=None, row_begin=0, row_end=None, step=step_f32, **kw):
    """One call on copies of the owned-row arrays: returns (master', state1', state2', applied ids, bad) -- `bad` is whether
    SCONE_ST_BAD_ID is raised.  Arrays are indexed by id - row_begin."""
    row_end = row_begin + master.shape[0] if row_end is None else row_end
    ids = np.asarray(ids, dtype=np.int64)
    ok = valid_entries(ids, row_begin, row_end)
    master = master.copy()
    state1 = None if state1 is None else state1.copy()
    state2 = None if state2 is None else state2.copy()
    at = ids[ok] - row_begin
    if len(at):
        w, m, v = step(kind, sc, np.asarray(grad_rows)[ok], master[at], None if state1 is None else state1[at],
                       None if state2 is None else state2[at], **kw)
        master[at] = w
        if kind_code(kind) == ADAM:
            state1[at] = m
        if kind_code(kind) != SGD:
            state2[at] = v
    return master, state1, state2, ids[ok], bool((~ok).any())
