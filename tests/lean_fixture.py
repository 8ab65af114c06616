"""The lean optimizer step (include/scone_hip.h, "lean optimizer step") in plain numpy, on tests/opt_fixture.py's `_Ops`.

`step_f32` is the contract: np.float32 scalars and arrays, ONE numpy operation per rounding, the scalars taken as arguments (the
tests read them from `scone_lean_scalars_of`; `scalars_f64` is their definition in numpy double).  `row_sum_sq` is the row sum
of row-wise Adagrad in the contract's order: element j belongs to lane (j / 4) % 64, a lane adds its elements in ascending j
(product rounded first, then the sum), the 64 lanes are combined by the butterfly s = 32 .. 1.  `step_f64` is the same formulas
in float64 with unrounded scalars and a plain sum.  `rand16`, `round_bf16_nearest` and `round_bf16_stochastic` state the
rounding of an in-place bf16 row in integer arithmetic.  `apply` walks an id list by `opt_fixture.valid_entries`' rules.
`fma=True` evaluates every `a * b + c` shape the way a fused multiply-add would; `ftz=True` flushes subnormals: the two wrong
machines the edge tests must tell from the contract.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import opt_fixture as OF  # noqa: E402

SGD, ROWWISE_ADAGRAD = 0, 1
KINDS = {"sgd": SGD, "rowwise_adagrad": ROWWISE_ADAGRAD}
NEAREST, STOCHASTIC = 0, 1
F32 = np.float32
U32 = np.uint32
LANES, PIECE = 64, 4


def kind_code(kind):
    return KINDS[kind] if isinstance(kind, str) else int(kind)


def scalars_f64(kind, lr, eps=1e-10, weight_decay=0.0, grad_scale=1.0):
    """The scalars in numpy double, not yet rounded (the fields the lean step does not use are 0)."""
    lr = np.float64(lr)
    out = {k: np.float64(0) for k in OF.NAMES}
    out.update(alpha=lr, eps=np.float64(eps), decay=lr * np.float64(weight_decay), gscale=np.float64(grad_scale))
    return out


def scalars_f32(*args, **kwargs):
    return {k: F32(v) for k, v in scalars_f64(*args, **kwargs).items()}


# ------------------------------------------------------------------ random bits and the rounding of a bf16 row
def _mix(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)      # 32-bit arithmetic held in 64 bits: the products are masked
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


def _halves(v):
    v = np.asarray(v)
    v = v.astype(np.int64).view(np.uint64) if v.dtype.kind == "i" else v.astype(np.uint64)
    return v & np.uint64(0xFFFFFFFF), v >> np.uint64(32)


def rand16(seed, step, row, col):
    """16 random bits of (seed uint64, step int64, GLOBAL row id uint64, column uint32); the arguments broadcast."""
    h = np.uint64(0x9E3779B9)
    for v in (*_halves(np.asarray(seed, dtype=np.uint64)), *_halves(np.asarray(step, dtype=np.int64)),
              *_halves(np.asarray(row, dtype=np.uint64)), np.asarray(col, dtype=np.uint64)):
        h = _mix(h ^ v)
    return (h >> np.uint64(16)).astype(U32)


def round_bf16_nearest(x):
    return BF.to_bf16_bits(x)


def round_bf16_stochastic(x, r):
    """(u + r) >> 16 in 32-bit arithmetic, r in [0, 65536); an exponent field of all ones (inf / NaN) rounds as nearest does."""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(U32).astype(np.uint64)
    r = np.broadcast_to(np.asarray(r, dtype=np.uint64), u.shape)
    assert (r < 65536).all()
    bits = (((u + r) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)).astype(np.uint16)
    special = (u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    return np.where(special, BF.to_bf16_bits(x), bits).astype(np.uint16)


def store_bf16(w, rounding, seed=0, step=1, row_ids=None):
    """The bf16 bits an in-place step stores for fp32 rows `w` [U, d] of GLOBAL rows `row_ids`."""
    if rounding in (NEAREST, "nearest"):
        return round_bf16_nearest(w)
    rows = np.asarray(row_ids, dtype=np.uint64).reshape(-1, 1)
    cols = np.arange(w.shape[1], dtype=np.uint64).reshape(1, -1)
    return round_bf16_stochastic(w, rand16(seed, step, rows, cols))


# ------------------------------------------------------------------ the arithmetic
def row_sum_sq(g1, fma=False, ftz=False):
    """q [rows] of g1 [rows, d] in the contract's order.  d % 4 == 0."""
    o = OF._Ops(fma, ftz)
    g1 = np.asarray(g1, dtype=F32)
    rows, d = g1.shape
    assert d % PIECE == 0
    block = LANES * PIECE
    nblocks = -(-d // block)
    pad = np.zeros((rows, nblocks * block), dtype=F32)
    pad[:, :d] = g1
    have = np.zeros(nblocks * block, dtype=bool)
    have[:d] = True
    x = pad.reshape(rows, nblocks, LANES, PIECE)                    # element j = ((b * 64) + lane) * 4 + k
    have = have.reshape(nblocks, LANES, PIECE)
    q = np.zeros((rows, LANES), dtype=F32)
    with np.errstate(all="ignore"):
        for b in range(nblocks):                                   # ascending j inside every lane
            for k in range(PIECE):
                e = x[:, b, :, k]
                nxt = o.mul_add(e, e, q)
                q = np.where(have[b, :, k][None, :], nxt, q).astype(F32)
        lanes = np.arange(LANES)
        for s in (32, 16, 8, 4, 2, 1):
            q = o.add(q, q[:, lanes ^ s])
    same = (q.view(U32) == q[:, :1].view(U32)) | (np.isnan(q) & np.isnan(q[:, :1]))
    assert same.all(), "the butterfly left the lanes with different bits"
    return q[:, 0].copy()


def step_f32(kind, sc, g, w, s=None, fma=False, ftz=False):
    """(w', s') of whole arrays: g, w [rows, d], s [rows] (returned unchanged by SGD)."""
    kind = kind_code(kind)
    o = OF._Ops(fma, ftz)
    sc = {k: F32(sc[k]) for k in OF.NAMES}
    g, w = np.asarray(g, dtype=F32), np.asarray(w, dtype=F32)
    with np.errstate(all="ignore"):
        g1 = g if sc["gscale"] == F32(1) else o.mul(g, sc["gscale"])
        w1 = w if sc["decay"] == F32(0) else o.mul_add(sc["decay"], w, w, sign=-1.0)
        if kind == SGD:
            return o.mul_add(sc["alpha"], g1, w1, sign=-1.0), s
        q = row_sum_sq(g1, fma, ftz)
        g2 = o.div(q, F32(g.shape[1]))
        s2 = o.add(np.asarray(s, dtype=F32), g2)
        den = o.add(o.sqrt(s2), sc["eps"])
        return o.sub(w1, o.div(o.mul(sc["alpha"], g1), den[:, None])), s2


def step_f64(kind, sc64, g, w, s=None):
    """The same formulas in float64 with the unrounded scalars of `scalars_f64` and a plain row sum."""
    kind = kind_code(kind)
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        g1 = g * sc64["gscale"]
        w1 = w - sc64["decay"] * w
        if kind == SGD:
            return w1 - sc64["alpha"] * g1, s
        s2 = np.asarray(s, dtype=np.float64) + (g1 * g1).sum(axis=1) / g.shape[1]
        return w1 - (sc64["alpha"] * g1) / (np.sqrt(s2) + sc64["eps"])[:, None], s2


def apply(kind, sc, ids, grad_rows, weights, row_state=None, row_begin=0, row_end=None, step=step_f32, **kw):
    """One call on copies of the owned-row arrays (fp32 weights [owned, d] -- the master, or an in-place fp32 table): returns
    (weights', row_state', applied ids, bad) -- `bad` is whether SCONE_ST_BAD_ID is raised.  Arrays are indexed by id - row_begin."""
    row_end = row_begin + weights.shape[0] if row_end is None else row_end
    ids = np.asarray(ids, dtype=np.int64)
    ok = OF.valid_entries(ids, row_begin, row_end)
    weights = weights.copy()
    row_state = None if row_state is None else row_state.copy()
    at = ids[ok] - row_begin
    if len(at):
        w, s = step(kind, sc, np.asarray(grad_rows)[ok], weights[at], None if row_state is None else row_state[at], **kw)
        weights[at] = w
        if kind_code(kind) == ROWWISE_ADAGRAD:
            row_state[at] = s
    return weights, row_state, ids[ok], bool((~ok).any())


def apply_bf16(kind, sc, ids, grad_rows, bits, row_state=None, row_begin=0, row_end=None, rounding=NEAREST, seed=0, step_no=1, **kw):
    """One in-place call on a bf16 table given as uint16 bits [owned, d]: returns (bits', row_state', applied ids, bad, w'), w'
    the fp32 rows [applied, d] before they were rounded."""
    row_end = row_begin + bits.shape[0] if row_end is None else row_end
    ids = np.asarray(ids, dtype=np.int64)
    ok = OF.valid_entries(ids, row_begin, row_end)
    bits = bits.copy()
    row_state = None if row_state is None else row_state.copy()
    at = ids[ok] - row_begin
    w = np.zeros((0, bits.shape[1]), dtype=F32)
    if len(at):
        w, s = step_f32(kind, sc, np.asarray(grad_rows)[ok], BF.from_bf16_bits(bits[at]), None if row_state is None else row_state[at], **kw)
        bits[at] = store_bf16(w, rounding, seed, step_no, ids[ok])
        if kind_code(kind) == ROWWISE_ADAGRAD:
            row_state[at] = s
    return bits, row_state, ids[ok], bool((~ok).any()), w
