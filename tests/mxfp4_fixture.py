"""TEST CODE ONLY -- the MXFP4 table format (SCONE_FMT_MXFP4, include/scone_hip.h) stated twice and independently in numpy.
Nothing under scone_amd/ may import this module.

The format: a row of d fp32 values (d % 128 == 0) is cut into blocks of 32 consecutive elements.  A block is stored as 32 E2M1
nibbles `s m2 m1 m0` (magnitude codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign; no inf / NaN code; element 2k is the
low nibble of payload byte k) and one E8M0 scale byte X: 2^(X-127) for X in 0..254, X = 255 makes the block NaN.
value = fp32(elem) * fp32(2^(X-127)), one IEEE fp32 product.

Quantiser (OCP MX v1.0): a block with a NaN or +-inf gets X = 255 (nibbles: the sign bits only); else amax = max|v|;
amax == 0 -> X = 127; else X = clamp(floor(log2(amax)) - 2 + 127, 0, 254); each v / 2^(X-127) goes to the nearest E2M1
magnitude, ties to the even code, above 6 to 6, sign kept.

  (a) `quantize`      value arithmetic: np.frexp for the exponent, np.ldexp for the quotient (exact in float64), the nearest of
                      the eight magnitudes with the midpoint table for the ties
  (b) `quantize_bits` integer work on the fp32 bit patterns: the exponent field for the scale, shift-and-round for the element
"""

import numpy as np

BLOCK = 32
MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)
MIDPOINTS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=np.float64)
MIDPOINT_CODES = np.array([0, 2, 2, 4, 4, 6, 6], dtype=np.uint8)       # a tie goes to the even code


def _blocks(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.ndim == 2 and x.shape[1] % 128 == 0, x.shape
    return x.reshape(x.shape[0], x.shape[1] // BLOCK, BLOCK)


def pack(codes):
    """nibbles uint8 [n, d] -> payload bytes [n, d/2]: element 2k is the low nibble of byte k."""
    codes = np.asarray(codes, dtype=np.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack(payload):
    payload = np.asarray(payload, dtype=np.uint8)
    out = np.empty((payload.shape[0], payload.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = payload & 0xF, payload >> 4
    return out


# ------------------------------------------------------------------ (a) value arithmetic
def scale_bytes(x):
    """uint8 [n, d/32]."""
    b = _blocks(x)
    with np.errstate(invalid="ignore"):
        amax = np.abs(b).max(axis=2)
    bad = ~np.isfinite(b).all(axis=2)
    _, e = np.frexp(np.where(bad | (amax == 0), np.float32(1), amax).astype(np.float64))     # amax = m 2^e, m in [0.5, 1)
    X = np.clip(e - 1 - 2 + 127, 0, 254)
    X = np.where(amax == 0, 127, X)
    return np.where(bad, 255, X).astype(np.uint8)


def quantize(x):
    """(payload uint8 [n, d/2], scales uint8 [n, d/32])."""
    b = _blocks(x)
    X = scale_bytes(x)
    live = (X != 255)[:, :, None]
    q = np.ldexp(np.abs(np.where(live, b, np.float32(0))).astype(np.float64), 127 - X.astype(np.int64)[:, :, None])   # exact
    dist = np.abs(q[..., None] - MAGNITUDES)
    code = dist.argmin(axis=-1).astype(np.uint8)                       # the nearest magnitude (above 6: 6) ...
    for m, c in zip(MIDPOINTS, MIDPOINT_CODES):
        code = np.where(q == m, c, code)                               # ... and on a midpoint the even code
    code = code | (np.signbit(b).astype(np.uint8) << 3)
    return pack(code.reshape(b.shape[0], -1)), X


# ------------------------------------------------------------------ (b) the bit patterns
def quantize_bits(x):
    b = _blocks(x)
    u = b.view(np.uint32).astype(np.int64)
    mag = u & 0x7FFFFFFF
    top = mag.max(axis=2)
    X = np.maximum((top >> 23) - 2, 0)                  # exponent field - 2: a subnormal amax has field 0, FLT_MAX 254
    X = np.where(top == 0, 127, X)
    X = np.where(top >= 0x7F800000, 255, X)
    field, frac = mag >> 23, mag & 0x7FFFFF
    sig = np.where(field > 0, frac | (1 << 23), frac)                   # |v| = sig 2^(max(field, 1) - 150)
    sh = np.maximum(field, 1) - 150 + 127 - X[:, :, None]               # q = sig 2^sh

    def below(limit_log2):                                              # q < 2^limit_log2
        n = limit_log2 - sh
        return np.where(n > 40, True, sig < (np.int64(1) << np.clip(n, 0, 40)))

    def round_half_even(s):                                             # sig 2^s to an integer; s < 0 wherever it is used
        n = np.clip(-s, 1, 62)
        fl, rem, half = sig >> n, sig & ((np.int64(1) << n) - 1), np.int64(1) << (n - 1)
        r = fl + ((rem > half) | ((rem == half) & ((fl & 1) == 1)))
        return np.where(-s > 62, 0, np.where(s >= 0, 1 << 20, r))

    # [0, 2): steps of 0.5, code = round(2 q); [2, 4): steps of 1, code = 2 + round(q); [4, ..): steps of 2, code = 4 + round(q / 2)
    code = np.where(below(1), round_half_even(sh + 1), np.where(below(2), 2 + round_half_even(sh), 4 + round_half_even(sh - 1)))
    code = np.minimum(code, 7)
    code = np.where((X == 255)[:, :, None], 0, code) | ((u >> 31) << 3)
    return pack(code.reshape(b.shape[0], -1).astype(np.uint8)), X.astype(np.uint8)


# ------------------------------------------------------------------ what the table holds
def scale_value(X):
    """fp32 factor of a scale byte: 2^(X-127), the subnormal 2^-127 at X = 0, NaN at 255."""
    X = np.asarray(X)
    f = np.ldexp(np.float32(1), X.astype(np.int32) - 127).astype(np.float32)
    return np.where(X == 255, np.float32(np.nan), f).astype(np.float32)


def dequantize(payload, scales):
    """fp32 [n, d]: one fp32 product per element."""
    codes = unpack(payload)
    elem = MAGNITUDES.astype(np.float32)[codes & 7] * np.where(codes & 8, np.float32(-1), np.float32(1))
    with np.errstate(over="ignore", invalid="ignore"):
        return (elem.astype(np.float32) * np.repeat(scale_value(scales), BLOCK, axis=1)).astype(np.float32)


def stored(x):
    return dequantize(*quantize(x))


def edge_values():
    """fp32 values around every decision of the quantiser, as multiples of a block maximum of 6 (X = 127): each midpoint, one ulp
    to either side, both signs; the saturating values; zeros."""
    v = []
    for m in MIDPOINTS.astype(np.float32):
        v += [np.nextafter(m, np.float32(0)), m, np.nextafter(m, np.float32(9))]
    v += [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 2.0 ** -140, 1e-30]
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([v, -v]).astype(np.float32)


def edge_rows(d=128, seed=0):
    """Rows [n, d] whose blocks meet every branch: the edge values under amax = 6 and under other powers of two, amax exactly a
    power of two and one ulp below, all-zero and all -0 blocks, NaN / inf blocks, subnormal amax (X = 0), FLT_MAX (X = 252), tiny
    elements under a huge amax, and random bit patterns."""
    rng = np.random.default_rng(seed)
    ev = edge_values()
    rows = []
    for scale in (1.0, 2.0 ** -20, 2.0 ** 100, 2.0 ** -125, 2.0 ** -128):
        r = np.resize(ev, d).astype(np.float32)
        r[::BLOCK] = 6.0                                                # every block's amax: 6 -> X = 127 before scaling
        rows.append((r.astype(np.float64) * scale).astype(np.float32))
    r = rng.standard_normal(d).astype(np.float32)
    r[0:32] = np.clip(r[0:32], -1, 1); r[5] = 4.0                       # amax a power of two
    r[32:64] = np.clip(r[32:64], -1, 1); r[40] = np.nextafter(np.float32(4.0), np.float32(0))     # one ulp below
    r[64:96] = 0.0
    r[96:128] = -0.0
    rows.append(r)
    r = rng.standard_normal(d).astype(np.float32)
    r[3] = np.nan; r[32 + 7] = np.inf; r[64 + 9] = -np.inf
    r[96:128] = (rng.integers(-2 ** 20, 2 ** 20, size=32) * 2.0 ** -149).astype(np.float32)      # subnormal amax
    rows.append(r)
    r = rng.standard_normal(d).astype(np.float32)
    r[0] = np.finfo(np.float32).max; r[33] = -np.finfo(np.float32).max
    r[64] = 2.0 ** 127; r[65:96] = (rng.integers(1, 2 ** 23, size=31) * 2.0 ** -149).astype(np.float32)
    r[96:128] = [6.0, 6.0000005, 7.99, -6.0000005, -7.99, 5.0, -5.0, 0.25] * 4
    rows.append(r)
    for _ in range(4):
        rows.append(rng.integers(0, 2 ** 32, size=d, dtype=np.uint64).astype(np.uint32).view(np.float32))
    return np.stack(rows).astype(np.float32)


# ------------------------------------------------------------------ the synthetic fill (scone_table_fill_synthetic), restated
def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    return x


def _base(seed, c):
    c = np.asarray(c, dtype=np.uint64)
    return hash32(((c & np.uint64(0xFFFFFFFF)) + np.uint64(0x9E3779B9) * (c >> np.uint64(32))) & np.uint64(0xFFFFFFFF)) ^ np.uint64(seed)


def synthetic(seed, ids, d, base_scale):
    """(payload [n, d/2], scales [n, d/32]) of rows `ids`: payload dword w = hash32(base(g) + w) (the words INT4 gets), scale byte
    of block b = E - 1 + (hash32(base(g * d/32 + b) + 0x51ED27) >> 8) % 3 with E the exponent field of base_scale in [1, 253]."""
    ids = np.asarray(ids, dtype=np.uint64)
    nb = d // BLOCK
    words = hash32((_base(seed, ids)[:, None] + np.arange(d // 8, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    payload = np.ascontiguousarray(words).view(np.uint8).reshape(len(ids), d // 2)
    E = int(np.clip((np.float32(base_scale).view(np.uint32) >> 23) & 0xFF, 1, 253))
    counters = ids[:, None] * np.uint64(nb) + np.arange(nb, dtype=np.uint64)[None, :]
    X = E - 1 + ((hash32((_base(seed, counters) + np.uint64(0x51ED27)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)) % np.uint64(3)).astype(np.int64)
    return payload, X.astype(np.uint8)
