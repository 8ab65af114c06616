"""TEST CODE ONLY -- the bfloat16 row format (SCONE_FMT_BF16) stated twice on the host, independently of the HIP code:

* `to_bf16_bits` / `from_bf16_bits`: integer arithmetic on the fp32 bit patterns, in numpy.  A bf16 is the upper half of an
  fp32; storing rounds to nearest, ties (low half exactly 0x8000) to the even upper half.  The carry of the increment does the
  rest of IEEE 754 by itself: the largest finite values carry into the exponent and become +-inf, fp32 subnormals round into
  bf16 subnormals, -0.0 and +-inf pass through.  NaN is taken out first (the increment would carry 0x7FFFFFFF into the sign bit,
  and a truncation could leave 0x7F80, an infinity): it stays a NaN with the quiet bit set.
* `torch_bf16_bits`: torch's CPU `.bfloat16()`.

tests/test_bf16_format_host.py holds the two to each other; the GPU tests quantise their tables with the first.  Nothing under
scone_amd/ may import this module (oracle/ref_port.py states the older formats; this is where the new one is stated).
"""

import numpy as np
import torch


def to_bf16_bits(x):
    """float32 array -> uint16 array of bf16 bit patterns (IEEE round-to-nearest-even; NaN -> quiet NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)                  # room for the carry out of bit 31
    rounded = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    quiet = (u >> np.uint64(16)) | np.uint64(0x0040)
    return np.where(nan, quiet, rounded).astype(np.uint16).reshape(x.shape)


def from_bf16_bits(b):
    """uint16 array of bf16 bit patterns -> the float32 values they stand for (bits << 16; exact)."""
    b = np.ascontiguousarray(b, dtype=np.uint16)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).reshape(b.shape)


def stored(x):
    """What a bf16 table holds of fp32 rows, as fp32: the oracle runs on this."""
    return from_bf16_bits(to_bf16_bits(x))


def torch_bf16_bits(x):
    """The same rounding by torch's CPU conversion, as uint16 bit patterns."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16()
    return t.view(torch.int16).numpy().view(np.uint16)


def is_nan_bits(b):
    b = np.asarray(b, dtype=np.uint16)
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


def same_bf16_bits(got, want):
    """NaN positions equal, every other element bit for bit (tests/edge_fixture.py same_bits, for uint16 bf16 patterns)."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    if got.shape != want.shape:
        return False
    gn, wn = is_nan_bits(got), is_nan_bits(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn]))


def rows_as_bits(raw_rows):
    """`SconeTable.download`'s uint8 [n, 2 d] payload of a bf16 table -> uint16 [n, d]."""
    raw_rows = np.ascontiguousarray(raw_rows)
    return raw_rows.view(np.uint16).reshape(raw_rows.shape[0], -1)


def edge_values():
    """fp32 values on every edge of the fp32 -> bf16 rounding, as one 1-D array."""
    def f(bits):
        return np.asarray(bits, dtype=np.uint32).view(np.float32)
    v = [
        f([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000]),      # ties: upper half even (stays) / odd (goes up), both signs
        f([0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001]),      # one fp32 ulp on either side of the ties
        f([0x7F7F0000, 0xFF7F0000]),                              # +-largest bf16
        f([0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF]),   # last to stay finite; first to round to inf; FLT_MAX
        f([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x007F8000, 0x80000001, 0x80008000,
           0x807FFFFF]),                                          # fp32 subnormals: to zero, ties, into bf16 subnormals, up to FLT_MIN
        f([0x00800000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000]),             # FLT_MIN, +-0, +-inf
        f([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF, 0x7FBF8000, 0xFFBFFFFF]),  # quiet / signalling NaNs
    ]
    return np.concatenate(v)
