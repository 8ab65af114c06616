"""CPU: the entry points of include/scone_hip.h, "backward and optimizer step without a host synchronisation" are declared,
bound and exported, and the bound on the partial slots that sizes a context's largest buffer holds.

The bound.  A row of r > C references is cut into ceil(r / C) chunks, each with a partial slot; a row of r <= C references has
none.  The header states slots <= floor(2 R / (C + 1)) for R references in all, and `scone_backward_ctx_partial_slots` returns
that number.  Here the slots of adversarial distributions are counted by numpy from the definition and held against the
library's number: all references on one row, every row at C + 1 (where the bound is reached), rows at C (no slot at all), rows
one short of and one above a multiple of C, and random mixes."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from scone_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["scone_backward_ctx_partial_slots", "scone_backward_ctx_create", "scone_backward_ctx_bytes", "scone_backward_ctx_destroy",
       "scone_backward_plan_dn", "scone_backward_plan_varlen_dn", "scone_backward_ctx_counts", "scone_backward_rows_dn",
       "scone_opt_step_dn", "scone_opt_step_lean_dn", "scone_grad_sqnorm_dn"]


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(scone_[a-z0-9_]+)\s*\(", text))


def test_new_symbols_are_declared_bound_and_exported():
    declared = _declared_symbols()
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scone_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.scone_abi_version() == _lib.ABI_VERSION == 2, "the section is appended: the ABI version stays"
    assert _lib.ST_ROWS_OVERFLOW == 16


def test_status_bit_4_is_documented_beside_the_others():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    at = text.index("int scone_status(")
    assert "bit 4" in text[at - 1200:at]


def _slots(lengths, chunk):
    """Partial slots of rows with these reference counts, from the definition."""
    r = np.asarray(lengths, dtype=np.int64)
    chunks = -(-r // chunk)
    return int(chunks[r > chunk].sum())


def _bound(refs):
    return _lib.backward_ctx_partial_slots(int(refs))


def _distributions(chunk):
    rng = np.random.default_rng(24)
    yield "one row", [1_000_003]
    yield "one row of C", [chunk]
    yield "one row of C + 1", [chunk + 1]
    yield "every row at C + 1", [chunk + 1] * 4097
    yield "every row at C", [chunk] * 4097
    yield "every row at 2 C + 1", [2 * chunk + 1] * 999
    yield "every row at 2 C - 1", [2 * chunk - 1] * 999
    yield "C + 1 and singles", [chunk + 1] * 500 + [1] * 77
    for i in range(20):
        n = int(rng.integers(1, 3000))
        kind = i % 4
        if kind == 0:
            r = rng.integers(1, 4 * chunk, size=n)
        elif kind == 1:
            r = rng.choice([1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 7 * chunk + 3], size=n)
        elif kind == 2:
            r = np.minimum(rng.zipf(1.3, size=n), 50_000)
        else:
            r = chunk + 1 + rng.integers(0, 3, size=n)
        yield f"random {i}", r.tolist()


def test_partial_slot_bound_holds_and_is_reached():
    chunk = _lib.lib().scone_backward_chunk()
    assert chunk >= 64
    reached = False
    for name, lengths in _distributions(chunk):
        refs = int(np.sum(np.asarray(lengths, dtype=np.int64)))
        slots, bound = _slots(lengths, chunk), _bound(refs)
        assert bound == 2 * refs // (chunk + 1), f"{name}: the library's number is not the header's formula"
        assert slots <= bound, f"{name}: {slots} slots for {refs} references, the bound says {bound}"
        reached |= slots == bound and slots > 0
        # ... and the bound does not shrink when references are added that the batch does not have (a context is sized by the
        # most references a batch CAN have)
        assert _bound(refs + 12345) >= bound
    assert reached, "no distribution reaches the bound: it is not tight, or the slots are counted wrongly"


def test_partial_slot_bound_refuses_what_cannot_be_numbered():
    out = C.c_uint64(0)
    lib = _lib.lib()
    assert lib.scone_backward_ctx_partial_slots(1 << 32, C.byref(out)) == _lib.EINVAL
    assert lib.scone_backward_ctx_partial_slots(10, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        _lib.backward_ctx_partial_slots(1 << 32)
    assert _bound(0) == 0 and _bound(chunk_plus(0)) == 1 and _bound(chunk_plus(1)) == 2


def chunk_plus(k):
    return _lib.lib().scone_backward_chunk() + k


def test_null_handles_and_contexts_are_refused_without_a_gpu():
    lib = _lib.lib()
    ctx = C.c_void_p()
    assert lib.scone_backward_ctx_create(None, 16, C.byref(ctx)) == _lib.EINVAL
    assert lib.scone_backward_ctx_bytes(None, None) == _lib.EINVAL
    assert lib.scone_backward_ctx_counts(None, None, None, None) == _lib.EINVAL
    assert lib.scone_backward_plan_dn(None, None, None, 1, 1, None) == _lib.EINVAL
    assert lib.scone_backward_rows_dn(None, None, None, 0, 0, None, None, 0, None, None) == _lib.EINVAL
    lib.scone_backward_ctx_destroy(None)                                   # a no-op
