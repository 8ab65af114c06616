"""CPU: the bindings of the gradient-accumulation entry points (include/scone_hip.h, "gradient accumulation"), what they refuse
without a GPU, and tests/grad_merge_fixture.py checked against an independent dict-based union-and-add.
"""

import ctypes as C
import inspect
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_merge_fixture as GM  # noqa: E402

from scone_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("scone_grad_merge_scratch", "scone_grad_merge_map", "scone_grad_merge_rows", "scone_backward_row_ids",
       "scone_backward_rows_acc")
SCALARS = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "int": C.c_int}


def _header_args(name):
    """The ctypes argument list the header's declaration of `name` asks for: a device pointer, a handle, a plan and a stream are
    c_void_p; a pointer to a host uint64 (not named d_*) is POINTER(c_uint64); scalars by their width."""
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    args = []
    for p in m.group(1).split(","):
        p = " ".join(p.replace("const", " ").split())
        if "*" in p:
            ctype, pname = [x.strip() for x in p.rsplit("*", 1)]
            args.append(C.POINTER(C.c_uint64) if ctype == "uint64_t" and not pname.startswith("d_") else C.c_void_p)
        else:
            ctype, pname = p.rsplit(" ", 1)
            args.append(C.c_void_p if ctype == "scone_stream_t" else SCALARS[ctype])
    return args


def test_header_argument_lists_equal_the_bindings():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == _header_args(name), name
    assert _lib.ABI_VERSION == 2


def test_library_exports_the_symbols():
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.scone_abi_version() == 2


def test_null_handle_is_refused_without_gpu_work():
    lib = _lib.lib()
    n = C.c_uint64(0)
    assert lib.scone_grad_merge_map(None, None, 0, None, 0, None, None, None, None, None, None, None, C.byref(n), None) == _lib.EINVAL
    assert lib.scone_grad_merge_rows(None, None, None, 0, None, None, None, None) == _lib.EINVAL
    assert lib.scone_backward_row_ids(None, None, None, 0, None) == _lib.EINVAL
    assert lib.scone_backward_rows_acc(None, None, None, 0, 0, None, None, None, 0, None, None, None) == _lib.EINVAL
    assert lib.scone_grad_merge_scratch(1, 1, None) == _lib.EINVAL


def test_scratch_is_monotone_in_both_arguments():
    sizes = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 1 << 20, (1 << 20) + 1, (1 << 32) - 2)
    got = np.array([[_lib.grad_merge_scratch(a, b) for b in sizes] for a in sizes], dtype=np.uint64)
    assert (got > 0).all() and (got % 16 == 0).all()
    assert (np.diff(got.astype(np.int64), axis=0) >= 0).all() and (np.diff(got.astype(np.int64), axis=1) >= 0).all()
    assert got[0, -1] > got[0, 0], "the scratch does not grow with the list it flags"
    assert got.max() < 5 * (1 << 32)                               # a word and a bit per id: never a row


# ------------------------------------------------------------------ the fixture against an independent road
def _lists(rng, n_a, n_b, span):
    a = np.sort(rng.choice(span, size=n_a, replace=False)).astype(np.int64)
    b = np.sort(rng.choice(span, size=n_b, replace=False)).astype(np.int64)
    return a, b


def test_fixture_equals_a_dict_based_union_and_add():
    rng = np.random.default_rng(5)
    for n_a, n_b, span, d in ((0, 0, 10, 4), (0, 5, 10, 4), (5, 0, 10, 8), (1, 1, 2, 4), (40, 40, 50, 12), (257, 63, 300, 8),
                              (64, 65, 1 << 40, 4)):
        a, b = _lists(rng, n_a, n_b, span)
        ra, rb = GM.edge_rows(n_a, d, n_a + 1), GM.edge_rows(n_b, d, n_b + 2)
        ids, rows = GM.merge(a, ra, b, rb)
        ids2, rows2 = GM.merge_dict(a, ra, b, rb)
        assert np.array_equal(ids, ids2) and GM.same_bits(rows, rows2), (n_a, n_b)
        _, src_a, src_b, pos_a, pos_b = GM.merge_map(a, b)
        assert np.array_equal(ids[pos_a], a) and np.array_equal(ids[pos_b], b)
        assert np.array_equal(src_a[pos_a], np.arange(n_a)) and np.array_equal(src_b[pos_b], np.arange(n_b))
        assert ((src_a != GM.ABSENT) | (src_b != GM.ABSENT)).all() and (np.diff(ids) > 0).all()


def test_fixture_copies_and_adds_special_values():
    neg0, sub = np.float32(-0.0), np.float32(1e-45)
    a, b = np.array([1, 5], dtype=np.int64), np.array([5, 9], dtype=np.int64)
    ra = np.array([[neg0, sub, np.inf, 1.0], [neg0, sub, np.inf, -np.inf]], dtype=np.float32)
    rb = np.array([[neg0, sub, -np.inf, np.nan], [neg0, -sub, np.nan, 2.0]], dtype=np.float32)
    ids, rows = GM.merge(a, ra, b, rb)
    assert ids.tolist() == [1, 5, 9]
    assert np.array_equal(rows[0].view(np.uint32), ra[0].view(np.uint32)), "a row only a has is not a copy"
    assert np.array_equal(rows[2].view(np.uint32)[:2], rb[1].view(np.uint32)[:2]) and np.isnan(rows[2][2])
    assert np.signbit(rows[0][0]) and np.signbit(rows[2][0]), "-0.0 became +0.0: an add to zero, not a copy"
    both = rows[1]
    assert np.signbit(both[0]) and both[0] == 0                    # -0 + -0 = -0
    assert both[1:2].view(np.uint32)[0] == 2                       # 2^-149 + 2^-149 = 2^-148: subnormals are kept
    assert np.isnan(both[2]) and np.isnan(both[3])                 # inf + -inf, -inf + nan
    # int64 order is signed, and ids beyond 2^31 and 2^40 are ordinary
    a = np.array([-3, 0, (1 << 31) - 1, 1 << 40], dtype=np.int64)
    b = np.array([0, (1 << 31) + 1, 1 << 40], dtype=np.int64)
    ids, src_a, src_b, pos_a, pos_b = GM.merge_map(a, b)
    assert ids.tolist() == [-3, 0, (1 << 31) - 1, (1 << 31) + 1, 1 << 40]
    assert src_a.tolist() == [0, 1, 2, 0xFFFFFFFF, 3] and src_b.tolist() == [0xFFFFFFFF, 0, 0xFFFFFFFF, 1, 2]
    assert pos_a.tolist() == [0, 1, 2, 4] and pos_b.tolist() == [1, 3, 4]


def test_rows_accumulate_is_keyword_only_with_default_none():
    from scone_amd.hip_backend import BackwardPlan, SconeTable
    p = inspect.signature(BackwardPlan.rows).parameters["accumulate"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(BackwardPlan.rows).parameters)[:4] == ["self", "grad_out", "reduce", "out"]
    assert callable(BackwardPlan.row_ids)
    assert list(inspect.signature(SconeTable.grad_merge).parameters) == ["self", "ids_a", "rows_a", "ids_b", "rows_b"]
