"""CPU: the entry points of include/scone_hip.h, "optimizer hyper-parameters on the device" are declared, bound and exported; the
block's layout; and scone_opt_hyper_scalars_of -- the host copy of what scone_opt_hyper_advance derives on the device -- against
tests/opt_hyper_fixture.py (bit for bit) and against scone_opt_scalars_of (every field but Adam's alpha identical; alpha within
one fp32 ulp everywhere, and identical on the grid the header names)."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_hyper_fixture as HF  # noqa: E402

from scone_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scone_hip.h")
NEW = ["scone_opt_hyper_scalars_of", "scone_opt_hyper_init", "scone_opt_hyper_advance", "scone_opt_step_dh", "scone_opt_step_lean_dh",
       "scone_grad_ctl_set_dh"]
NO_DEVICE_WORK = {"scone_opt_hyper_scalars_of"}
KINDS = ("sgd", "adagrad", "adam")


NEXT_SECTION = "/* ---- backward and optimizer step without a host synchronisation"


def _section():
    text = open(HEADER).read()
    return text[text.index("typedef struct scone_opt_hyper {"):text.index(NEXT_SECTION)]


def _protos(section):
    section = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    return re.findall(r"^(?:int|void)\s+(scone_\w+)\s*\(([^;{}]*?)\)\s*;", section, flags=re.S | re.M)


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scone_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scone_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert [name for name, _ in _protos(_section())] == NEW, "the section's prototypes, in the header's order"


def test_the_abi_version_is_unchanged():
    assert _lib.lib().scone_abi_version() == _lib.ABI_VERSION == 2, "the section is appended: the ABI version stays"
    assert re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", open(HEADER).read())


def test_the_section_stands_where_the_older_tests_leave_room():
    """tests/test_fit_partition_host.py pins scone_embed_select as the header's last prototype and tests/test_gpu_backward_dn.py
    counts the prototypes of the _dn section: the new section stands in front of the _dn section, behind everything older."""
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\bint\s+(scone_\w+)\s*\(", code)[-1] == "scone_embed_select"
    assert text.index("int scone_backward_rows_acc(") < text.index("/* ---- optimizer hyper-parameters on the device") \
        < text.index("typedef struct scone_opt_hyper {") < text.index(NEXT_SECTION) < text.index("typedef struct scone_bwd_ctx scone_bwd_ctx;")
    dn = text[text.index("typedef struct scone_bwd_ctx scone_bwd_ctx;"):text.index("the fused lookup at CHOSEN positions only")]
    assert "_dh(" not in dn and "scone_opt_hyper_" not in re.sub(r"/\*.*?\*/", "", dn, flags=re.S)
    assert "\"optimizer hyper-parameters on the\n * device\"" in text, "the 'Scalars under capture' paragraph points to the new section"


def test_prototypes_that_enqueue_work_end_in_a_void_pointer_stream():
    protos = _protos(_section())
    assert len(protos) == len(NEW)
    for name, args in protos:
        assert "scone_stream_t" not in args, f"{name}: the section spells its stream `void *stream`"
        if name in NO_DEVICE_WORK:
            assert "stream" not in args and "scone_handle" not in args, f"{name} takes no GPU and no handle"
        else:
            assert re.search(r",\s*void \*stream\s*$", args), f"{name}: `void *stream` is not its last argument"


def test_block_layout():
    H = _lib.SconeOptHyper
    assert C.sizeof(H) == 104 and C.alignment(H) == 8
    want = {"lr": 0, "beta1": 8, "beta2": 16, "eps": 24, "weight_decay": 32, "grad_scale": 40, "seed": 48, "step": 56, "sc": 64,
            "applied": 96, "bad": 100}
    assert {name: getattr(H, name).offset for name, _ in H._fields_} == want
    assert C.sizeof(_lib.OptScalars) == 32
    # ... and the header says the same
    section = _section()
    for name, at in (("seed", 48), ("step", 56), ("sc", 64), ("applied", 96), ("bad", 100)):
        assert re.search(rf"\b{name};\s*/\* {at}:", section), f"the header's comment on {name}"


def _cfg(kind, lr, betas, eps, wd, gs, step):
    return _lib.OptCfg(C.sizeof(_lib.OptCfg), HF.KINDS[kind], lr, betas[0], betas[1], eps, wd, gs, step)


def _of(fn, cfg):
    out = _lib.OptScalars()
    assert fn(C.byref(cfg), C.byref(out)) == _lib.OK
    return {name: np.float32(getattr(out, name)) for name in HF.FIELDS}


def _bits(x):
    return int(np.float32(x).view(np.uint32))


GRID_BETAS = ((0.9, 0.999), (0.0, 0.999), (0.5, 0.5))
GRID_T = (1, 2, 3, 1000, 2 ** 31 - 1)


@pytest.mark.parametrize("kind", KINDS)
def test_scalars_equal_the_fixture_and_the_by_value_scalars(kind):
    lib = _lib.lib()
    for betas in GRID_BETAS:
        for t in GRID_T:
            for lr, eps, wd, gs in ((1e-3, 1e-8, 0.0, 1.0), (0.0375, 1e-10, 0.01, 2.0 ** -16), (3.0, 0.5, 0.3, 1.0 / 3.0)):
                cfg = _cfg(kind, lr, betas, eps, wd, gs, t)
                got = _of(lib.scone_opt_hyper_scalars_of, cfg)
                want = HF.scalars(kind, lr, betas[0], betas[1], eps, wd, gs, t)
                tag = f"{kind} betas {betas} t {t} lr {lr}"
                assert {k: _bits(v) for k, v in got.items()} == {k: _bits(v) for k, v in want.items()}, f"{tag}: {got} != {want}"
                old = _of(lib.scone_opt_scalars_of, cfg)
                for name in HF.FIELDS:
                    if name != "alpha":
                        assert _bits(got[name]) == _bits(old[name]), f"{tag}: {name} differs from scone_opt_scalars_of"
                assert abs(_bits(got["alpha"]) - _bits(old["alpha"])) <= 1, f"{tag}: alpha is more than one fp32 ulp from pow()'s"
                if kind != "adam":
                    assert _bits(got["alpha"]) == _bits(np.float32(lr))


def test_alpha_equals_the_by_value_alpha_on_the_headers_grid():
    """lr = 1e-3, the four beta pairs, t = 1 .. 20000, 10^6, 12345678, 2^31 - 1: identical fp32 bits (the header says so)."""
    lib = _lib.lib()
    a, b = _lib.OptScalars(), _lib.OptScalars()
    ts = list(range(1, 20001)) + [10 ** 6, 12345678, 2 ** 31 - 1]
    for betas in ((0.9, 0.999), (0.9, 0.95), (0.5, 0.99), (0.0, 0.999)):
        cfg = _cfg("adam", 1e-3, betas, 1e-8, 0.0, 1.0, 1)
        for t in ts:
            cfg.step = t
            assert lib.scone_opt_hyper_scalars_of(C.byref(cfg), C.byref(a)) == 0 and lib.scone_opt_scalars_of(C.byref(cfg), C.byref(b)) == 0
            assert _bits(a.alpha) == _bits(b.alpha), f"betas {betas} t {t}: {a.alpha!r} != {b.alpha!r}"


def test_the_fixtures_advance():
    """The model the GPU test holds the device against: skip, bad and the count of APPLIED steps."""
    b0 = HF.init(1e-3, 0.9, 0.999, 1e-8, 0.01, 0.5, 7, 6)
    b1 = HF.advance(b0, "adam")
    assert b1["step"] == 7 and b1["applied"] == 1 and b1["bad"] == 0
    assert _bits(b1["sc"]["alpha"]) == _bits(HF.scalars("adam", 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.5, 7)["alpha"])
    b2 = HF.advance(b1, "adam", skip=True)
    assert b2["step"] == 7 and b2["applied"] == 0 and HF.same_block(dict(b2, applied=1), b1)
    b3 = HF.advance(dict(b1, lr=float("inf")), "adam")
    assert b3["step"] == 7 and b3["applied"] == 0 and b3["bad"] == 1 and HF.same_block(dict(b3, applied=1, bad=0, lr=1e-3), b1)
    assert HF.advance(dict(b1, step=HF.INT64_MAX), "sgd")["bad"] == 1
    assert HF.ipow(0.5, 10) == 2.0 ** -10 and HF.ipow(3.0, 0) == 1.0 and HF.ipow(0.0, 5) == 0.0


def test_refusals_without_a_gpu():
    lib = _lib.lib()
    out = _lib.OptScalars()
    good = _cfg("adam", 1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0, 1)
    assert lib.scone_opt_hyper_scalars_of(C.byref(good), C.byref(out)) == _lib.OK
    assert lib.scone_opt_hyper_scalars_of(None, C.byref(out)) == _lib.EINVAL
    assert lib.scone_opt_hyper_scalars_of(C.byref(good), None) == _lib.EINVAL
    for change in (dict(step=0), dict(kind=3), dict(struct_size=8), dict(lr=float("nan")), dict(beta2=float("inf")),
                   dict(grad_scale=float("-inf"))):
        bad = _cfg("adam", 1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0, 1)
        for k, v in change.items():
            setattr(bad, k, v)
        assert lib.scone_opt_hyper_scalars_of(C.byref(bad), C.byref(out)) == _lib.EINVAL, change
        assert lib.scone_opt_scalars_of(C.byref(bad), C.byref(out)) == _lib.EINVAL, f"{change}: the by-value call refuses it too"
    sgd0 = _cfg("sgd", 1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0, 0)
    assert lib.scone_opt_hyper_scalars_of(C.byref(sgd0), C.byref(out)) == _lib.OK, "only Adam reads the step"
    # every call that takes a handle refuses a null one before anything else
    assert lib.scone_opt_hyper_init(None, C.byref(good), 0, None, None) == _lib.EINVAL
    assert lib.scone_opt_hyper_advance(None, 0, None, None, None) == _lib.EINVAL
    assert lib.scone_opt_step_dh(None, 0, None, None, None, 0, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.scone_opt_step_lean_dh(None, 0, 0, None, None, None, 0, None, None, None, None, None) == _lib.EINVAL
    assert lib.scone_grad_ctl_set_dh(None, None, 1, None, 1.0, 0, None, None) == _lib.EINVAL
    from scone_amd.hip_backend import opt_hyper_scalars
    with pytest.raises(ValueError):
        opt_hyper_scalars("adam", 1e-3, step=0)
    assert _bits(opt_hyper_scalars("adam", 1e-3, step=3)["alpha"]) == _bits(HF.scalars("adam", 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 3)["alpha"])


def test_refusals_of_the_python_layer():
    """hyper= beside a by-value scalar, and capturable beside fused_backward: ValueError before anything touches a device."""
    import torch
    from scone_amd import FGramOptimizer
    from scone_amd.hip_backend import SconeTable
    ids, rows = torch.zeros(1, dtype=torch.int64), torch.zeros((1, 8))
    block = object()
    with pytest.raises(ValueError, match="hyper=.*lr="):
        SconeTable.opt_step(None, ids, rows, rows, kind="sgd", lr=0.1, hyper=block)
    with pytest.raises(ValueError, match="grad_scale="):
        SconeTable.opt_step(None, ids, rows, rows, kind="adam", grad_scale=0.5, hyper=block)
    with pytest.raises(ValueError, match="step="):
        SconeTable.opt_step_lean(None, ids, rows, kind="sgd", step=3, hyper=block)
    with pytest.raises(ValueError, match="lr="):
        SconeTable.opt_step_lean(None, ids, rows, kind="sgd", lr=0.1, hyper=block)
    with pytest.raises(ValueError, match="grad_scale="):
        SconeTable.grad_ctl(None, [1.0], grad_scale=1.0, hyper=block)
    with pytest.raises(ValueError, match="needs n="):
        SconeTable.opt_step(None, ids, rows, rows, kind="sgd", hyper=block)
    with pytest.raises(ValueError, match="lr is required"):
        SconeTable.opt_step(None, ids, rows, rows, kind="sgd")
    with pytest.raises(ValueError, match="capturable=True and fused_backward=True"):
        FGramOptimizer(object(), "sgd", fused_backward=True, capturable=True)
