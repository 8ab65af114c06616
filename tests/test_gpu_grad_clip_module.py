"""`FGramOptimizer.step(max_norm=, extra_sqnorm=, skip_nonfinite=)`, `grad_sqnorm()` and `found_nonfinite()` on both module kinds
(scone_amd/training.py; include/scone_hip.h, "gradient norm, clipping and skipped steps").

The clipped step must leave the bits of the same loop written by hand from its parts -- `grad_sqnorm`, `SconeTable.grad_ctl`, the
block's `coef` read back, and the PLAIN step given `fp32(grad_scale) * coef` -- so there is no tolerance anywhere.  Everything runs
on the WS vocabulary (max_n = 3, a few hundred rows), the 9 x 37 batch and d = 64.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only: the WS batches)
import test_gpu_opt_lean as TL  # noqa: E402  (helpers only: the cache builder)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies)

pytestmark = pytest.mark.gpu

MAX_N, D = 3, 64
LOSS_SCALE = 1024.0
SEED = 0x1234_5678_9ABC_DEF1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _tok():
    B, T = TB.RECTS["r37"]
    return torch.from_numpy(TB._batch("r37", MAX_N)[0].reshape(B, T)), B, T


def _make(which):
    """A module of the kind, its optimizer and a dense parameter (the base the lookup is added to)."""
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    n_rows = WS.N_ROWS[MAX_N]
    w0 = np.random.default_rng(41).standard_normal((n_rows, D)).astype(np.float32)
    tok, B, T = _tok()
    base = torch.from_numpy(np.random.default_rng(42).standard_normal((B, T, D)).astype(np.float16)).cuda().requires_grad_(True)
    if which == "adam":
        fg = TrainableFGramTable(TL._cache("int8", D, MAX_N, torch.from_numpy(w0)), torch.from_numpy(w0.copy()))
        opt = FGramOptimizer(fg, "adam", lr=0.05, weight_decay=0.01)
    else:
        fg = InPlaceFGramTable(TL._cache("bf16", D, MAX_N, torch.from_numpy(BF.stored(w0))))
        opt = FGramOptimizer(fg, "rowwise_adagrad", lr=0.05, eps=1e-10, weight_decay=0.01, rounding="stochastic", seed=SEED)
    return fg, opt, base, tok


def _backward(fg, base, tok, it, poison=False):
    """One loss-scaled backward: grad_out = LOSS_SCALE * a pattern of the iteration, in the output's dtype, fp16 (poison: one inf in it, at a
    position with f-gram hits)."""
    out = fg(tok, base=base)
    pattern = np.random.default_rng(100 + it).standard_normal(tuple(out.shape)).astype(np.float32)
    grad_out = (torch.from_numpy(pattern).cuda() * LOSS_SCALE).to(out.dtype)
    if poison:
        grad_out[3, 5, 7] = float("inf")
    base.grad = None
    out.backward(gradient=grad_out)
    return (base.grad.double() ** 2).sum()                        # the dense parameter's squared norm, at the same loss scale


def _snapshot(fg, opt):
    table = fg.cache.to_device()
    rows, scales = table.download(0, table.n_rows)
    out = [rows.copy(), None if scales is None else scales.copy()]
    out.append(fg.weight.detach().cpu().numpy().copy() if hasattr(fg, "weight") else None)
    out += [None if s is None else s.cpu().numpy().copy() for s in (opt.state1, opt.state2)]
    return out


def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and x.shape == y.shape
                                             and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def _loop(which, by_hand, max_norm=20.0, iters=3):
    fg, opt, base, tok = _make(which)
    table = fg.cache.to_device()
    history, coefs = [], []
    for it in range(1, iters + 1):
        extra = _backward(fg, base, tok, it)
        if by_hand:
            sq = opt.grad_sqnorm()
            ctl = table.grad_ctl([sq, extra], grad_scale=1.0 / LOSS_SCALE, max_norm=max_norm)
            coef = ctl.read()["coef"]
            n = opt.step(grad_scale=float(np.float32(1.0 / LOSS_SCALE) * np.float32(coef)))
            assert opt.last_ctl is None, "the plain step made a block"
        else:
            n = opt.step(grad_scale=1.0 / LOSS_SCALE, max_norm=max_norm, extra_sqnorm=extra)
            ctl = opt.last_ctl
            assert not opt.found_nonfinite()
        got = ctl.read()
        # the norm is the un-scaled one: the table's and the dense parameter's together
        rows = fg.grad[1] if which != "adam" else fg.weight.grad._values()
        want = np.sqrt(float((rows.double() ** 2).sum() + extra)) / LOSS_SCALE
        assert abs(float(got["norm"]) - want) <= 1e-5 * want and got["skip"] == 0
        coefs.append(float(got["coef"]))
        assert n > 0 and opt.t == it and table.status() == 0
        opt.zero_grad()
        history.append(_snapshot(fg, opt))
    return history, coefs


@pytest.mark.parametrize("which", ["adam", "in_place_stochastic"])
def test_clipped_loop_equals_the_loop_written_by_hand(which):
    fused, coefs = _loop(which, by_hand=False)
    assert all(0 < c < 1 for c in coefs), f"nothing was clipped: {coefs}"
    assert not _same(fused[0], fused[1]) and not _same(fused[1], fused[2])
    hand, hand_coefs = _loop(which, by_hand=True)
    assert coefs == hand_coefs
    for it, (x, y) in enumerate(zip(fused, hand), start=1):
        assert _same(x, y), f"iteration {it}: the clipped step differs from grad_sqnorm + grad_ctl + the plain step"
    again, _ = _loop(which, by_hand=False)
    assert all(_same(x, y) for x, y in zip(fused, again)), "two runs differ"


def test_a_large_max_norm_is_the_plain_step():
    clipped, coefs = _loop("adam", by_hand=False, max_norm=1e9, iters=2)
    assert coefs == [1.0, 1.0]
    fg, opt, base, tok = _make("adam")
    for it in (1, 2):
        _backward(fg, base, tok, it)
        opt.step(grad_scale=1.0 / LOSS_SCALE)
        opt.zero_grad()
        assert _same(_snapshot(fg, opt), clipped[it - 1])


@pytest.mark.parametrize("which", ["adam", "in_place_stochastic"])
def test_an_overflowed_backward_is_skipped_on_the_device(which):
    fg, opt, base, tok = _make(which)
    scratch_fg, scratch_opt, scratch_base, _ = _make(which)             # a scratch copy: it takes the unguarded step
    for f, o, b in ((fg, opt, base), (scratch_fg, scratch_opt, scratch_base)):
        _backward(f, b, tok, 1)
        o.step(grad_scale=1.0 / LOSS_SCALE, skip_nonfinite=True)
        assert not o.found_nonfinite()
        o.zero_grad()
    good = _snapshot(fg, opt)
    assert _same(good, _snapshot(scratch_fg, scratch_opt))
    extra = _backward(fg, base, tok, 2, poison=True)
    assert not bool(torch.isfinite(opt.grad_sqnorm()))
    assert opt.step(grad_scale=1.0 / LOSS_SCALE, max_norm=1.0, extra_sqnorm=extra, skip_nonfinite=True) > 0
    assert opt.found_nonfinite() and opt.last_ctl.read()["skip"] == 1
    assert opt.t == 2, "t advances on a device-skipped step: the host does not know the outcome"
    assert _same(_snapshot(fg, opt), good), "a skipped step changed the table, the master or the state"
    assert fg.cache.to_device().status() == 0
    # the bug the feature prevents, once: the same step without the guard writes NaN
    _backward(scratch_fg, scratch_base, tok, 2, poison=True)
    scratch_opt.step(grad_scale=1.0 / LOSS_SCALE)
    bad = _snapshot(scratch_fg, scratch_opt)
    assert not _same(bad, good)
    floats = [bad[2]] if which == "adam" else [BF.from_bf16_bits(BF.rows_as_bits(bad[0]))]
    assert any(np.isnan(x).any() for x in floats), "the unguarded step was expected to write NaN"
    # the next good step goes through
    opt.zero_grad()
    _backward(fg, base, tok, 3)
    opt.step(grad_scale=1.0 / LOSS_SCALE, skip_nonfinite=True)
    assert not opt.found_nonfinite() and not _same(_snapshot(fg, opt), good)


def test_grad_sqnorm_without_a_gradient_and_found_nonfinite_before_a_step():
    for which in ("adam", "in_place_stochastic"):
        fg, opt, base, tok = _make(which)
        sq = opt.grad_sqnorm()
        assert sq.dtype == torch.float64 and sq.dim() == 0 and sq.is_cuda and float(sq) == 0.0
        assert not opt.found_nonfinite() and opt.last_ctl is None
        assert opt.step(max_norm=1.0, skip_nonfinite=True) == 0 and opt.t == 0 and opt.last_ctl is None
        _backward(fg, base, tok, 1)
        rows = fg.grad[1] if which != "adam" else fg.weight.grad._values()
        want = float((rows.double() ** 2).sum())
        assert abs(float(opt.grad_sqnorm()) - want) <= 1e-12 * want


def test_fused_backward_refuses_the_clipping_arguments():
    from scone_amd import FGramOptimizer, InPlaceFGramTable
    w0 = torch.zeros((WS.N_ROWS[MAX_N], D))
    fg = InPlaceFGramTable(TL._cache("bf16", D, MAX_N, w0))
    opt = FGramOptimizer(fg, "sgd", lr=0.05, fused_backward=True)
    for kw in (dict(max_norm=1.0), dict(extra_sqnorm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="default road"):
            opt.step(**kw)
    assert opt.step() == 0 and opt.t == 0


def test_step_without_the_new_arguments_is_scone_opt_step():
    from scone_amd.hip_backend import SconeTable
    fg, opt, base, tok = _make("adam")
    n_rows = WS.N_ROWS[MAX_N]
    w0 = fg.weight.detach().clone()
    twin = SconeTable(MAX_N, n_rows, dim=D, table_format="int8")
    twin.store_f32(w0)
    m, v = torch.zeros_like(w0), torch.zeros_like(w0)
    for it in (1, 2):
        _backward(fg, base, tok, it)
        ids, rows = fg.weight.grad._indices()[0].clone(), fg.weight.grad._values().clone()
        assert opt.step(0.5) == ids.numel() and opt.last_ctl is None
        opt.zero_grad()
        twin.opt_step(ids, rows, w0, kind="adam", lr=0.05, step=it, state1=m, state2=v, weight_decay=0.01, grad_scale=0.5)
        assert torch.equal(fg.weight.detach(), w0) and torch.equal(opt.state1, m) and torch.equal(opt.state2, v)
        a, b = fg.cache.to_device().download(0, n_rows), twin.download(0, n_rows)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
