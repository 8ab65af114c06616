"""`FGramOptimizer.step()` on its four roads leaves the same bits: the default road (the gradient on the module, every scalar by
value) is the reference; static mode (`static_rows=`: the `_dn` calls), `capturable=True` eagerly (the `_dh` calls, the row count
in a word the optimizer keeps) and `capturable=True` with `static_rows=` are held against it.

Every kind a module takes -- a master copy beside an INT8 table with sgd / adagrad / adam / rowwise_adagrad, fp32 and bf16 rows in
place with sgd / rowwise_adagrad, bf16 rows also with stochastic rounding -- as the plain step and as the step with `max_norm` and
`skip_nonfinite`.  Two steps each, 2 x 16 tokens on a 300-row table at d = 128; the served table's bytes, the master, `state1`,
`state2`, `t` and the control block are compared bit for bit, so there is no tolerance.  Nothing is captured here (the capture
tests are tests/test_gpu_backward_dn.py's and tests/test_gpu_opt_hyper.py's); the default road's result is computed once per kind
and shared."""

import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS, D, MAX_N, VOCAB, B, T = 300, 128, 3, 7, 2, 16
ROADS = {"static": dict(static=True, capturable=False), "capturable": dict(static=False, capturable=True),
         "capturable_static": dict(static=True, capturable=True)}
# name: (table format, a master copy?, kind, rounding, lr)
KINDS = {"int8-master-sgd": ("int8", True, "sgd", "nearest", 0.05),
         "int8-master-adagrad": ("int8", True, "adagrad", "nearest", 0.05),
         "int8-master-adam": ("int8", True, "adam", "nearest", 1e-3),
         "int8-master-rowwise_adagrad": ("int8", True, "rowwise_adagrad", "nearest", 0.05),
         "fp32-inplace-sgd": ("fp32", False, "sgd", "nearest", 0.05),
         "fp32-inplace-rowwise_adagrad": ("fp32", False, "rowwise_adagrad", "nearest", 0.05),
         "bf16-inplace-sgd": ("bf16", False, "sgd", "nearest", 0.05),
         "bf16-inplace-rowwise_adagrad": ("bf16", False, "rowwise_adagrad", "nearest", 0.05),
         "bf16-inplace-sgd-stochastic": ("bf16", False, "sgd", "stochastic", 0.05),
         "bf16-inplace-rowwise_adagrad-stochastic": ("bf16", False, "rowwise_adagrad", "stochastic", 0.05)}
STEPS = {"plain": (dict(), dict(grad_scale=0.5)),
         "clipped": (dict(max_norm=1.0, skip_nonfinite=True), dict(grad_scale=0.5, max_norm=1.0, skip_nonfinite=True))}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


@functools.lru_cache(maxsize=None)
def _inputs():
    """300 distinct f-grams over 7 tokens, the rows, and two batches of 2 x 16 tokens with their output gradients."""
    rng = np.random.default_rng(2025)
    grams = [g for n in range(1, MAX_N + 1) for g in itertools.product(range(VOCAB), repeat=n)]
    picked = [grams[i] for i in sorted(rng.choice(len(grams), size=N_ROWS, replace=False))]
    keys = np.zeros((N_ROWS, MAX_N), dtype=np.uint32)
    lens = np.array([len(g) for g in picked], dtype=np.uint8)
    for i, g in enumerate(picked):
        keys[i, :len(g)] = g
    w0 = rng.standard_normal((N_ROWS, D)).astype(np.float32)
    toks = [rng.integers(0, VOCAB, size=(B, T)).astype(np.int32) for _ in range(2)]
    grads = [rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(2)]
    return keys, lens, w0, toks, grads


def _run(kind_name, steps_name, static, capturable):
    """Two steps on fresh modules; what they leave, as bytes."""
    from scone_amd import EmbeddingCache, FGramOptimizer, InPlaceFGramTable, NGramExtractor, TrainableFGramTable
    fmt, with_master, kind, rounding, lr = KINDS[kind_name]
    keys, lens, w0, toks, grads = _inputs()
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=MAX_N), D, table_format=fmt)
    cache.cache_embeddings(list(range(N_ROWS)), torch.from_numpy(w0), verbose=False)
    kw = dict(static_rows=N_ROWS, max_tokens=B * T) if static else {}
    fg = TrainableFGramTable(cache, torch.from_numpy(w0.copy()), **kw) if with_master else InPlaceFGramTable(cache, **kw)
    opt = FGramOptimizer(fg, kind, lr=lr, weight_decay=0.01, rounding=rounding, seed=9, capturable=capturable)
    ctls, listed = [], []
    for tok, grad, step_kw in zip(toks, grads, STEPS[steps_name]):
        out = fg(torch.from_numpy(tok).cuda())
        out.backward(gradient=torch.from_numpy(grad).cuda().to(out.dtype))
        n = opt.step(**step_kw)
        listed.append(int(fg.static_grad[2].item()) if static else n)
        assert n == (N_ROWS if static else listed[-1])
        ctls.append(None if opt.last_ctl is None else {k: np.asarray(v).tobytes() for k, v in opt.last_ctl.read().items()})
        if step_kw.get("max_norm") is not None:
            assert 0 < float(opt.last_ctl.read()["coef"]) < 1 and not opt.found_nonfinite()
        opt.zero_grad()
    table = cache.to_device()
    rows, scales = table.download(0, N_ROWS)
    assert table.status() == 0 and not opt.rows_overflowed()
    return {"rows": rows.copy(), "scales": None if scales is None else scales.copy(),
            "master": fg.weight.detach().cpu().numpy() if with_master else None,
            "state1": None if opt.state1 is None else opt.state1.cpu().numpy(),
            "state2": None if opt.state2 is None else opt.state2.cpu().numpy(), "t": opt.t, "ctls": ctls, "listed": listed}


@functools.lru_cache(maxsize=None)
def _default_road(kind_name, steps_name):
    got = _run(kind_name, steps_name, static=False, capturable=False)
    assert min(got["listed"]) > 0 and got["t"] == 2
    return got


@pytest.mark.parametrize("steps_name", list(STEPS))
@pytest.mark.parametrize("kind_name", list(KINDS))
@pytest.mark.parametrize("road", list(ROADS))
def test_road_equals_the_default_road(road, kind_name, steps_name):
    kind = KINDS[kind_name][2]
    if kind == "adam":                                             # the precondition: both roads derive the same step size here
        from scone_amd.hip_backend import opt_hyper_scalars, opt_scalars
        for t in (1, 2):
            assert opt_hyper_scalars("adam", 1e-3, betas=(0.9, 0.999), step=t) == opt_scalars("adam", 1e-3, betas=(0.9, 0.999), step=t)
    want = _default_road(kind_name, steps_name)
    got = _run(kind_name, steps_name, **ROADS[road])
    assert got["t"] == want["t"] and got["listed"] == want["listed"] and got["ctls"] == want["ctls"]
    for name in ("rows", "scales", "master", "state1", "state2"):
        a, b = got[name], want[name]
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name} differs from the default road's"
    assert (want["state1"] is not None) == (kind == "adam") and (want["state2"] is not None) == (kind != "sgd")
