"""The backward of the dense side on the GPU (include/scone_hip.h, "backward of the dense side"): index plans, the lookup's
default positions, the no-plan `scone_backward_wpe`, and `wte` / `wpe` trained through the modules of scone_amd/training.py and
through `SconeEmbedding`.

No expectation passes through HIP code.  An index plan is the backward plan of one-element lists, so what it must give is
tests/backward_fixture.py's `backward_rows(off = arange, ids = idx, ...)` on the kept positions
(tests/test_dense_backward_host.py::index_rows, which also shows on the CPU that the batches used here tell the contract's
summation order from a backwards walk and from an unchunked sum).  Bits are compared with `edge_fixture.same_bits`; output
buffers carry 64 guard rows (NaN / -7) that must stay untouched, and `table.status()` must be 0.

Against fp64 the bound is the one tests/test_backward_host.py derives: an fp32 sum of n terms is within
(n + 2) * 2^-24 * sum |c| of the exact sum.

Shapes: the packed batches "small" (2,961 tokens: every token row has several chunks) and "tiny" (61) of
tests/test_gpu_varlen.py, constructed ids with exactly 1 / C / C + 1 / 3C + 5 references, rectangles around C batch rows, and
the 3 x 13 batch of tests/embed_rows_fixture.py for the modules; d = 64 (one column tile) and 776 (the last column tile partial).
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import embed_rows_fixture as ER  # noqa: E402
import stream_fixture as SF  # noqa: E402
import test_dense_backward_host as DH  # noqa: E402  (index_rows: the fixture on one-element lists)
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, bit views)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
GUARD = 64
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
DIMS = (64, 776)
MAX_N, B, T = 3, 3, 13
N_POS = 24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _L():
    from scone_amd import _lib
    return _lib


def _chunk():
    return int(_L().lib().scone_backward_chunk())


def _table(d, n_rows=40, mode="cover"):
    """A handle whose table has nothing to do with the id spaces below: 40 rows, no index."""
    from scone_amd.hip_backend import SconeTable
    return SconeTable(MAX_N, n_rows, dim=d, table_format="fp32", lookup_mode=mode)


def _grad(ntok, d, dtype, seed=0):
    """(device tensor in `dtype`, the same values as fp32 numpy)."""
    g = torch.from_numpy(np.random.default_rng(900 + seed).standard_normal((ntok, d)).astype(np.float32)).to(DTYPES[dtype])
    return g.cuda(), g.float().numpy()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _cur():
    return torch.cuda.current_stream().cuda_stream


def _guarded_rows(plan, g, reduce="sum"):
    """plan.rows into buffers with GUARD rows of NaN / -7 behind the U the plan reports; the guards must stay."""
    U, d = plan.n_rows, g.shape[-1]
    ids = torch.full((U + GUARD,), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((U + GUARD, d), float("nan"), dtype=torch.float32, device="cuda")
    got_ids, got_rows = plan.rows(g, reduce, out=(ids, rows))
    torch.cuda.synchronize()
    assert (ids[U:] == -7).all() and torch.isnan(rows[U:]).all(), "guard rows were written"
    return got_ids.cpu().numpy(), got_rows.cpu().numpy()


def _check_plan(t, idx, n_ids, g, g32, skip=None):
    """Plan, row ids, rows (both reduces), counts and the host counts against the fixture; status 0."""
    want_ids, want_rows, K = DH.index_rows(idx, g32, n_ids, skip, C_=_chunk())
    idx_t = torch.from_numpy(np.asarray(idx, dtype=np.int32)).cuda()
    skip_t = None if skip is None else torch.from_numpy(np.asarray(skip, dtype=np.int32)).cuda()
    with t.backward_plan_index(idx_t, n_ids, skip=skip_t) as plan:
        assert (plan.n_rows, plan.n_refs, plan.ntok) == (len(want_ids), int(K.sum()), len(K))
        assert np.array_equal(plan.row_ids().cpu().numpy(), want_ids)
        assert np.array_equal(plan.counts().cpu().numpy(), K)
        for reduce in ("sum", "mean"):
            ids, rows = _guarded_rows(plan, g, reduce)
            assert np.array_equal(ids, want_ids)
            assert E.same_bits(rows, want_rows), f"{reduce}: {E.first_difference(rows, want_rows)}"
    assert t.status() == 0
    return want_ids, want_rows


# ------------------------------------------------------------------ 1. index plans
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("batch", ["small", "tiny"])
def test_index_plan_against_the_fixture(batch, dtype, d):
    tok = VL._batch(batch)[0]
    g, g32 = _grad(len(tok), d, dtype)
    ids, _ = _check_plan(_table(d), tok, VL.VOCAB + 1, g, g32)
    if batch == "small":
        assert len(ids) == 4 and (np.bincount(tok) > _chunk()).all()          # every row takes the partials road


def test_constructed_reference_counts_and_ids_out_of_range():
    """Rows with exactly 1, C, C + 1 and 3C + 5 references, interleaved, between ids -1, n_ids and n_ids + 5."""
    c, n_ids, d = _chunk(), 9, 64
    counts = {7: 1, 2: c, 5: c + 1, 0: 3 * c + 5}
    idx = np.concatenate([np.full(n, i) for i, n in counts.items()] + [np.array([-1, n_ids, n_ids + 5, -1, n_ids])])
    np.random.default_rng(4).shuffle(idx)
    g, g32 = _grad(len(idx), d, "fp32", seed=1)
    ids, rows = _check_plan(_table(d), idx, n_ids, g, g32)
    assert ids.tolist() == [0, 2, 5, 7]
    for wrong in (dict(reverse=True), dict(chunked=False)):                   # the 3C + 5 row pins the order
        assert not E.same_bits(DH.index_rows(idx, g32, n_ids, C_=c, **wrong)[1], rows)


@pytest.mark.parametrize("n_ids", [50257, 1])
def test_id_space_is_independent_of_the_table(n_ids):
    """50,257 ids with references up to 50,256 on a table of 40 rows; and an id space of one id."""
    d = 64
    rng = np.random.default_rng(n_ids)
    idx = rng.integers(0, n_ids, size=700) if n_ids > 1 else rng.integers(-1, 2, size=300)
    if n_ids > 1:
        idx[[3, 500]] = n_ids - 1
        idx[9] = n_ids
    g, g32 = _grad(len(idx), d, "fp16", seed=2)
    ids, _ = _check_plan(_table(d), idx, n_ids, g, g32)
    assert ids[-1] == n_ids - 1


def test_skip_mask():
    """The mask removes id 1 entirely and part of id 2."""
    d, n_ids = 64, 4
    idx = np.random.default_rng(8).integers(0, n_ids, size=500)
    skip = np.zeros(len(idx), dtype=np.int32)
    skip[idx == 1] = 3
    two = np.flatnonzero(idx == 2)
    skip[two[::2]] = 1
    g, g32 = _grad(len(idx), d, "fp32", seed=3)
    ids, _ = _check_plan(_table(d), idx, n_ids, g, g32, skip)
    assert ids.tolist() == [0, 2, 3]


def test_empty_plans_and_refusals():
    L = _L()
    lib = L.lib()
    d = 64
    t = _table(d)
    g, _ = _grad(5, d, "fp32")
    with t.backward_plan_index(torch.zeros(0, dtype=torch.int32), 4) as plan:                       # ntok == 0
        assert (plan.n_rows, plan.n_refs) == (0, 0) and plan.row_ids().numel() == 0
        assert plan.rows(g[:0])[1].shape == (0, d)
    idx = torch.tensor([1, 2, 2, 9, -4], dtype=torch.int32).cuda()
    with t.backward_plan_index(idx, 4, skip=torch.ones(5, dtype=torch.int32)) as plan:              # all skipped: U == 0
        assert (plan.n_rows, plan.n_refs) == (0, 0) and plan.counts().cpu().tolist() == [0] * 5
        assert plan.rows(g)[0].numel() == 0
    with t.backward_plan_index(idx, 4) as plan:
        assert plan.n_rows == 2
        ids = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        rows = torch.full((1, d), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.scone_backward_rows(t._h, plan._p, _ptr(g), L.DT_F32, L.REDUCE_SUM, _ptr(ids), _ptr(rows), 1, _cur())
        assert rc == L.ERANGE                                                                       # rows_cap < U
        torch.cuda.synchronize()
        assert ids.item() == -7 and torch.isnan(rows).all()
        cfg = L.LeanCfg()
        cfg.struct_size, cfg.kind, cfg.lr, cfg.eps, cfg.grad_scale, cfg.step = C.sizeof(L.LeanCfg), L.LEAN_SGD, 0.1, 1e-10, 1.0, 1
        rc = lib.scone_backward_apply_lean(t._h, plan._p, _ptr(g), L.DT_F32, L.REDUCE_SUM, C.byref(cfg), None, _cur())
        assert rc == L.EINVAL and b"index plan" in lib.scone_last_error(t._h)
    p, n = C.c_void_p(), C.c_uint64(0)

    def refused(h, idx_p, ntok, n_ids):
        return lib.scone_backward_plan_index(h, idx_p, ntok, n_ids, None, C.byref(p), C.byref(n), C.byref(n), _cur())
    assert refused(t._h, None, 5, 4) == L.EINVAL                                                    # null d_idx
    for bad in (0, -3, 2 ** 32 - 1, 2 ** 33):
        assert refused(t._h, _ptr(idx), 5, bad) == L.EINVAL and b"n_ids" in lib.scone_last_error(t._h)
    assert refused(t._h, _ptr(idx), 2 ** 32, 4) == L.EINVAL and refused(t._h, _ptr(idx), -1, 4) == L.EINVAL
    assert p.value is None
    from scone_amd.hip_backend import SconeTable
    t12 = SconeTable(MAX_N, 40, dim=12, table_format="fp32")                                        # d % 8 != 0
    assert refused(t12._h, _ptr(idx), 5, 4) == L.EINVAL
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    assert lib.scone_backward_wpe(t12._h, _ptr(g), L.DT_F32, 1, 5, 4, _ptr(out), None, _cur()) == L.EINVAL
    assert lib.scone_backward_wpe(t._h, _ptr(g), 99, 1, 5, 4, _ptr(out), None, _cur()) == L.EINVAL   # bad grad_dtype
    assert lib.scone_backward_wpe(t._h, _ptr(g), L.DT_F32, 1, 5, 0, _ptr(out), None, _cur()) == L.EINVAL
    assert lib.scone_backward_wpe(t._h, None, L.DT_F32, 1, 5, 4, _ptr(out), None, _cur()) == L.EINVAL
    assert lib.scone_backward_wpe(t._h, None, L.DT_F32, 0, 5, 4, None, None, _cur()) == L.OK          # B * T == 0: a no-op
    assert lib.scone_backward_default_positions(t._h, None, 0, 0, 5, _ptr(idx), _cur()) == L.EINVAL  # a rectangle with T == 0
    assert lib.scone_backward_default_positions(t._h, None, 0, 2, 5, _ptr(idx), _cur()) == L.EINVAL  # 5 % 2 != 0
    torch.cuda.synchronize()
    assert (out == 0).all() and idx.cpu().tolist() == [1, 2, 2, 9, -4]                               # no device work
    assert t.status() == 0


# ------------------------------------------------------------------ 2. default positions
def test_default_positions():
    t = _table(64)
    assert np.array_equal(t.default_positions(5, 7).cpu().numpy(), np.arange(35) % 7)
    assert t.default_positions(0, 7).numel() == 0
    for batch in ("tiny", "small"):
        _, cu, _ = VL._batch(batch)
        want = VL._default_positions(cu)
        for cu_in in (cu.tolist(), torch.from_numpy(cu.astype(np.int32)).cuda()):
            got = t.default_positions(cu_seqlens=cu_in, total=int(cu[-1]))
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), batch
    assert t.status() == 0


# ------------------------------------------------------------------ 3. scone_backward_wpe
def _wpe_shapes():
    c = 128                                   # asserted equal to scone_backward_chunk() in the test
    return [(2 * c + 5, 3, 3), (c + 1, 2, 64), (c, 5, 64), (1, 37, 64), (2, 37, 20)]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("Bz,Tz,n_pos", _wpe_shapes(), ids=lambda v: str(v))
def test_backward_wpe_against_the_fixture_and_the_index_road(Bz, Tz, n_pos, dtype, d):
    """Row t sums g[b * T + t] for b ascending; rows t >= n_pos do not exist.  The scratch has exactly the queried size and
    starts as NaN; the output carries guard rows."""
    L = _L()
    lib = L.lib()
    c = _chunk()
    assert c == 128 and (Bz, Tz) in {(2 * c + 5, 3), (c + 1, 2), (c, 5), (1, 37), (2, 37)}
    t = _table(d)
    g, g32 = _grad(Bz * Tz, d, dtype, seed=Bz)
    rows_n = min(Tz, n_pos)
    pos = np.arange(Bz * Tz) % Tz
    want_ids, want, _ = DH.index_rows(pos, g32, n_pos, C_=c)
    assert np.array_equal(want_ids, np.arange(rows_n))
    need = L.backward_wpe_scratch(Bz, Tz, d)
    assert (need > 0) == (Bz > c)
    scratch = torch.full((need // 4,), float("nan"), dtype=torch.float32, device="cuda") if need else None
    out = torch.full((rows_n + GUARD, d), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.scone_backward_wpe(t._h, _ptr(g), L.DT_F32 if dtype == "fp32" else (L.DT_F16 if dtype == "fp16" else L.DT_BF16),
                                Bz, Tz, n_pos, _ptr(out), _ptr(scratch), _cur())
    assert rc == L.OK
    torch.cuda.synchronize()
    assert torch.isnan(out[rows_n:]).all(), "guard rows were written"
    got = out[:rows_n].cpu().numpy()
    assert E.same_bits(got, want), E.first_difference(got, want)
    # the wrapper (which holds its scratch) and the index-plan road: the same bits
    assert E.same_bits(t.backward_wpe(g.view(Bz, Tz, d), n_pos).cpu().numpy(), want)
    with t.backward_plan_index(t.default_positions(Bz, Tz), n_pos) as plan:
        ids, rows = plan.rows(g, "sum")
        assert np.array_equal(ids.cpu().numpy(), want_ids) and E.same_bits(rows.cpu().numpy(), got)
    assert t.status() == 0


# ------------------------------------------------------------------ 4. the modules
def _cache(d, mode, w):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = WS._vocabulary(MAX_N)
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=MAX_N), d, table_format="fp32", lookup_mode=mode)
    cache.cache_embeddings(list(range(len(lens))), torch.from_numpy(w), verbose=False)
    return cache


CU = np.array([0, 5, 5, 20, 39], dtype=np.int64)          # the 39 tokens as a packed batch, one sequence empty


def _world(d, pdtype, positions, seed=0):
    """The 3 x 13 batch, parameters in `pdtype`, grad_out in `pdtype`, and what the lookup is called with."""
    keys, lens, tok = ER.batch(MAX_N, B, T)
    rng = np.random.default_rng(70 + seed)
    w = rng.standard_normal((len(lens), d)).astype(np.float32)
    wte = torch.from_numpy(rng.standard_normal((VL.VOCAB + 1, d)).astype(np.float32)).to(pdtype).cuda()
    wpe = torch.from_numpy(rng.standard_normal((N_POS, d)).astype(np.float32)).to(pdtype).cuda()
    g = torch.from_numpy(rng.standard_normal((B * T, d)).astype(np.float32)).to(pdtype).cuda()
    cu = CU if positions == "packed" else None
    tok_in = torch.from_numpy(tok.reshape(-1) if cu is not None else tok)
    if positions == "explicit":
        pid = rng.integers(0, N_POS, size=(B, T))
        pid_in = torch.from_numpy(pid)
    else:
        pid, pid_in = ER.default_positions(tok.reshape(-1) if cu is not None else tok, cu), None
    g = g if cu is not None else g.view(B, T, d)
    return keys, lens, tok, w, wte, wpe, g, cu, tok_in, np.asarray(pid).reshape(-1), pid_in


def _dense_want(keys, lens, tok, cu, pid, g32, mode, pdtype):
    """(grad_wte, grad_wpe) as dense tensors of `pdtype`, from the fixture alone."""
    c = _chunk()
    skip = None
    if mode == "longest_suffix":                           # a matched f-gram replaced the token term
        off, _ = ER.paper_lists(keys, lens, MAX_N, tok.reshape(-1) if cu is not None else tok, cu)
        skip = np.diff(off)
        assert (skip == 0).any() and (skip == 1).any(), "the batch must have matched and unmatched positions"
    out = []
    for idx, n_ids, sk in ((tok.reshape(-1), VL.VOCAB + 1, skip), (pid, N_POS, None)):
        ids, rows, _ = DH.index_rows(idx, g32, n_ids, sk, C_=c)
        dense = np.zeros((n_ids, g32.shape[1]), dtype=np.float32)
        dense[ids] = rows
        out.append(torch.from_numpy(dense).to(pdtype))
    return out


def _run_module(kind, cache, w, tok_in, cu, kwargs, g, sparse=False):
    """One forward + backward through module `kind`; returns (y, the table gradient as (ids, rows))."""
    from scone_amd import InPlaceFGramTable, TrainableFGramTable
    cu_kw = {} if cu is None else dict(cu_seqlens=cu.tolist())
    if kind == "trainable":
        m = TrainableFGramTable(cache, torch.from_numpy(w.copy()), sparse_wte_grad=sparse)
        y = m(tok_in, out_dtype=g.dtype, **cu_kw, **kwargs)
        y.backward(g)
        return y, (m.weight.grad._indices()[0], m.weight.grad._values())
    if kind == "in_place":
        m = InPlaceFGramTable(cache, sparse_wte_grad=sparse)
        y = m(tok_in, out_dtype=g.dtype, **cu_kw, **kwargs)
        y.backward(g)
        return y, m.grad
    with cache.live_rows(tok_in, **cu_kw) as lb:
        rows = torch.from_numpy(w[lb.row_ids.cpu().numpy()]).cuda().requires_grad_()
        y = lb.embed(rows, out_dtype=g.dtype, **kwargs, **(dict(sparse_wte_grad=True) if sparse else {}))
        y.backward(g)
        return y, (lb.row_ids, rows.grad)


@pytest.mark.parametrize("positions", ["default", "explicit", "packed"])
@pytest.mark.parametrize("pdtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mode", ["cover", "longest_suffix"])
@pytest.mark.parametrize("kind", ["trainable", "in_place", "live"])
def test_modules_train_wte_and_wpe(kind, mode, pdtype, positions):
    d = 64
    keys, lens, tok, w, wte, wpe, g, cu, tok_in, pid, pid_in = _world(d, pdtype, positions)
    cache = _cache(d, mode, w)
    want_wte, want_wpe = _dense_want(keys, lens, tok, cu, pid, g.float().cpu().numpy().reshape(-1, d), mode, pdtype)
    pos_kw = {} if pid_in is None else dict(position_ids=pid_in)
    P_wte, P_wpe = wte.clone().requires_grad_(), wpe.clone().requires_grad_()
    y, table_grad = _run_module(kind, cache, w, tok_in, cu, dict(wte=P_wte, wpe=P_wpe, **pos_kw), g)
    serve = cache.embed_tokens(tok_in, wte=wte, wpe=wpe, **({} if cu is None else dict(cu_seqlens=cu.tolist())), **pos_kw)
    assert y.dtype == pdtype and E.same_bits(WS._bits(y.detach()), WS._bits(serve)), "the forward's bits changed"
    assert P_wte.grad.dtype == pdtype and not P_wte.grad.is_sparse and tuple(P_wte.grad.shape) == tuple(wte.shape)
    assert E.same_bits(WS._bits(P_wte.grad), WS._bits(want_wte)), "grad_wte"
    assert P_wpe.grad.dtype == pdtype and tuple(P_wpe.grad.shape) == tuple(wpe.shape)
    assert E.same_bits(WS._bits(P_wpe.grad), WS._bits(want_wpe)), "grad_wpe"
    # the table's own gradient: what the same batch and grad_out give with base=
    base = torch.zeros_like(g)
    _, base_grad = _run_module(kind, cache, w, tok_in, cu, dict(base=base), g)
    assert np.array_equal(table_grad[0].cpu().numpy(), base_grad[0].cpu().numpy())
    assert E.same_bits(table_grad[1].cpu().numpy(), base_grad[1].cpu().numpy()), "the table gradient changed"
    assert cache.table.status() == 0


@pytest.mark.parametrize("kind", ["trainable", "in_place", "live"])
def test_sparse_wte_grad_option(kind):
    d, mode = 64, "longest_suffix"
    keys, lens, tok, w, wte, wpe, g, cu, tok_in, pid, _ = _world(d, torch.float32, "default", seed=1)
    cache = _cache(d, mode, w)
    want_wte, _ = _dense_want(keys, lens, tok, cu, pid, g.cpu().numpy().reshape(-1, d), mode, torch.float32)
    P = wte.clone().requires_grad_()
    _run_module(kind, cache, w, tok_in, cu, dict(wte=P, wpe=wpe), g, sparse=True)
    sp = P.grad
    assert sp.is_sparse and sp.is_coalesced() and tuple(sp.shape) == tuple(wte.shape)
    ids = sp._indices()[0].cpu().numpy()
    assert np.array_equal(ids, np.flatnonzero(np.abs(want_wte.numpy()).sum(1) > 0))
    assert E.same_bits(sp._values().cpu().numpy(), want_wte.numpy()[ids])


def test_refusals_of_the_modules():
    from scone_amd import InPlaceFGramTable, TrainableFGramTable
    d = 64
    keys, lens, tok, w, wte, wpe, g, cu, tok_in, pid, _ = _world(d, torch.float32, "default")
    cache = _cache(d, "cover", w)
    P = wte.clone().requires_grad_()
    for m in (TrainableFGramTable(cache, torch.from_numpy(w.copy()), static_rows=64, max_tokens=B * T),
              InPlaceFGramTable(cache, static_rows=64, max_tokens=B * T)):
        with pytest.raises(ValueError, match="static_rows="):
            m(tok_in, wte=P, wpe=wpe)                                      # static mode trains the table only
        assert m(tok_in, wte=wte, wpe=wpe).requires_grad                   # detached wte / wpe: as before
    m = TrainableFGramTable(cache, torch.from_numpy(w.copy()))
    with pytest.raises(ValueError, match="base="):
        m(tok_in, wte=P, base=g)
    with cache.live_rows(tok_in) as lb:
        rows = torch.zeros((len(lb), d), device="cuda", requires_grad=True)
        with pytest.raises(ValueError, match="base="):
            lb.embed(rows, wte=P, base=g)


# ------------------------------------------------------------------ 5. against fp64
def test_against_fp64_and_the_stock_road():
    """fp32 parameters, cover mode: the gradients against `backward_rows_f64` on the one-element lists, and against torch
    autograd on wte(ids) + fg + wpe(pos) in fp64 (fg does not depend on either), both within (refs + 2) u sum |c|."""
    from scone_amd import TrainableFGramTable
    d = 64
    keys, lens, tok, w, wte, wpe, g, cu, tok_in, pid, _ = _world(d, torch.float32, "default", seed=2)
    cache = _cache(d, "cover", w)
    P_wte, P_wpe = wte.clone().requires_grad_(), wpe.clone().requires_grad_()
    TrainableFGramTable(cache, torch.from_numpy(w.copy()))(tok_in, wte=P_wte, wpe=P_wpe).backward(g)
    g32 = g.cpu().numpy().reshape(-1, d)
    w64, p64 = wte.double().requires_grad_(), wpe.double().requires_grad_()
    fg = cache.embed_tokens(tok_in).double()
    ids_t = torch.from_numpy(tok).cuda()
    stock = torch.nn.functional.embedding(ids_t, w64) + fg + torch.nn.functional.embedding(torch.from_numpy(pid).cuda().view(B, T), p64)
    stock.backward(g.double())
    worst = 0.0
    for got, idx, n_ids, stock_grad in ((P_wte.grad, tok.reshape(-1), VL.VOCAB + 1, w64.grad), (P_wpe.grad, pid, N_POS, p64.grad)):
        off = np.arange(len(idx) + 1)
        rid, sums, mags, refs = BW.backward_rows_f64(off, idx, g32, "sum", n_rows=n_ids)
        bound = (refs[:, None] + 2) * U32 * mags
        got64 = got.double().cpu().numpy()
        err = np.abs(got64[rid] - sums)
        assert (err <= bound).all()
        assert (np.abs(got64[rid] - stock_grad.cpu().numpy()[rid]) <= bound).all()
        untouched = np.setdiff1d(np.arange(n_ids), rid)
        assert (got64[untouched] == 0).all()
        worst = max(worst, err.max())
    assert worst > 0, "fp32 sums of ten references that equal the fp64 sums everywhere: the comparison compares nothing"


# ------------------------------------------------------------------ 6. SconeEmbedding
def _scone_embedding(d, mode, seed=3):
    from scone_amd.models.language_model import SconeEmbedding
    keys, lens, tok, w, wte, wpe, g, cu, tok_in, pid, _ = _world(d, torch.float32, "default", seed=seed)
    cache = _cache(d, mode, w)
    e_wte, e_wpe = torch.nn.Embedding(VL.VOCAB + 1, d).cuda(), torch.nn.Embedding(N_POS, d).cuda()
    with torch.no_grad():
        e_wte.weight.copy_(wte)
        e_wpe.weight.copy_(wpe)
    return SconeEmbedding(e_wte, e_wpe, None, cache), cache, (keys, lens, tok, g, pid)


@pytest.mark.parametrize("mode", ["cover", "longest_suffix"])
def test_scone_embedding_trains_its_embeddings(mode):
    """With a cache attached, forward(ids).backward(g) leaves the fixture's gradients on wte.weight and wpe.weight.  Before
    this change the lookup was given detached weights: the output did not require grad and this test fails."""
    d = 64
    emb, cache, (keys, lens, tok, g, pid) = _scone_embedding(d, mode)
    ids = torch.from_numpy(tok).cuda()
    y = emb(ids)
    assert y.requires_grad, "the fused road cut wte / wpe off the tape"
    want_y = cache.embed_tokens(ids, wte=emb.wte.weight.detach(), wpe=emb.wpe.weight.detach())
    assert E.same_bits(y.detach().cpu().numpy(), want_y.cpu().numpy())
    y.backward(g)
    want_wte, want_wpe = _dense_want(keys, lens, tok, None, pid, g.cpu().numpy().reshape(-1, d), mode, torch.float32)
    assert E.same_bits(emb.wte.weight.grad.cpu().numpy(), want_wte.numpy())
    assert E.same_bits(emb.wpe.weight.grad.cpu().numpy(), want_wpe.numpy())
    assert cache.table.status() == 0


def test_scone_embedding_inference_road_is_unchanged(monkeypatch):
    """Under no_grad, and with frozen embeddings, the call is the one made before: `embed_tokens` on detached weights, never
    the autograd road."""
    import scone_amd.training as TR
    d = 64
    emb, cache, (keys, lens, tok, g, pid) = _scone_embedding(d, "cover")
    ids = torch.from_numpy(tok).cuda()
    want = cache.embed_tokens(ids, wte=emb.wte.weight.detach(), wpe=emb.wpe.weight.detach()).cpu().numpy()

    def never(*a, **k):
        raise AssertionError("the inference road went through autograd")
    monkeypatch.setattr(TR, "embed_tokens_dense_grad", never)
    monkeypatch.setattr(TR._Lookup, "apply", never)
    calls = []
    real = cache.embed_tokens
    monkeypatch.setattr(cache, "embed_tokens", lambda *a, **k: (calls.append(sorted(k)), real(*a, **k))[1])
    with torch.no_grad():
        y = emb(ids)
    assert not y.requires_grad and y.grad_fn is None and E.same_bits(y.cpu().numpy(), want)
    emb.wte.weight.requires_grad_(False)
    emb.wpe.weight.requires_grad_(False)
    y = emb(ids)
    assert not y.requires_grad and E.same_bits(y.cpu().numpy(), want)
    assert calls == [["out_dtype", "position_ids", "reduce", "wpe", "wte"]] * 2


# ------------------------------------------------------------------ 7. stream order
# The section's prototypes spell their stream `void *stream`, so the table of tests/test_gpu_stream_order.py (which lists the
# `scone_stream_t` ones) does not hold them; this one does, with the header's sentence.
CONTRACT_DENSE = {
    "scone_backward_plan_index": (SF.S, "Synchronises the stream ONCE, to return U", "test_plan_index_synchronises_once"),
    "scone_backward_default_positions": (SF.A, "it does not synchronise and does not allocate", "test_no_sync_entry_points_are_stream_ordered"),
    "scone_backward_wpe": (SF.A, "it does not synchronise and allocates nothing", "test_no_sync_entry_points_are_stream_ordered"),
}


def test_every_entry_point_of_the_section_that_takes_a_stream_has_a_case():
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scone_hip.h")) as f:
        text = f.read()
    section = text[text.index("/* ---- backward of the dense side"):text.index("/* ---- optimizer hyper-parameters on the device")]
    protos = re.findall(r"^(?:int|void)\s+(scone_\w+)\s*\(([^;{}]*?)\)\s*;", section, flags=re.S | re.M)
    assert len(protos) == 4
    assert sorted(CONTRACT_DENSE) == sorted(name for name, args in protos if re.search(r"\bstream\b", args))
    for name, (klass, sentence, where) in CONTRACT_DENSE.items():
        assert sentence in " ".join(section.replace(" *", " ").split()) and callable(globals().get(where)), name


def _other_cu(cu):
    other = cu.copy()
    other[1:-1] = np.sort(np.random.default_rng(5).integers(0, cu[-1] + 1, size=len(cu) - 2))
    assert not np.array_equal(other, cu)
    return other


@pytest.mark.parametrize("entry", ["default_positions", "wpe_one_chunk", "wpe_partials"])
def test_no_sync_entry_points_are_stream_ordered(entry):
    """Class A of tests/stream_fixture.py: the call returns while the delay in front of it still runs, reads its inputs behind
    the copies queued on the stream, and its bits are the fixture's."""
    d = 64
    t = _table(d)
    stream = SF.side_stream(t)
    if entry == "default_positions":
        cu = VL._batch("tiny")[1].astype(np.int32)
        x = SF.Input(cu, _other_cu(cu).astype(np.int32))
        total = int(cu[-1])

        def call():
            return {"pos": t.default_positions(cu_seqlens=x.buf, total=total)}, None
        want = VL._default_positions(cu.astype(np.int64)).astype(np.int32)
    else:
        Bz, Tz = (7, 5) if entry == "wpe_one_chunk" else (_chunk() + 3, 2)
        g, g32 = _grad(Bz * Tz, d, "fp32", seed=11)
        x = SF.Input(g.view(Bz, Tz, d), _grad(Bz * Tz, d, "fp32", seed=12)[0].view(Bz, Tz, d))
        t.backward_wpe(x.truth, Tz)                        # the wrapper's scratch exists before the sequence

        def call():
            return {"pos": t.backward_wpe(x.buf, Tz)}, None
        want = DH.index_rows(np.arange(Bz * Tz) % Tz, g32, Tz, C_=_chunk())[1]
    res = SF.run(call, [x], stream=stream, table=t)
    SF.check_class(res, SF.A, entry)
    got = res.out["pos"]
    assert got.dtype == want.dtype and E.same_bits(got, want.reshape(got.shape)), entry
    assert res.status == 0


def test_plan_index_synchronises_once():
    """Class S: everything queued before it on the stream had completed when it returned, and U / n_refs are the fixture's."""
    d = 64
    t = _table(d)
    tok = VL._batch("tiny")[0].astype(np.int32)
    x = SF.Input(tok, ((tok + 1) % (VL.VOCAB + 1)).astype(np.int32))
    g, g32 = _grad(len(tok), d, "fp32", seed=13)
    want_ids, want_rows, K = DH.index_rows(tok, g32, VL.VOCAB + 1, C_=_chunk())
    plans = []

    def call():
        plan = t.backward_plan_index(x.buf, VL.VOCAB + 1)
        plans.append(plan)                                 # freeing a plan waits for the device: after the sequence
        ids, rows = plan.rows(g, "sum")
        return {"ids": ids, "rows": rows}, (plan.n_rows, plan.n_refs)
    res = SF.run(call, [x], stream=SF.side_stream(t), table=t)
    SF.check_class(res, SF.S, "backward_plan_index")
    assert res.host == (len(want_ids), int(K.sum())) and np.array_equal(res.out["ids"], want_ids)
    assert E.same_bits(res.out["rows"], want_rows) and res.status == 0
    for p in plans:
        p.close()
