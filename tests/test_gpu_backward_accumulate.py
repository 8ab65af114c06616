"""The backward that accumulates (`scone_backward_rows_acc`, `BackwardPlan.rows(accumulate=)`, `BackwardPlan.row_ids`) against
the two calls it fuses, `BackwardPlan.rows` followed by `SconeTable.grad_merge(old, new)`: bit equality, no tolerance.  Then the
modules: micro-batch backwards onto a gradient that is there against the left fold of the numpy statements
(tests/backward_fixture.py folded by tests/grad_merge_fixture.py), the optimizer step and `commit()` after it, and the old
gradients that stay on `_add_coalesced`.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import grad_merge_fixture as GM  # noqa: E402
import lean_fixture as LF  # noqa: E402
import test_gpu_backward as TB  # noqa: E402  (helpers only: batches, their id lists, plans, gradients)
import test_gpu_backward_edges as GE  # noqa: E402  (helpers only: CSR lists)
import test_gpu_opt_lean as LT  # noqa: E402  (helpers only: scalars, the module's cache)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies)

pytestmark = pytest.mark.gpu

N = 48          # rows of the CSR tables
HOT = 5         # the row every position lists


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _table(d, n=N):
    from scone_amd.hip_backend import SconeTable
    return SconeTable(3, n, dim=d, table_format="fp32")


def _hot_lists(C):
    """2 C + 3 positions that all list row HOT (three chunks, the last of 3 references) next to rows of 1 .. 4 references; rows
    30 .. 39 are listed by nobody."""
    ntok = 2 * C + 3
    lists = [[HOT] for _ in range(ntok)]
    for r in range(6, 30):
        for k in range(1 + r % 4):
            lists[(7 * r + 11 * k) % ntok].append(r)
    lists[3] += [8, 8]                                          # an id three times in one list
    return GE._csr(lists)


def _old(d, ids, seed=0):
    ids = np.asarray(ids, dtype=np.int64)
    rows = np.random.default_rng(100 + seed).standard_normal((len(ids), d)).astype(np.float32)
    if rows.size:
        rows[::2, ::3] = -0.0
        rows[1::3, 1::5] = 1e-41
    return ids, rows


def _both_roads(table, plan_of, g_t, reduce, old, tag):
    """(ids, rows) of rows(accumulate=old), checked against rows() + grad_merge(old, new) bit for bit."""
    g = g_t.cuda()
    old_t = (torch.from_numpy(old[0]).cuda(), torch.from_numpy(old[1]).cuda())
    with plan_of(table) as plan:
        new_ids, new_rows = plan.rows(g, reduce)
        want_ids, want = table.grad_merge(old_t[0], old_t[1], new_ids, new_rows)
        assert torch.equal(plan.row_ids(), new_ids), f"{tag}: row_ids() is not rows()'s"
        got_ids, got = plan.rows(g, reduce, accumulate=old_t)
        again = plan.rows(g, reduce, accumulate=old_t)[1]
    assert torch.equal(got_ids, want_ids), f"{tag}: ids"
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{tag}: {E.first_difference(got, want)}"
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32)), f"{tag}: two runs differ"
    assert table.status() == 0, tag
    return got_ids.cpu().numpy(), got, new_ids.cpu().numpy()


def _csr_plan(off, ids):
    return lambda t: t.backward_plan_csr(torch.from_numpy(np.asarray(off)), torch.from_numpy(np.asarray(ids)))


# ------------------------------------------------------------------ 1. the two roads
@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("d", [8, 768, 4104])
def test_accumulate_equals_rows_then_merge(d, dtype, reduce):
    """old has the hot row (it takes the partial pass: old is added last), rows of one chunk, and rows nobody else has (0 .. 4 in
    front, 30 .. 33 inside, 47 behind); the plan has rows old does not."""
    C = TB._chunk()
    off, ids = _hot_lists(C)
    rid, lens = BW.row_lengths(off, ids)
    assert lens[rid == HOT][0] == 2 * C + 3 and (lens <= C).sum() >= 20
    old = _old(d, [0, 1, 2, 3, 4, HOT, 6, 9, 10, 17, 29, 30, 31, 32, 33, 47], seed=d)
    assert np.setdiff1d(old[0], rid).size and np.setdiff1d(rid, old[0]).size and HOT in old[0] and HOT in rid
    table = _table(d)
    g = TB._grad(len(off) - 1, d, dtype, seed=1)
    got_ids, got, _ = _both_roads(table, _csr_plan(off, ids), g, reduce, old, f"d{d}-{dtype}-{reduce}")
    if d == 8:                                                   # and against the numpy statements
        want_ids, want = GM.merge(old[0], old[1], *BW.backward_rows(off, ids, TB._g32(g), reduce, C, 0, None, N))
        assert np.array_equal(got_ids, want_ids) and GM.same_bits(got, want)
        only_old = np.isin(got_ids, np.setdiff1d(old[0], rid))
        assert np.array_equal(got[only_old].view(np.uint32), old[1][np.isin(old[0], got_ids[only_old])].view(np.uint32))


def test_an_empty_old_gradient_and_an_empty_plan():
    d, C = 264, TB._chunk()
    off, ids = _hot_lists(C)
    table = _table(d)
    g = TB._grad(len(off) - 1, d, "fp16", seed=2)
    got_ids, got, new_ids = _both_roads(table, _csr_plan(off, ids), g, "mean", _old(d, []), "old-empty")
    assert np.array_equal(got_ids, new_ids) and len(got_ids) > 20
    # U == 0: out is a copy of old
    empty = GE._csr([[] for _ in range(10)])
    old = _old(d, [1, 2, 40], seed=5)
    got_ids, got, new_ids = _both_roads(table, _csr_plan(*empty), TB._grad(10, d, "fp16"), "mean", old, "plan-empty")
    assert len(new_ids) == 0 and np.array_equal(got_ids, old[0]) and np.array_equal(got.view(np.uint32), old[1].view(np.uint32))
    # both empty
    got_ids, got, _ = _both_roads(table, _csr_plan(*empty), TB._grad(10, d, "fp16"), "sum", _old(d, []), "both-empty")
    assert got_ids.size == 0 and got.shape == (0, d)


@pytest.mark.parametrize("batch,max_n", [("small", 4), ("r37", 3)])
def test_token_plans(batch, max_n):
    """The packed (cu_seqlens) plan and a rectangle, matched by the library."""
    d = 200
    table = TB._table(max_n, d)
    tok, _ = TB._batch(batch, max_n)
    rid = BW.row_lengths(*TB._lists(batch, max_n, "cover"))[0]
    n = WS.N_ROWS[max_n]
    old_ids = np.union1d(rid[::3], np.setdiff1d(np.arange(n), rid)[:7])
    assert np.setdiff1d(old_ids, rid).size and np.setdiff1d(rid, old_ids).size
    got_ids, _, new_ids = _both_roads(table, lambda t: TB._plan(t, batch, max_n), TB._grad(len(tok), d, "bf16", seed=3), "mean",
                                      _old(d, old_ids, seed=7), f"{batch}")
    assert np.array_equal(new_ids, rid) and np.array_equal(got_ids, np.union1d(old_ids, rid))


def test_one_workgroup(monkeypatch):
    """SCONE_OPT_MAX_BLOCKS=1 (read at create) on the handle of the fused road: 4 waves walk ~300 rows of every kind."""
    from scone_amd.hip_backend import SconeTable
    d, n, C = 264, 400, TB._chunk()
    lists = [[p] if p < 150 else [] for p in range(2 * C + 40)]
    for p in range(3, 2 * C + 6):
        lists[p].append(399)
    off, ids = GE._csr(lists)
    old = _old(d, np.concatenate([np.arange(100, 300), [399]]), seed=9)
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "1")
    capped = SconeTable(3, n, dim=d, table_format="fp32")
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    g = TB._grad(len(off) - 1, d, "fp16", seed=4)
    ids_c, rows_c, _ = _both_roads(capped, _csr_plan(off, ids), g, "mean", old, "capped")
    ids_f, rows_f, _ = _both_roads(SconeTable(3, n, dim=d, table_format="fp32"), _csr_plan(off, ids), g, "mean", old, "free")
    assert len(ids_c) == 301 and np.array_equal(ids_c, ids_f) and np.array_equal(rows_c.view(np.uint32), rows_f.view(np.uint32))


def test_refusals():
    d = 64
    table, other = _table(d), _table(d)
    off, ids = _hot_lists(TB._chunk())
    g = TB._grad(len(off) - 1, d, "fp32").cuda()
    old = tuple(torch.from_numpy(x).cuda() for x in _old(d, [1, 2, 3]))
    with _csr_plan(off, ids)(table) as plan:
        with pytest.raises(ValueError):
            plan.rows(g, "mean", accumulate=(old[0], old[1].half()))
        with pytest.raises(ValueError):
            plan.rows(g, "mean", accumulate=(old[0][:2], old[1]))
        with pytest.raises(ValueError):
            plan.rows(g, "median", accumulate=old)
        with pytest.raises(ValueError):
            plan.rows(g, "mean", out=(old[0], old[1]), accumulate=old)
        ids_a, rows_a = plan.rows(g, "mean", accumulate=old)          # and the plan still works
        assert ids_a.numel() >= plan.n_rows and rows_a.shape == (ids_a.numel(), d)
    assert table.status() == 0 and other.status() == 0


# ------------------------------------------------------------------ 2. the modules
BATCHES = (("r37", 11), ("small", 12), ("r3", 13))


def _micro_batches(module, max_n, d, reduce="mean"):
    """Three backwards without zeroing in between; returns the fixture's rows of every micro-batch."""
    C, mode, out = TB._chunk(), module.cache.lookup_mode, []
    for batch, seed in BATCHES:
        tok, cu = TB._batch(batch, max_n)
        g = TB._grad(len(tok), d, "fp32", seed=seed)
        if batch in TB.RECTS:
            B, T = TB.RECTS[batch]
            module(torch.from_numpy(tok.reshape(B, T)), reduce=reduce).backward(g.reshape(B, T, d).cuda())
        else:
            module(torch.from_numpy(tok), cu_seqlens=cu, reduce=reduce).backward(g.cuda())
        out.append(BW.backward_rows(*TB._lists(batch, max_n, mode), TB._g32(g), reduce, C, 0, None, WS.N_ROWS[max_n]))
    return out


def _fold(parts):
    ids, rows = parts[0]
    for p in parts[1:]:
        ids, rows = GM.merge(ids, rows, *p)
    return ids, rows


@pytest.mark.parametrize("which", ["trainable", "in_place"])
def test_three_micro_batches_then_a_step(which):
    from scone_amd import FGramOptimizer, InPlaceFGramTable, TrainableFGramTable
    max_n, d = 4, 64
    n = WS.N_ROWS[max_n]
    w0 = np.random.default_rng(41).standard_normal((n, d)).astype(np.float32)
    if which == "trainable":
        cache = LT._cache("int8", d, max_n, torch.from_numpy(w0))
        module = TrainableFGramTable(cache, torch.from_numpy(w0.copy()))
        kind = "rowwise_adagrad"
    else:
        cache = LT._cache("fp32", d, max_n, torch.from_numpy(w0))
        module = InPlaceFGramTable(cache)
        kind = "sgd"
    parts = _micro_batches(module, max_n, d)
    want_ids, want = _fold(parts)
    assert len(want_ids) < sum(len(p[0]) for p in parts), "no row is touched twice"
    assert any(np.setdiff1d(want_ids, p[0]).size for p in parts), "every micro-batch touches every row"
    if which == "trainable":
        grad = module.weight.grad
        assert grad.is_sparse and grad.is_coalesced() and tuple(grad.shape) == (n, d)
        got_ids, got = grad._indices()[0].cpu().numpy(), grad._values().cpu().numpy()
        assert len(module._touched) == 3 and all(np.array_equal(t.cpu().numpy(), p[0]) for t, p in zip(module._touched, parts))
    else:
        got_ids, got = (x.cpu().numpy() for x in module.grad)
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), E.first_difference(got, want)
    # the step that follows: the bits of the numpy update
    gs = 1.0 / 3.0
    opt = FGramOptimizer(module, kind, lr=0.05, eps=1e-10)
    assert opt.step(grad_scale=gs) == len(want_ids)
    sc = LT._scalars(kind, gs=gs, lr=0.05, eps=1e-10)
    table = cache.to_device()
    if which == "trainable":
        neww, s, _, bad = LF.apply(kind, sc, want_ids, want, w0, np.zeros(n, dtype=np.float32))
        assert not bad and E.same_bits(module.weight.detach().cpu().numpy(), neww) and E.same_bits(opt.state2.cpu().numpy(), s)
        assert module.commit() == 0
    else:
        neww = LF.apply(kind, sc, want_ids, want, w0)[0]
        assert E.same_bits(table.download(0, n)[0].view(np.float32), neww)
    assert table.status() == 0


def test_commit_after_accumulation_stores_the_union_of_touched_rows():
    from scone_amd import TrainableFGramTable
    max_n, d = 4, 64
    n = WS.N_ROWS[max_n]
    w0 = torch.from_numpy(np.random.default_rng(42).standard_normal((n, d)).astype(np.float32))
    cache = LT._cache("fp16", d, max_n, w0)
    module = TrainableFGramTable(cache, w0.clone())
    parts = _micro_batches(module, max_n, d)
    union = _fold(parts)[0]
    torch.optim.SGD([module.weight], lr=0.5).step()
    assert module.commit() == len(union) and module.commit() == 0
    fresh = LT._cache("fp16", d, max_n, module.weight.detach().cpu())
    got, want = cache.to_device().download(0, n), fresh.to_device().download(0, n)
    assert np.array_equal(got[0], want[0]), "the served table is not a table built from the updated weights"
    stale = LT._cache("fp16", d, max_n, w0).to_device().download(0, n)[0]
    assert not np.array_equal(got[0][union], stale[union])


def test_a_gradient_set_by_hand_stays_on_add_coalesced():
    """A non-coalesced weight.grad (duplicates, unsorted) and an fp64 one are not the library's operands."""
    from scone_amd import TrainableFGramTable
    from scone_amd.training import _add_coalesced
    max_n, d = 3, 64
    n = WS.N_ROWS[max_n]
    w0 = torch.from_numpy(np.random.default_rng(43).standard_normal((n, d)).astype(np.float32))
    cache = LT._cache("fp32", d, max_n, w0)
    module = TrainableFGramTable(cache, w0.clone())
    B, T = TB.RECTS["r37"]
    tok = torch.from_numpy(TB._batch("r37", max_n)[0].reshape(B, T))
    g = TB._grad(B * T, d, "fp32", seed=5).reshape(B, T, d).cuda()
    hand_ids = torch.tensor([7, 2, 7, 40, 2], dtype=torch.int64, device="cuda")
    hand_rows = torch.from_numpy(np.random.default_rng(44).standard_normal((5, d)).astype(np.float32)).cuda()
    hand = torch.sparse_coo_tensor(hand_ids[None], hand_rows, (n, d))
    assert not hand.is_coalesced() and module._mergeable_grad() is None
    module.weight.grad = hand
    assert module._mergeable_grad() is None
    module(tok).backward(g)
    with cache.to_device().backward_plan(tok) as plan:
        want = _add_coalesced(hand, *plan.rows(g, "mean"))
    got = module.weight.grad
    assert got.is_coalesced() and torch.equal(got._indices(), want._indices())
    assert np.array_equal(got._values().cpu().numpy().view(np.uint32), want._values().cpu().numpy().view(np.uint32))
    assert module._mergeable_grad() is not None                    # ... and what it left is the library's operand
    module(tok).backward(g)
    with cache.to_device().backward_plan(tok) as plan:
        ids2, rows2 = cache.to_device().grad_merge(want._indices()[0], want._values(), *plan.rows(g, "mean"))
    assert torch.equal(module.weight.grad._indices()[0], ids2)
    assert np.array_equal(module.weight.grad._values().cpu().numpy().view(np.uint32), rows2.cpu().numpy().view(np.uint32))
    assert cache.to_device().status() == 0
