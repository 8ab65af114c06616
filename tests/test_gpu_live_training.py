"""Training an f-gram model THROUGH the lookup: `EmbeddingCache.live_rows` -> `LiveFGramBatch.embed` (autograd over
`scone_embed_rows` and the backward plan), `store` and `EmbeddingCache.bake`.

Bit-for-bit where the library owns the arithmetic: the gradient of `rows` is tests/backward_fixture.py's `backward_rows` on the
batch's CSR lists (cast to the rows' dtype), and equals the values of `TrainableFGramTable`'s sparse `weight.grad` on the same
batch; `grad_base` is what `_Lookup` gives.  Against an fp64 dense model `y = base + A @ rows` (A built from the oracle's
lists) the bound is the one tests/test_backward_host.py derives from `backward_rows_f64`: an fp32 sum of n terms t_i, each
rounded at most once more, is within (n + 2) * 2^-24 * sum |t_i| of the exact sum.  Where torch's fp32 matrix products join the
chain (the toy model), n is the longest chain of additions behind the element: the references of the batch plus the inner
dimensions of the products.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import embed_rows_fixture as ER  # noqa: E402
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, rounding)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24            # unit roundoff of fp32
MAX_N, B, T = 3, 3, 13


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _cache(fmt, d, mode="cover", rows=None, max_n=MAX_N, keys_lens=None):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = keys_lens or WS._vocabulary(max_n)
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt, lookup_mode=mode)
    if rows is None:
        rows = torch.zeros(len(lens), d)
    cache.cache_embeddings(list(range(len(lens))), rows, verbose=False)
    return cache


def _world(d, seed=0):
    keys, lens, tok = ER.batch(MAX_N, B, T)
    off, ids = ER.lists(keys, lens, MAX_N, tok)
    rng = np.random.default_rng(40 + seed)
    g = rng.standard_normal((B * T, d)).astype(np.float32)
    base = rng.standard_normal((B * T, d)).astype(np.float32)
    return keys, lens, tok, off, ids, np.unique(ids), g, base


def _dense_A(off, ids, live, reduce="mean"):
    """fp64 [ntok, U]: y = base + A @ rows is the cover-mode lookup."""
    ntok = len(off) - 1
    A = np.zeros((ntok, len(live)))
    slot = {int(r): u for u, r in enumerate(live)}
    for p in range(ntok):
        K = off[p + 1] - off[p]
        for r in ids[off[p]:off[p + 1]]:
            A[p, slot[int(r)]] += 1.0 / K if reduce == "mean" else 1.0
    return A


@pytest.mark.parametrize("mode", ["cover", "longest_suffix"])
@pytest.mark.parametrize("rows_dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_row_and_base_gradients_bit_for_bit(mode, rows_dtype, reduce):
    from scone_amd import _lib, LiveFGramBatch
    d = 64
    keys, lens, tok, off, ids, live, g, base = _world(d)
    if mode == "longest_suffix":                                    # the plan of such a handle holds the paper's lists
        off, ids = ER.paper_lists(keys, lens, MAX_N, tok)
        live = np.unique(ids)
        assert 0 < len(live) and (np.diff(off) == 0).any() and (np.diff(off) == 1).any()
    cache = _cache("fp32", d, mode)
    with cache.live_rows(torch.from_numpy(tok)) as lb:
        assert isinstance(lb, LiveFGramBatch) and len(lb) == len(live)
        assert np.array_equal(lb.row_ids.cpu().numpy(), live)
        assert np.array_equal(lb.lens.cpu().numpy(), lens[live].astype(np.int64))
        assert np.array_equal(lb.tokens.cpu().numpy(), keys[live].astype(np.int64))
        assert lb.tokens.dtype == torch.int64 and cache.f_gram_keys()[0] is cache.f_gram_keys()[0]
        rows = torch.from_numpy(np.random.default_rng(1).standard_normal((len(live), d)).astype(np.float32)).to(rows_dtype).cuda()
        rows.requires_grad_()
        base_t = torch.from_numpy(base).cuda().requires_grad_()
        g_t = torch.from_numpy(g).cuda()
        y = lb.embed(rows, base=base_t, reduce=reduce)
        assert tuple(y.shape) == (B, T, d) and y.dtype == torch.float32
        want_y = ER.expected(keys, lens, MAX_N, len(lens), tok, None, live, ER.widen(rows), mode, reduce, base32=base)
        assert E.same_bits(y.detach().cpu().numpy().reshape(B * T, d), want_y)
        y.backward(g_t.view(B, T, d))
        rid, want = BW.backward_rows(off, ids, g, reduce, _lib.lib().scone_backward_chunk())
        assert np.array_equal(rid, live)
        assert rows.grad.dtype == rows_dtype and tuple(rows.grad.shape) == (len(live), d)
        assert E.same_bits(WS._bits(rows.grad), WS._bits(torch.from_numpy(want).to(rows_dtype)))
        k = lb.plan.counts().cpu().numpy()
        assert np.array_equal(k, np.diff(off))
        want_base = g if mode == "cover" else g * (k == 0)[:, None].astype(np.float32)
        assert E.same_bits(base_t.grad.cpu().numpy(), want_base)
        # a second call on the same batch, without base: the gradient accumulates as autograd adds it
        first = rows.grad.clone()
        lb.embed(rows, reduce=reduce).backward(g_t.view(B, T, d))
        assert E.same_bits(WS._bits(rows.grad), WS._bits(first + first))
    assert cache.table.status() == 0


@pytest.mark.parametrize("mode", ["cover", "longest_suffix"])
def test_row_gradient_equals_the_trainable_table(mode):
    """fp32 rows: bit-equal to the values of TrainableFGramTable's sparse weight.grad on the same batch and grad_out; grad_base
    as _Lookup gives it."""
    from scone_amd import TrainableFGramTable
    d = 768
    keys, lens, tok, off, ids, live, g, base = _world(d, seed=1)
    w = np.random.default_rng(2).standard_normal((len(lens), d)).astype(np.float32)
    cache = _cache("fp32", d, mode, rows=torch.from_numpy(w))
    tr = TrainableFGramTable(cache, torch.from_numpy(w.copy()))
    b1 = torch.from_numpy(base).cuda().view(B, T, d).requires_grad_()
    g_t = torch.from_numpy(g).cuda().view(B, T, d)
    y1 = tr(torch.from_numpy(tok), base=b1)
    y1.backward(g_t)
    sp = tr.weight.grad
    with cache.live_rows(torch.from_numpy(tok)) as lb:
        plan_ids = lb.row_ids.cpu().numpy()
        rows = torch.from_numpy(w[plan_ids]).cuda().requires_grad_()
        b2 = torch.from_numpy(base).cuda().view(B, T, d).requires_grad_()
        y2 = lb.embed(rows, base=b2)
        assert E.same_bits(y2.detach().cpu().numpy(), y1.detach().cpu().numpy())       # the same forward bits, too
        y2.backward(g_t)
    assert np.array_equal(sp._indices()[0].cpu().numpy(), plan_ids)
    assert E.same_bits(rows.grad.cpu().numpy(), sp._values().cpu().numpy())
    assert E.same_bits(b2.grad.cpu().numpy(), b1.grad.cpu().numpy())


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_against_an_fp64_dense_model(reduce):
    """y = base + A @ rows in fp64.  Forward: K_p rows, one division and the base -- (K_p + 1 + 2) u sum |terms|; gradients:
    (references of the row + 2) u sum |c|, the bound of tests/test_backward_host.py; grad_base is exact."""
    d = 64
    keys, lens, tok, off, ids, live, g, base = _world(d, seed=2)
    A = _dense_A(off, ids, live, reduce)
    rows32 = np.random.default_rng(3).standard_normal((len(live), d)).astype(np.float32)
    cache = _cache("fp32", d)
    with cache.live_rows(torch.from_numpy(tok)) as lb:
        rows = torch.from_numpy(rows32).cuda().requires_grad_()
        base_t = torch.from_numpy(base).cuda().requires_grad_()
        y = lb.embed(rows, base=base_t, reduce=reduce)
        y.backward(torch.from_numpy(g).cuda().view(B, T, d))
    K = np.diff(off)
    y64 = base.astype(np.float64) + A @ rows32.astype(np.float64)
    mag = np.abs(base).astype(np.float64) + np.abs(A) @ np.abs(rows32).astype(np.float64)
    err = np.abs(y.detach().cpu().numpy().reshape(B * T, d).astype(np.float64) - y64)
    assert (err <= (K[:, None] + 3) * U32 * mag).all() and err.max() > 0
    rid, sums, mags, refs = BW.backward_rows_f64(off, ids, g, reduce)
    assert np.array_equal(rid, live) and np.allclose(sums, A.T @ g.astype(np.float64), rtol=1e-12, atol=1e-12)
    err = np.abs(rows.grad.cpu().numpy().astype(np.float64) - sums)
    assert (err <= (refs[:, None] + 2) * U32 * mags).all() and err.max() > 0
    assert E.same_bits(base_t.grad.cpu().numpy(), g)


class _ToyFGramModel(torch.nn.Module):
    """nn.Embedding summed over each f-gram's tokens (masked by lens), then a bias-free Linear."""

    def __init__(self, vocab, d_e, d, dtype=torch.float32):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, d_e, dtype=dtype)
        self.proj = torch.nn.Linear(d_e, d, bias=False, dtype=dtype)

    def forward(self, tokens, lens):
        mask = (torch.arange(tokens.shape[1], device=tokens.device)[None, :] < lens[:, None]).to(self.emb.weight.dtype)
        return self.proj((self.emb(tokens) * mask[:, :, None]).sum(dim=1))


def test_a_toy_f_gram_model_trains_through_the_lookup():
    """Three SGD steps on a 3 x 13 batch through lb.embed(model(lb.tokens, lb.lens), base=wte(ids)); the same loop in fp64 torch
    ops over the oracle's lists (y = base + A @ rows) gives every parameter gradient within (n + 2) u sum |terms|, where the sum
    of magnitudes is the same loop run on absolute values and n counts the longest chain of additions behind an element: the
    batch's references, the inner dimensions of the products and the f-gram length.  The loss decreases."""
    d, d_e, vocab = 64, 16, WS.VOCAB + 1
    keys, lens, tok, off, ids, live, _, _ = _world(d, seed=3)
    A64 = torch.from_numpy(_dense_A(off, ids, live))
    cache = _cache("fp32", d)
    torch.manual_seed(0)
    model = _ToyFGramModel(vocab, d_e, d).cuda()
    wte = torch.nn.Embedding(vocab, d).cuda()
    ref_model = _ToyFGramModel(vocab, d_e, d, dtype=torch.float64)
    ref_wte = torch.nn.Embedding(vocab, d, dtype=torch.float64)
    with torch.no_grad():
        ref_model.emb.weight.copy_(model.emb.weight.double().cpu())
        ref_model.proj.weight.copy_(model.proj.weight.double().cpu())
        ref_wte.weight.copy_(wte.weight.double().cpu())
    target = torch.from_numpy(np.random.default_rng(9).standard_normal((B, T, d)).astype(np.float32))
    ids_t = torch.from_numpy(tok)
    params, ref_params = [*model.parameters(), *wte.parameters()], [*ref_model.parameters(), *ref_wte.parameters()]
    opt, ref_opt = torch.optim.SGD(params, lr=0.5), torch.optim.SGD(ref_params, lr=0.5)
    n_chain = int(off[-1]) + d + d_e + MAX_N + B * T
    losses = []
    for step in range(3):
        opt.zero_grad()
        ref_opt.zero_grad()
        with cache.live_rows(ids_t) as lb:
            assert np.array_equal(lb.row_ids.cpu().numpy(), live)
            y = lb.embed(model(lb.tokens, lb.lens), base=wte(ids_t.cuda()))
            loss = ((y - target.cuda()) ** 2).mean()
            loss.backward()
            tokens, flens = lb.tokens.cpu(), lb.lens.cpu()
        y64 = ref_wte(ids_t).view(B * T, d) + A64 @ ref_model(tokens, flens)
        ref_loss = ((y64.view(B, T, d) - target.double()) ** 2).mean()
        ref_loss.backward()
        # the same backward on magnitudes: |dL/dy| through |A|, |W|, |h|
        with torch.no_grad():
            gy = (2.0 / y64.numel()) * (y64.view(B, T, d) - target.double()).abs().view(B * T, d)
            g_rows = A64.abs().T @ gy
            mask = (torch.arange(MAX_N)[None, :] < flens[:, None]).double()
            h = (ref_model.emb(tokens).abs() * mask[:, :, None]).sum(dim=1)
            mag_proj = g_rows.T @ h
            g_h = g_rows @ ref_model.proj.weight.abs()
            mag_emb = torch.zeros_like(ref_model.emb.weight)
            mag_emb.index_add_(0, tokens.reshape(-1), (g_h[:, None, :] * mask[:, :, None]).reshape(-1, d_e))
            mag_wte = torch.zeros_like(ref_wte.weight).index_add_(0, ids_t.reshape(-1), gy)
        for p, rp, mag, name in zip(params, ref_params, (mag_emb, mag_proj, mag_wte), ("emb", "proj", "wte")):
            err = (p.grad.double().cpu() - rp.grad).abs()
            bound = (n_chain + 2) * U32 * mag
            assert bool((err <= bound).all()), (step, name, float((err / bound.clamp_min(1e-300)).max()))
            assert float(rp.grad.abs().max()) > 0
        losses.append(float(loss.detach()))
        assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * abs(float(ref_loss.detach()))
        opt.step()
        ref_opt.step()
    assert losses[2] < losses[1] < losses[0], losses


@pytest.mark.parametrize("fmt", ["fp32", "int8"])
def test_store_and_bake(fmt):
    """300 rows, chunk_rows = 128 (three calls, the last of 44 rows).  store: the served table holds `rows` at row_ids and is
    unchanged elsewhere (int8: what store_f32 of the same rows leaves).  bake: embed_tokens on the baked table has the bits of
    lb.embed(fn(lb.tokens, lb.lens))."""
    from scone_amd import EmbeddingCache, NGramExtractor
    d, n, max_n = 64, 300, 3
    rng = np.random.default_rng(77)
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, 7, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    tok = rng.integers(0, 8, size=(B, T)).astype(np.int64)
    w0 = rng.standard_normal((n, d)).astype(np.float32)

    def make():
        c = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt)
        c.cache_embeddings(list(range(n)), torch.from_numpy(w0), verbose=False)
        return c

    cache, twin = make(), make()
    all_ids = torch.arange(n)
    before = cache.table.gather_rows(all_ids).cpu().numpy()
    with cache.live_rows(torch.from_numpy(tok)) as lb:
        live = lb.row_ids.cpu().numpy()
        assert 3 <= len(live) < n
        new = torch.from_numpy(rng.standard_normal((len(live), d)).astype(np.float32)).cuda()
        lb.store(new.to(torch.bfloat16))
        with pytest.raises(ValueError, match="rows must be"):
            lb.store(new[:-1])
    stored = new.to(torch.bfloat16).float()
    twin.table.store_f32(stored, ids=torch.from_numpy(live))
    after = cache.table.gather_rows(all_ids).cpu().numpy()
    assert E.same_bits(after, twin.table.gather_rows(all_ids).cpu().numpy())
    rest = np.setdiff1d(np.arange(n), live)
    assert E.same_bits(after[rest], before[rest]) and not np.array_equal(after[live], before[live])
    if fmt == "fp32":
        assert E.same_bits(after[live], stored.cpu().numpy())

    # elementwise (a bag of token embeddings times a column scale): its rows have the same bits whatever the chunk they are in,
    # which a matrix product does not promise
    torch.manual_seed(1)
    emb, scale = torch.randn(8, d, device="cuda"), torch.rand(d, device="cuda") + 0.5

    def model(tokens, flens):
        mask = (torch.arange(tokens.shape[1], device=tokens.device)[None, :] < flens[:, None]).float()
        return (emb[tokens] * mask[:, :, None]).sum(dim=1) * scale

    calls = []

    def fn(tokens, flens):
        calls.append(int(tokens.shape[0]))
        assert tokens.dtype == torch.int64 and tokens.shape[1] == max_n and bool((tokens * (torch.arange(max_n, device=tokens.device)
                                                                                            [None, :] >= flens[:, None])).eq(0).all())
        return model(tokens, flens)

    cache.bake(fn, chunk_rows=128)
    assert calls == [128, 128, 44]
    with torch.no_grad():
        full = model(*cache.f_gram_keys())
    twin.table.store_f32(full)                                        # the same rows through store_f32 in one piece
    assert E.same_bits(cache.table.gather_rows(all_ids).cpu().numpy(), twin.table.gather_rows(all_ids).cpu().numpy())
    base = torch.from_numpy(rng.standard_normal((B, T, d)).astype(np.float32)).cuda()
    served = cache.embed_tokens(torch.from_numpy(tok), base=base)
    with cache.live_rows(torch.from_numpy(tok)) as lb, torch.no_grad():
        rows = cache.table.gather_rows(lb.row_ids)                    # what the table's format made of fn's rows
        if fmt == "fp32":
            assert E.same_bits(rows.cpu().numpy(), model(lb.tokens, lb.lens).cpu().numpy())
            rows = model(lb.tokens, lb.lens)
        live_y = lb.embed(rows, base=base)
    assert E.same_bits(served.cpu().numpy(), live_y.cpu().numpy())
    assert cache.table.status() == 0
