"""Training the f-gram table behind the fused lookup.

In the reference the f-gram table is a trained ``nn.Embedding`` (scone/models/f_gram_model.py:120,172) whose output is
added to the token embeddings (scone/models/language_model.py:239-243).  :class:`TrainableFGramTable` puts the one-launch
lookup of :class:`~scone_amd.EmbeddingCache` on an autograd tape: the forward is the existing kernel, bit for bit, and the
backward is the library's deterministic sparse row gradient (include/scone_hip.h, "backward") -- no host synchronise in
the reduction, no float atomics, the same bits on every run.  ``wte`` / ``wpe`` either stay the caller's torch code, added
outside as language_model.py:239-254 does (``base=``), or are passed to the lookup (``wte=`` / ``wpe=``) and trained through it:
their gradients are the same fixed-order sums in a second id space (include/scone_hip.h, "backward of the dense side").  The table's own update is either a stock ``torch.optim``
sparse step followed by :meth:`TrainableFGramTable.commit`, or :class:`FGramOptimizer`: one kernel launch that updates the
touched master rows, their optimizer state and the served table (include/scone_hip.h, "optimizer step").
"""

from typing import Optional

import torch
from torch import nn

from scone_amd import _lib
from scone_amd.hip_backend import APPLY_LEAN_MAX_DIM
from scone_amd.inference.embedding_cache import EmbeddingCache


def _add_coalesced(old: torch.Tensor, row_ids: torch.Tensor, grad_rows: torch.Tensor) -> torch.Tensor:
    """``old + sparse(row_ids, grad_rows)`` as a coalesced sparse tensor, without ``torch``'s ``coalesce()``, which is wrong
    for wide values with torch 2.10.0+rocm7.0 on gfx950.  Torch alone shows it (profiles/r17a/torch_coalesce_wide_values.txt):
    with 25 sorted ids and fp32 ``a``, ``b`` ``[25, d]`` on the device,
    ``torch.sparse_coo_tensor(torch.cat([ids, ids])[None], torch.cat([a, b]), (60, d)).coalesce().values()`` equals ``a + b``
    at d = 64 and 256, and differs in 228 of 512, 456 of 768 (all zero from column 312 on) and 684 of 1024 columns;
    ``(sa + sb).coalesce()`` of the two coalesced tensors gives the same.  So no path here calls it.  ``row_ids`` are sorted
    and distinct; a row both operands have is ``old + new`` (one fp32 add), a row one has is that row, bit for bit.  An
    ``old`` that is not coalesced (set by the caller) has its duplicates added first, by ``index_add_``."""
    old_ids, old_rows = old._indices()[0], old._values()
    ids, inverse = torch.unique(torch.cat([old_ids, row_ids]), return_inverse=True)         # sorted
    at_old, at_new = inverse[:old_ids.numel()], inverse[old_ids.numel():]
    rows = torch.zeros((ids.numel(), grad_rows.shape[1]), dtype=grad_rows.dtype, device=grad_rows.device)
    if old.is_coalesced():
        rows.index_copy_(0, at_old, old_rows)
    else:
        rows.index_add_(0, at_old, old_rows)
    in_old = torch.zeros(ids.numel(), dtype=torch.bool, device=ids.device)
    in_old[at_old] = True
    both = in_old[at_new]
    rows.index_copy_(0, at_new, torch.where(both[:, None], rows[at_new] + grad_rows, grad_rows))
    return torch.sparse_coo_tensor(ids[None], rows, tuple(old.shape), is_coalesced=True)


def _is_library_rows(rows: torch.Tensor, table) -> bool:
    """fp32 ``[n, d]`` rows on the table's device: what ``SconeTable.grad_merge`` takes."""
    return (isinstance(rows, torch.Tensor) and rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == table.dim
            and rows.device == table.device and table.dim % 4 == 0)


def _library_operand(grad: Optional[torch.Tensor], table):
    """``(row_ids, grad_rows)`` of a sparse gradient the library adds to (include/scone_hip.h, "gradient accumulation"): a
    coalesced ``[N, d]`` COO tensor with fp32 values on the table's device -- what the backward sets.  Anything else (none, or a
    gradient set by the caller: not coalesced, another dtype or device) is ``None`` and stays with :func:`_add_coalesced`."""
    if grad is None or not grad.is_sparse or grad.layout != torch.sparse_coo or not grad.is_coalesced():
        return None
    if grad.sparse_dim() != 1 or not _is_library_rows(grad._values(), table):
        return None
    return grad._indices()[0], grad._values()


class _StaticGrad:
    """The buffers of a module in static mode (``static_rows=``): one :class:`~scone_amd.hip_backend.BackwardContext` and one
    ``(ids [cap] int64, rows [cap, d] fp32, n [1] int64)`` set, allocated once.  The backward fills them with the count left on
    the device, so ``forward; backward; FGramOptimizer.step()`` neither synchronises nor allocates and can be captured in a
    ``torch.cuda.graph`` and replayed on new tokens (include/scone_hip.h, "backward and optimizer step without a host
    synchronisation")."""

    def __init__(self, table, static_rows: int, max_tokens: int) -> None:
        if max_tokens is None or int(max_tokens) <= 0:
            raise ValueError("static_rows= needs max_tokens=: the most positions a batch can have")
        if int(static_rows) <= 0:
            raise ValueError("static_rows must be positive: the most distinct rows a batch can touch")
        self.cap = int(static_rows)
        self.ctx = table.backward_context(int(max_tokens))
        self.ids = torch.zeros(self.cap, dtype=torch.int64, device=table.device)
        self.rows = torch.zeros((self.cap, table.dim), dtype=torch.float32, device=table.device)
        self.n = torch.zeros(1, dtype=torch.int64, device=table.device)

    def check(self, module, ctx_base_dtype) -> None:
        """The refusals of a static backward: ``ValueError`` before any device work."""
        if getattr(module, "_fused_opt", None) is not None:
            raise ValueError("static_rows= and fused_backward=True do not go together (scone_backward_apply_lean takes a plan "
                             "whose counts are on the host)")
        if module.static_grad is not None:
            raise ValueError("static_rows=: a gradient is already there, and accumulation over micro-batches is not available "
                             "with the counts on the device; call zero_grad() between backwards, or build the module without "
                             "static_rows=")
        if ctx_base_dtype is not None and module.cache.lookup_mode == "longest_suffix":
            raise ValueError("static_rows= with base= on a longest_suffix cache is not available (grad_base needs the hit counts "
                             "of a plan)")

    def backward(self, module, tok, cu, grad_out, reduce) -> None:
        self.ctx.plan(tok, cu)
        module.static_grad = self.ctx.rows(grad_out, reduce, out=(self.ids, self.rows, self.n))


def _dense_inputs(who: str, wte, wpe, base, static) -> None:
    """The refusals of the dense side, before any device work (called outside the autograd function, where the caller's grad
    mode is still visible)."""
    if wte is not None and base is not None:
        raise ValueError(f"{who}: wte= and base= do not go together (base IS the dense term: pass one of them)")
    if static is not None and torch.is_grad_enabled() and any(w is not None and w.requires_grad for w in (wte, wpe)):
        raise ValueError(f"{who}: static_rows= trains the table only -- a wte / wpe that requires grad needs the index plan with "
                         "its counts on the device (the _dn form of scone_backward_plan_index), which does not exist yet; "
                         "pass them detached, or build the module without static_rows=")


def _dense_grads(table, tok, cu, position_ids, grad_out, wte, wpe, skip, sparse_wte):
    """``(grad_wte, grad_wpe)`` of ``out = (wte[tok] + fg) + wpe[pos]`` (include/scone_hip.h, "backward of the dense side"): each
    an index plan summed in the backward's fixed order -- no float atomics, the same bits on every run.  ``wte`` / ``wpe``: the
    tensor whose gradient is wanted, or ``None``.  ``skip``: the table plan's hit counts in longest_suffix mode (a matched f-gram
    replaced the token term), else ``None``.  ``grad_wpe`` is never masked: the position term is added in both modes."""
    grad_wte = grad_wpe = None
    d = table.dim
    if wte is not None:
        with table.backward_plan_index(tok.reshape(-1), wte.shape[0], skip=skip) as plan:
            ids, rows = plan.rows(grad_out, "sum")
        rows = rows.to(wte.dtype)
        if sparse_wte:
            grad_wte = torch.sparse_coo_tensor(ids[None], rows, tuple(wte.shape), is_coalesced=True)
        else:                                           # distinct ids: index_copy_ is deterministic
            grad_wte = torch.zeros(tuple(wte.shape), dtype=wte.dtype, device=rows.device).index_copy_(0, ids, rows)
    if wpe is not None:
        n_pos = wpe.shape[0]
        grad_wpe = torch.zeros((n_pos, d), dtype=wpe.dtype, device=grad_out.device)
        if cu is None and position_ids is None:         # the rectangle with default positions: no plan
            g3 = grad_out if grad_out.dim() == 3 else grad_out.reshape(1, -1, d)
            rows = table.backward_wpe(g3, n_pos)
            grad_wpe[:rows.shape[0]].copy_(rows)
        else:
            ntok = grad_out.numel() // d
            if position_ids is not None:
                pos = torch.as_tensor(position_ids).to(device=table.device, dtype=torch.int32)
                pos = pos.reshape(-1) if cu is not None else pos.expand(*grad_out.shape[:-1]).reshape(-1)
            else:
                pos = table.default_positions(cu_seqlens=cu, total=ntok)
            with table.backward_plan_index(pos, n_pos) as plan:
                ids, rows = plan.rows(grad_out, "sum")
            grad_wpe.index_copy_(0, ids, rows.to(wpe.dtype))
    return grad_wte, grad_wpe


def _hand_over_wte_grad(wte: torch.Tensor, grad):
    """A SPARSE ``grad_wte`` is set on a leaf ``wte`` here, not returned: autograd's accumulation re-creates a sparse gradient
    without its coalesced flag (as for the table's own gradient).  Returns what the backward still has to return."""
    if grad is None or not grad.is_sparse or not wte.is_leaf:
        return grad
    if wte.grad is None:
        wte.grad = grad
    elif wte.grad.is_sparse:
        wte.grad = _add_coalesced(wte.grad, grad._indices()[0], grad._values())
    else:
        wte.grad.index_add_(0, grad._indices()[0], grad._values())        # onto a dense gradient: distinct ids, one add per element
    return None


class _Lookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, base, module, input_ids, cu_seqlens, reduce, out_dtype, wte=None, wpe=None, position_ids=None):
        cache = module.cache
        tok = torch.as_tensor(input_ids)
        dense = {}
        if wte is not None or wpe is not None or position_ids is not None:
            dense = dict(wpe=None if wpe is None else wpe.detach().contiguous(), position_ids=position_ids)
        if base is not None and cache.lookup_mode == "longest_suffix":
            # the paper's lookup onto a dense base (a matched f-gram REPLACES the base row) is the table's call
            table = cache.to_device()
            if cu_seqlens is None:
                out = table.embed_base(tok, base, reduce=reduce, out_dtype=out_dtype, **dense)
            else:
                out = table.embed_base_varlen(tok, cu_seqlens, base, reduce=reduce, out_dtype=out_dtype, **dense)
        else:
            if wte is not None:
                dense["wte"] = wte.detach().contiguous()
            out = cache.embed_tokens(tok, reduce=reduce, base=base, cu_seqlens=cu_seqlens, out_dtype=out_dtype, **dense)
        ctx.module, ctx.tok, ctx.cu, ctx.reduce = module, tok, cu_seqlens, reduce
        ctx.base_dtype = None if base is None else base.dtype
        ctx.base_shape = None if base is None else base.shape
        ctx.wte, ctx.wpe, ctx.position_ids = wte, wpe, position_ids
        return out

    @staticmethod
    def backward(ctx, grad_out):
        module = ctx.module
        table = module.cache.to_device()
        grad_weight = grad_base = grad_wte = grad_wpe = None
        grad_out = grad_out.contiguous()
        need_wte = ctx.wte is not None and ctx.needs_input_grad[7]
        need_wpe = ctx.wpe is not None and ctx.needs_input_grad[8]
        static = getattr(module, "_static", None)
        if static is not None:                                # static_rows=: the counts stay on the device
            static.check(module, ctx.base_dtype)              # (a trainable wte / wpe was refused by the forward)
            if ctx.needs_input_grad[0]:
                static.backward(module, ctx.tok, ctx.cu, grad_out, ctx.reduce)
            if ctx.base_dtype is not None and ctx.needs_input_grad[1]:
                grad_base = grad_out.to(ctx.base_dtype).reshape(ctx.base_shape)
            return grad_weight, grad_base, None, None, None, None, None, None, None, None
        fused = getattr(module, "_fused_opt", None)           # an FGramOptimizer(fused_backward=True): the update happens here
        suffix = module.cache.lookup_mode == "longest_suffix"
        need_base = ctx.base_dtype is not None and ctx.needs_input_grad[1]
        skip = None
        if ctx.needs_input_grad[0] or (suffix and (need_base or need_wte)):   # else the table's plan has nothing to give
            with table.backward_plan(ctx.tok, ctx.cu) as plan:
                if ctx.needs_input_grad[0] and fused is not None:
                    fused._apply_backward(plan, grad_out, ctx.reduce)
                elif ctx.needs_input_grad[0]:
                    old = module._mergeable_grad()
                    if old is not None:
                        # a gradient is already there: the library adds this batch's rows to it, and they are never stored
                        module._set_merged(plan.row_ids(), *plan.rows(grad_out, ctx.reduce, accumulate=old))
                    else:
                        row_ids, grad_rows = plan.rows(grad_out, ctx.reduce)
                        # set on the module, not returned: autograd's accumulation re-creates a sparse gradient without its
                        # coalesced flag
                        module._accumulate(row_ids, grad_rows)
                if suffix and (need_base or need_wte):        # a matched f-gram replaced the base row / the token term
                    skip = plan.counts()
            # (the plan is closed while its kernels may still run: freeing device memory waits for the device)
        if need_base:
            grad_base = grad_out
            if suffix:
                grad_base = grad_out * (skip == 0).reshape(*grad_out.shape[:-1], 1)
            grad_base = grad_base.to(ctx.base_dtype).reshape(ctx.base_shape)
        if need_wte or need_wpe:
            grad_wte, grad_wpe = _dense_grads(table, ctx.tok, ctx.cu, ctx.position_ids, grad_out, ctx.wte if need_wte else None,
                                              ctx.wpe if need_wpe else None, skip, getattr(module, "sparse_wte_grad", False))
            if need_wte:
                grad_wte = _hand_over_wte_grad(ctx.wte, grad_wte)
        return grad_weight, grad_base, None, None, None, None, None, grad_wte, grad_wpe, None


class _DenseSide:
    """What :class:`_Lookup` asks of a module, for a lookup whose table is NOT trained (``SconeEmbedding`` with a cache)."""

    def __init__(self, cache, sparse_wte_grad: bool = False) -> None:
        self.cache, self.sparse_wte_grad = cache, bool(sparse_wte_grad)


def embed_tokens_dense_grad(cache: EmbeddingCache, input_ids: torch.Tensor, *, wte: Optional[torch.Tensor] = None,
                            wpe: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None, cu_seqlens=None,
                            reduce: str = "mean", out_dtype: Optional[torch.dtype] = None,
                            sparse_wte_grad: bool = False) -> torch.Tensor:
    """``cache.embed_tokens(input_ids, wte=, wpe=, ...)`` -- the same call, the same bits -- differentiable in ``wte`` and ``wpe``
    while the table stays fixed: their gradients are the library's deterministic index-plan sums (``_dense_grads``).  In cover
    mode no table plan is built."""
    return _Lookup.apply(None, None, _DenseSide(cache, sparse_wte_grad), input_ids, cu_seqlens, reduce, out_dtype, wte, wpe,
                         position_ids)


class _LiveLookup(torch.autograd.Function):
    """:meth:`LiveFGramBatch.embed` on the tape: the forward is ``scone_embed_rows`` on the batch's live rows, the backward
    the plan's deterministic row gradient -- ``[U, d]``, row ``u`` belonging to ``row_ids[u]``: the gradient of ``rows`` -- and
    the index-plan gradients of ``wte`` / ``wpe``."""

    @staticmethod
    def forward(ctx, rows, base, batch, wte, wpe, position_ids, reduce, out_dtype, out, sparse_wte):
        y = batch.table.embed_rows(batch.input_ids, batch.plan.row_ids(), rows.detach(), cu_seqlens=batch.cu_seqlens,
                                   wte=None if wte is None else wte.detach(), wpe=None if wpe is None else wpe.detach(),
                                   base=None if base is None else base.detach(), pos=position_ids, reduce=reduce,
                                   out_dtype=out_dtype, out=out)
        if out is not None:
            ctx.mark_dirty(out)
        ctx.batch, ctx.reduce, ctx.rows_dtype = batch, reduce, rows.dtype
        ctx.base_dtype = None if base is None else base.dtype
        ctx.base_shape = None if base is None else base.shape
        ctx.wte, ctx.wpe, ctx.position_ids, ctx.sparse_wte = wte, wpe, position_ids, sparse_wte
        return y

    @staticmethod
    def backward(ctx, grad_out):
        batch = ctx.batch
        grad_rows = grad_base = grad_wte = grad_wpe = None
        grad_out = grad_out.contiguous()
        suffix = batch.cache.lookup_mode == "longest_suffix"
        need_wte = ctx.wte is not None and ctx.needs_input_grad[3]
        need_wpe = ctx.wpe is not None and ctx.needs_input_grad[4]
        if ctx.needs_input_grad[0]:
            grad_rows = batch.plan.rows(grad_out, ctx.reduce)[1].to(ctx.rows_dtype)
        if ctx.base_dtype is not None and ctx.needs_input_grad[1]:
            grad_base = grad_out                                     # as _Lookup returns it
            if suffix:                                               # a matched f-gram replaced the base row
                grad_base = grad_out * (batch.plan.counts() == 0).reshape(*grad_out.shape[:-1], 1)
            grad_base = grad_base.to(ctx.base_dtype).reshape(ctx.base_shape)
        if need_wte or need_wpe:
            skip = batch.plan.counts() if suffix and need_wte else None
            grad_wte, grad_wpe = _dense_grads(batch.table, batch.input_ids, batch.cu_seqlens, ctx.position_ids, grad_out,
                                              ctx.wte if need_wte else None, ctx.wpe if need_wpe else None, skip, ctx.sparse_wte)
            if need_wte:
                grad_wte = _hand_over_wte_grad(ctx.wte, grad_wte)
        return grad_rows, grad_base, None, grad_wte, grad_wpe, None, None, None, None, None


class LiveFGramBatch:
    """The f-grams one batch matches, and the fused lookup over rows computed for them: what connects an f-gram MODEL to the
    lookup during training (the reference trains its f-gram embeddings with a separate model and only bakes them into a table
    for inference, README.md:21-23).  Made by :meth:`EmbeddingCache.live_rows`; a context manager, ``close()`` frees the plan.

    ``row_ids [U]`` (int64, ascending) are the distinct f-gram ids the batch hits, ``tokens [U, max_n]`` / ``lens [U]`` their
    token ids (0 beyond ``lens``) -- the f-gram model's input.  :meth:`embed` looks the batch up in ``rows [U, d]``, the model's
    output for exactly those f-grams, and is differentiable in ``rows`` and ``base``; :meth:`store` writes rows into the served
    table."""

    def __init__(self, cache: EmbeddingCache, input_ids: torch.Tensor, cu_seqlens=None) -> None:
        self.cache = cache
        self.table = table = cache.to_device()
        tok = torch.as_tensor(input_ids)
        if cu_seqlens is None and tok.dim() == 1:
            tok = tok.unsqueeze(0)
        self.input_ids = tok.to(device=table.device, dtype=torch.int32).contiguous()
        self.cu_seqlens = cu_seqlens
        if cu_seqlens is not None and not (isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda):
            from scone_amd.hip_backend import check_cu_seqlens
            self.cu_seqlens = torch.from_numpy(check_cu_seqlens(cu_seqlens, self.input_ids.shape[0])).to(table.device)
        self.plan = table.backward_plan(self.input_ids, self.cu_seqlens)      # the one synchronise: it reads U
        self.row_ids = self.plan.row_ids()
        keys, lens = cache.f_gram_keys(table.device)
        self.tokens = keys.index_select(0, self.row_ids)
        self.lens = lens.index_select(0, self.row_ids)

    def close(self) -> None:
        self.plan.close()

    def __enter__(self) -> "LiveFGramBatch":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __len__(self) -> int:
        return int(self.row_ids.shape[0])

    def embed(self, rows: torch.Tensor, *, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
              base: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None, reduce: str = "mean",
              out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
              sparse_wte_grad: bool = False) -> torch.Tensor:
        """``out = (base | wte[input_ids]) + reduce_k rows[slot of f_gram_k] + wpe[position_ids]`` -- :meth:`EmbeddingCache.embed_tokens`
        with the f-gram rows taken from ``rows [U, d]`` (fp32 / fp16 / bf16; row ``u`` is the row of ``row_ids[u]``), bit
        for bit what a table of that type holding them would give.  The gradient of ``rows`` is the library's deterministic
        sparse row gradient (``[U, d]``, cast to ``rows.dtype``); the gradient of ``base`` is ``grad_out`` (``lookup_mode="cover"``)
        or ``grad_out * (K == 0)`` (``"longest_suffix"``: a matched f-gram replaced the base row).  A ``wte`` / ``wpe``
        that requires grad is trained through the same call (include/scone_hip.h, "backward of the dense side"): its gradient
        is dense, in its own dtype, summed in the backward's fixed order without float atomics -- ``grad_wte`` over the tokens
        (in ``"longest_suffix"`` mode only where no f-gram matched), ``grad_wpe`` over ``position_ids`` or the lookup's default
        positions, never masked; ``sparse_wte_grad=True`` hands ``grad_wte`` over as a coalesced ``torch.sparse_coo_tensor``.
        ``wte=`` together with ``base=`` is refused.  May be called more than once per batch."""
        _dense_inputs("LiveFGramBatch.embed", wte, wpe, base, None)
        return _LiveLookup.apply(rows, base, self, wte, wpe, position_ids, reduce, out_dtype, out, bool(sparse_wte_grad))

    def store(self, rows: torch.Tensor) -> None:
        """Write the batch's rows into the served table at ``row_ids``, whatever its format (``store_f32``)."""
        if rows.dim() != 2 or tuple(rows.shape) != (len(self), self.table.dim):
            raise ValueError(f"rows must be [{len(self)}, {self.table.dim}], got {tuple(rows.shape)}")
        if len(self):
            self.table.store_f32(rows.detach().float(), ids=self.row_ids)


class TrainableFGramTable(nn.Module):
    """The f-gram table of ``cache`` as a trainable module.

    ``weight`` (fp32 ``[N, d]`` on the table's device, an ``nn.Parameter``) is the master copy; the cache may hold any
    ``table_format`` -- an INT8 table served from an fp32 master, a folded projection -- because the gradient of the lookup
    never reads a table row.  ``forward`` runs the existing one-launch lookup (``embed_tokens``, with ``base=`` when given;
    on a ``lookup_mode="longest_suffix"`` cache with ``base=`` the paper's form, ``cache.table.embed_base``), so its output
    has the serving path's bits exactly.  ``backward`` sets ``weight.grad`` itself, to a coalesced ``torch.sparse_coo_tensor``
    (a backward onto a gradient that is already there adds to it on the device -- ``scone_backward_rows_acc``, include/scone_hip.h
    "gradient accumulation": the new rows are never stored; a gradient the caller has set that is not coalesced, fp32 and on the
    table's device is added by torch glue instead; ``torch.autograd.grad`` does not see it; use an
    optimiser that takes sparse gradients: ``SGD``, ``SparseAdam``, ``Adagrad`` -- or :class:`FGramOptimizer`, which updates
    the served table in the same launch), and returns ``grad_base = grad_out``
    (cover mode) or ``grad_out * (K == 0)`` (longest suffix: a matched f-gram replaced the base row).
    ``forward(ids, wte=, wpe=, position_ids=)`` is ``embed_tokens(wte=, wpe=)``, bit for bit; a ``wte`` / ``wpe`` that requires
    grad gets a dense gradient in its own dtype from the library's index plans (deterministic, no float atomics; dense because
    GPT-2 ties ``wte`` to ``lm_head``, whose gradient is dense) -- ``sparse_wte_grad=True``: a coalesced sparse ``wte.grad``, set
    on the leaf as the table's is.  ``wte=`` with ``base=`` is refused, and so is a trainable ``wte`` / ``wpe`` in static mode.
    :meth:`commit` re-stores the rows touched since the last commit into the served table, after which it equals a table built
    from the updated weights.  The cache's host copy of the rows, if it keeps one, is not updated: it is the table at
    ingestion time.

    ``static_rows=cap, max_tokens=`` (static mode; :class:`FGramOptimizer` only): the backward plans in one
    ``BackwardContext`` of ``max_tokens`` positions and writes into one ``(ids [cap], rows [cap, d], n)`` buffer set, with the
    row count ``n`` left on the device, and sets ``static_grad`` to that triple instead of ``weight.grad``; nothing
    synchronises or allocates, so ``forward; backward; opt.step()`` can be captured and replayed.  A batch that touches more
    than ``cap`` rows writes nothing and the step changes nothing (``opt.rows_overflowed()``)."""

    def __init__(self, cache: EmbeddingCache, weight: torch.Tensor, static_rows: Optional[int] = None,
                 max_tokens: Optional[int] = None, sparse_wte_grad: bool = False) -> None:
        super().__init__()
        self.sparse_wte_grad = bool(sparse_wte_grad)
        table = cache.to_device()
        if not isinstance(weight, nn.Parameter):
            weight = nn.Parameter(torch.as_tensor(weight).to(device=table.device, dtype=torch.float32).contiguous())
        if weight.dtype != torch.float32 or tuple(weight.shape) != (table.n_rows, table.dim) or weight.device != table.device:
            raise ValueError(f"weight must be an fp32 [{table.n_rows}, {table.dim}] parameter on {table.device}")
        self.cache = cache
        self.weight = weight
        self._touched = []
        self._static = None if static_rows is None else _StaticGrad(table, static_rows, max_tokens)
        self.static_grad = None         # static mode: (ids, rows, n) after a backward

    def forward(self, input_ids: torch.Tensor, *, base: Optional[torch.Tensor] = None, cu_seqlens=None, reduce: str = "mean",
                out_dtype: Optional[torch.dtype] = None, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        _dense_inputs("TrainableFGramTable", wte, wpe, base, self._static)
        return _Lookup.apply(self.weight, base, self, input_ids, cu_seqlens, reduce, out_dtype, wte, wpe, position_ids)

    def _mergeable_grad(self):
        """``(row_ids, grad_rows)`` of ``weight.grad`` if the library can add to it (``SconeTable.grad_merge``: coalesced, fp32,
        on the table's device), else ``None`` -- no gradient, or one the caller has set that stays on ``_add_coalesced``."""
        return _library_operand(self.weight.grad, self.cache.to_device())

    def _set_merged(self, touched_ids: torch.Tensor, row_ids: torch.Tensor, grad_rows: torch.Tensor) -> None:
        self._touched.append(touched_ids)
        self.weight.grad = torch.sparse_coo_tensor(row_ids[None], grad_rows, tuple(self.weight.shape), is_coalesced=True)

    def _accumulate(self, row_ids: torch.Tensor, grad_rows: torch.Tensor) -> None:
        old = self._mergeable_grad()
        if old is not None and _is_library_rows(grad_rows, self.cache.to_device()):
            self._set_merged(row_ids, *self.cache.to_device().grad_merge(*old, row_ids, grad_rows))
            return
        self._touched.append(row_ids)
        sparse = torch.sparse_coo_tensor(row_ids[None], grad_rows, tuple(self.weight.shape), is_coalesced=True)
        weight = self.weight
        weight.grad = sparse if weight.grad is None else _add_coalesced(weight.grad, row_ids, grad_rows)

    @torch.no_grad()
    def commit(self, ids: Optional[torch.Tensor] = None) -> int:
        """Re-store ``weight[ids]`` into the served table (``ids=None``: the rows touched by a backward since the last
        commit -- all an optimiser without momentum or weight decay has changed).  Returns the number of rows stored."""
        if ids is None:
            if not self._touched:
                return 0
            ids = torch.unique(torch.cat(self._touched))
        ids = torch.as_tensor(ids).to(device=self.weight.device, dtype=torch.int64).reshape(-1)
        self._touched = []
        if ids.numel():
            self.cache.to_device().store_f32(self.weight.detach()[ids], ids=ids)
        return int(ids.numel())


class InPlaceFGramTable(nn.Module):
    """The f-gram table of ``cache`` trained IN PLACE: the served fp32 / bf16 rows are the weights, and there is no ``[N, d]``
    tensor of any kind (include/scone_hip.h, "lean optimizer step").  ``forward`` and ``grad_base`` are
    :class:`TrainableFGramTable`'s.  ``anchor``, a parameter of zero elements, only makes autograd call the backward; the
    sparse gradient lands on the module as ``grad = (row_ids, grad_rows)`` -- ``row_ids`` int64 ``[U]`` sorted and distinct,
    ``grad_rows`` fp32 ``[U, d]`` -- and a backward onto a gradient that is already there adds to it (a row both have is one fp32
    add, a row one has is that row, bit for bit).  Only :class:`FGramOptimizer` (``"sgd"`` or ``"rowwise_adagrad"``) updates it.
    ``static_rows=cap, max_tokens=``: static mode, as on :class:`TrainableFGramTable` -- the backward sets ``static_grad =
    (ids, rows, n)`` with the count on the device, and ``grad`` stays ``None``."""

    def __init__(self, cache: EmbeddingCache, static_rows: Optional[int] = None, max_tokens: Optional[int] = None,
                 sparse_wte_grad: bool = False) -> None:
        super().__init__()
        self.sparse_wte_grad = bool(sparse_wte_grad)
        table = cache.to_device()
        self.cache = cache
        self.shape = (table.n_rows, table.dim)
        self.anchor = nn.Parameter(torch.zeros(0, dtype=torch.float32, device=table.device))
        self.grad = None
        self._fused_opt = None          # set by FGramOptimizer(fused_backward=True)
        self._static = None if static_rows is None else _StaticGrad(table, static_rows, max_tokens)
        self.static_grad = None         # static mode: (ids, rows, n) after a backward

    def forward(self, input_ids: torch.Tensor, *, base: Optional[torch.Tensor] = None, cu_seqlens=None, reduce: str = "mean",
                out_dtype: Optional[torch.dtype] = None, wte: Optional[torch.Tensor] = None, wpe: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        _dense_inputs("InPlaceFGramTable", wte, wpe, base, self._static)
        return _Lookup.apply(self.anchor, base, self, input_ids, cu_seqlens, reduce, out_dtype, wte, wpe, position_ids)

    def _mergeable_grad(self):
        """``grad`` if the library can add to it (fp32 rows and int64 ids on the table's device), else ``None``."""
        if self.grad is None:
            return None
        ids, rows = self.grad
        table = self.cache.to_device()
        ok = _is_library_rows(rows, table) and ids.dtype == torch.int64 and ids.dim() == 1 and ids.device == table.device
        return (ids, rows) if ok and ids.numel() == rows.shape[0] else None

    def _set_merged(self, touched_ids: torch.Tensor, row_ids: torch.Tensor, grad_rows: torch.Tensor) -> None:
        self.grad = (row_ids, grad_rows)

    def _accumulate(self, row_ids: torch.Tensor, grad_rows: torch.Tensor) -> None:
        old = self._mergeable_grad()
        if old is not None and _is_library_rows(grad_rows, self.cache.to_device()):
            self.grad = self.cache.to_device().grad_merge(*old, row_ids, grad_rows)
            return
        if self.grad is not None:
            old = torch.sparse_coo_tensor(self.grad[0][None], self.grad[1], self.shape, is_coalesced=True)
            both = _add_coalesced(old, row_ids, grad_rows)
            row_ids, grad_rows = both._indices()[0], both._values()
        self.grad = (row_ids, grad_rows)


class FGramOptimizer:
    """The fused sparse optimizer of a :class:`TrainableFGramTable` (include/scone_hip.h, "optimizer step").

    ``step()`` consumes ``module.weight.grad`` -- the coalesced sparse gradient the backward set -- and in ONE kernel launch
    updates the touched rows of ``module.weight``, their optimizer state and the served table, so the next forward reads the
    updated rows and ``module.commit()`` has nothing left to store.  ``kind``: ``"sgd"``, ``"adagrad"`` or ``"adam"`` (the
    arithmetic of ``torch.optim.SparseAdam``: lazy moments, bias correction folded into the step size); ``weight_decay`` is
    decoupled and lazy (only the touched rows decay).  Adam's ``m`` / ``v`` and Adagrad's sum of squares are fp32 ``[N, d]``
    on the table's device, allocated at the first step.  ``lr`` is a plain attribute: change it between steps (schedules are
    the caller's).  No host synchronisation, no ``coalesce()``; the same bits on every run.

    The lean kinds (include/scone_hip.h, "lean optimizer step").  ``"rowwise_adagrad"`` keeps ONE fp32 accumulator per row:
    ``state2`` is fp32 ``[N]``.  On a :class:`TrainableFGramTable` it updates the fp32 master and re-stores the served rows, as
    the other kinds do.  On an :class:`InPlaceFGramTable` (``"sgd"`` or ``"rowwise_adagrad"`` only, an fp32 or bf16 cache only)
    the served rows themselves are updated; ``rounding="stochastic"`` (bf16 rows) draws its bits from ``seed``, the step count
    ``t``, the row id and the column, so a run is reproducible and a resumed one (``state_dict``) continues it.

    ``fused_backward=True`` (an :class:`InPlaceFGramTable` of ``d <= 4096`` only; include/scone_hip.h, "backward applied in
    place").  The lookup's backward itself updates the served rows, so the fp32 ``[U, d]`` gradient is never stored:
    ``module.grad`` stays ``None``, ``t`` advances once per backward, and the update reads ``lr``, ``eps``, ``weight_decay`` and
    the attribute ``grad_scale`` at backward time.  TWO BACKWARDS ARE TWO UPDATES -- nothing is left to accumulate into -- so
    gradient accumulation over micro-batches needs the default road (where a second backward adds to the gradient on the device:
    include/scone_hip.h, "gradient accumulation").  ``step()`` only returns the number of rows updated since
    the last ``step()`` (its ``grad_scale`` argument is not used) and ``zero_grad()`` has nothing to do.  One backward of this
    road leaves the bits one backward + ``step(grad_scale)`` of the default road leaves.

    ``capturable=True`` (include/scone_hip.h, "optimizer hyper-parameters on the device"; what ``torch.optim.Adam(capturable=True)``
    is to Adam).  ``lr``, ``betas``, ``eps``, ``weight_decay``, the gradient scale, ``seed`` and the step count ``t`` live in a
    104-byte block on the device, ``opt.hyper`` (an :class:`~scone_amd.hip_backend.OptHyper`): ``step()`` advances the count and
    derives the kernels' scalars ON THE DEVICE (``scone_opt_hyper_advance``) and the update reads them there (``scone_opt_step_dh``
    / ``scone_opt_step_lean_dh``), in static and in non-static mode.  So every kind and ``rounding="stochastic"`` can be captured
    with a module built with ``static_rows=``, a replay counts its own step, and a schedule or a dynamic loss scale is a device
    write between replays: ``opt.hyper.lr.copy_(device_scalar)``, ``step(grad_scale=device_scalar)``.  Assigning ``opt.lr``,
    ``opt.weight_decay``, ``opt.eps``, ``opt.betas`` or ``opt.t`` enqueues the write; READING ``opt.t`` SYNCHRONISES (it reads the
    device).  ``t`` does NOT advance on a step the device skipped (``skip_nonfinite=True``).  Adam's step size uses the header's
    integer power in place of ``pow``: at most one fp32 ulp from the default road's, and the same bits wherever the header lists.
    Not with ``fused_backward=True`` (``ValueError``)."""

    def __init__(self, module, kind: str = "adam", lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, rounding: str = "nearest", seed: int = 0, fused_backward: bool = False,
                 capturable: bool = False) -> None:
        self.capturable, self.hyper = False, None      # until the block exists the setters below only keep the host's copy
        self.in_place = isinstance(module, InPlaceFGramTable)
        kinds = ("sgd", "rowwise_adagrad") if self.in_place else ("sgd", "adagrad", "adam", "rowwise_adagrad")
        if kind not in kinds:
            raise ValueError(f"unknown optimizer kind {kind!r} for a {type(module).__name__} ({', '.join(kinds)})")
        if rounding not in ("nearest", "stochastic"):
            raise ValueError(f"unknown rounding {rounding!r} (nearest, stochastic)")
        if self.in_place:
            fmt = module.cache.to_device().fmt
            if fmt not in (_lib.FMT_F32, _lib.FMT_BF16):
                raise ValueError("an InPlaceFGramTable is trained on an fp32 or bf16 cache: a quantised or fp16 row cannot hold "
                                 "small updates")
            if rounding == "stochastic" and fmt != _lib.FMT_BF16:
                raise ValueError("stochastic rounding is for bf16 rows: an fp32 row has nothing to round")
        elif rounding == "stochastic":
            raise ValueError("stochastic rounding is for an InPlaceFGramTable: a master copy has nothing to round")
        if capturable and fused_backward:
            raise ValueError("capturable=True and fused_backward=True do not go together (scone_backward_apply_lean takes its "
                             "hyper-parameters by value)")
        self.module, self.kind = module, kind
        self.rounding, self.seed = rounding, int(seed)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.t = 0
        self.grad_scale = 1.0                          # fused_backward: read at backward time
        self.fused_backward = False
        self._fused_rows = 0                           # rows updated by fused backwards since the last step()
        self._set_fused(fused_backward)
        self.state1: Optional[torch.Tensor] = None     # Adam's m
        self.state2: Optional[torch.Tensor] = None     # Adam's v / Adagrad's sum of squares
        self.last_ctl = None                           # the GradCtl of the last clipped / guarded step()
        self._static_ctl = self._static_sq = self._static_scratch = None    # static mode: kept across steps (and replays)
        if capturable:
            table = module.cache.to_device()
            self._n_word = torch.zeros(1, dtype=torch.int64, device=table.device)   # non-static mode: the row count, for the _dh calls
            self.capturable = True
            self._init_hyper(0)

    def _init_hyper(self, t: int) -> None:
        """(Re-)initialise the device block from the host's copies and ``t`` steps already applied (``scone_opt_hyper_init``)."""
        self.hyper = self.module.cache.to_device().opt_hyper(lr=self._lr, betas=self._betas, eps=self._eps,
                                                             weight_decay=self._weight_decay, grad_scale=1.0, seed=self.seed,
                                                             step=int(t), out=self.hyper)

    # lr, betas, eps, weight_decay and t are plain values on the default road; with capturable=True an assignment also enqueues
    # the write into the device block, and t is read from there
    def _put(self, field: str, value) -> None:
        if self.hyper is not None:
            getattr(self.hyper, field).fill_(value)

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value) -> None:
        self._lr = float(value)
        self._put("lr", self._lr)

    @property
    def eps(self) -> float:
        return self._eps

    @eps.setter
    def eps(self, value) -> None:
        self._eps = float(value)
        self._put("eps", self._eps)

    @property
    def weight_decay(self) -> float:
        return self._weight_decay

    @weight_decay.setter
    def weight_decay(self, value) -> None:
        self._weight_decay = float(value)
        self._put("weight_decay", self._weight_decay)

    @property
    def betas(self):
        return self._betas

    @betas.setter
    def betas(self, value) -> None:
        self._betas = (float(value[0]), float(value[1]))
        self._put("beta1", self._betas[0])
        self._put("beta2", self._betas[1])

    @property
    def t(self) -> int:
        """The number of steps applied.  ``capturable=True``: read from the device -- SYNCHRONISES."""
        return int(self.hyper.step.item()) if self.hyper is not None else self._t

    @t.setter
    def t(self, value) -> None:
        self._t = int(value)
        self._put("step", self._t)

    def _set_fused(self, on: bool) -> None:
        on = bool(on)
        if on and self.capturable:
            raise ValueError("capturable=True and fused_backward=True do not go together (scone_backward_apply_lean takes its "
                             "hyper-parameters by value)")
        if on:
            if getattr(self.module, "_static", None) is not None:
                raise ValueError("fused_backward=True and a module built with static_rows= do not go together "
                                 "(scone_backward_apply_lean takes a plan whose counts are on the host)")
            if not self.in_place:
                raise ValueError("fused_backward is for an InPlaceFGramTable: a TrainableFGramTable's master rows are updated by "
                                 "step()")
            dim = self.module.cache.to_device().dim
            if dim > APPLY_LEAN_MAX_DIM:
                raise ValueError(f"fused_backward needs d <= {APPLY_LEAN_MAX_DIM}, this table has d = {dim}")
            other = self.module._fused_opt
            if other is not None and other is not self and other.fused_backward:
                other.fused_backward = False           # one optimizer updates a module
        if self.in_place and (on or self.module._fused_opt is self):
            self.module._fused_opt = self if on else None
        self.fused_backward = on

    @torch.no_grad()
    def _apply_backward(self, plan, grad_out: torch.Tensor, reduce: str) -> None:
        """One update, from inside the lookup's backward (``fused_backward=True``)."""
        table = self.module.cache.to_device()
        self.t += 1
        self._ensure_state()
        state = None if self.state2 is None else self.state2[table.row_begin:table.row_end]
        self._fused_rows += plan.apply_lean(grad_out, reduce, kind=self.kind, lr=self.lr, row_state=state, eps=self.eps,
                                            weight_decay=self.weight_decay, grad_scale=self.grad_scale, rounding=self.rounding,
                                            seed=self.seed, step=self.t)

    def _ensure_state(self) -> None:
        if self.kind == "rowwise_adagrad":
            if self.state2 is None:
                table = self.module.cache.to_device()
                self.state2 = torch.zeros(table.n_rows, dtype=torch.float32, device=table.device)
            return
        if self.in_place:
            return
        w = self.module.weight
        if self.kind == "adam" and self.state1 is None:
            self.state1 = torch.zeros_like(w.detach(), memory_format=torch.contiguous_format)
        if self.kind in ("adam", "adagrad") and self.state2 is None:
            self.state2 = torch.zeros_like(w.detach(), memory_format=torch.contiguous_format)

    def _current_grad(self):
        """``(row_ids, grad_rows)`` of the gradient on the module, or ``None``."""
        module = self.module
        if self.in_place:
            return module.grad
        weight, grad = module.weight, module.weight.grad
        if grad is None:
            return None
        if not grad.is_sparse:
            raise ValueError("FGramOptimizer.step: module.weight.grad must be the sparse gradient the lookup's backward sets")
        if not grad.is_coalesced():                      # set by the caller: its duplicates are added first, never by coalesce()
            none = torch.zeros(0, dtype=torch.int64, device=grad.device)
            grad = _add_coalesced(grad, none, torch.zeros((0, weight.shape[1]), dtype=grad.dtype, device=grad.device))
        return grad._indices()[0], grad._values()

    @torch.no_grad()
    def grad_sqnorm(self) -> torch.Tensor:
        """The squared norm of the gradient now on the module (both module kinds), as it is -- before any ``grad_scale`` -- a
        0-dim float64 tensor on the table's device, summed in the fixed order of ``scone_grad_sqnorm``: the same bits on every
        run.  No gradient: zero.  No synchronisation."""
        table = self.module.cache.to_device()
        static = getattr(self.module, "static_grad", None)
        if static is not None:
            return table.grad_sqnorm(static[1], n=static[2])[0]
        grad = self._current_grad()
        if grad is None:
            return torch.zeros((), dtype=torch.float64, device=table.device)
        return table.grad_sqnorm(grad[1])[0]

    def rows_overflowed(self) -> bool:
        """Static mode: whether a backward since the last call touched more rows than ``static_rows`` -- it then wrote nothing,
        left ``n = 0``, and the step behind it changed nothing.  Reads and CLEARS the table's sticky status bits (all of them,
        as ``table.status()`` does).  SYNCHRONISES."""
        return self.module.cache.to_device().rows_overflowed()

    def _static_state_ready(self) -> bool:
        if self.kind == "rowwise_adagrad":
            return self.state2 is not None
        if self.in_place:
            return True
        return (self.kind != "adam" or self.state1 is not None) and (self.kind == "sgd" or self.state2 is not None)

    def _need_warm_up(self, ctl_road: bool) -> None:
        """Under capture nothing may be allocated: the state, and on the clipped road the kept control buffers, must be there."""
        if not self._static_state_ready() or (ctl_road and self._static_ctl is None):
            raise ValueError("FGramOptimizer.step under capture: the optimizer state is allocated at the first step; run one "
                             "step eagerly (the warm-up) before capturing")

    def _static_control(self, table, cap: int):
        """Static mode's control block, squared norm and norm scratch (for buffers of ``cap`` rows): allocated at the first
        clipped step, then kept across steps -- and replays."""
        if self._static_ctl is None:
            from scone_amd.hip_backend import GradCtl
            self._static_ctl = GradCtl(table.device)
            self._static_sq = torch.zeros((), dtype=torch.float64, device=table.device)
            self._static_scratch = torch.zeros(_lib.grad_sqnorm_scratch(cap), dtype=torch.float64, device=table.device)
        return self._static_ctl, self._static_sq, self._static_scratch

    @staticmethod
    def _extra_terms(extra_sqnorm) -> list:
        """``extra_sqnorm`` -- nothing, one term or a sequence of terms -- as a list."""
        if extra_sqnorm is None:
            return []
        return list(extra_sqnorm) if isinstance(extra_sqnorm, (list, tuple)) else [extra_sqnorm]

    def _launch_step(self, ids, rows, *, grad_scale, ctl, n=None, hyper=None) -> None:
        """The one launch of every road: ``opt_step_lean`` in place on the served rows, ``opt_step_lean`` on the master for
        row-wise Adagrad, else ``opt_step``.  ``n`` / ``hyper``: the row count / the scalars on the device; without ``hyper`` the
        scalars go by value, ``self.t`` (already advanced) among them."""
        module = self.module
        table = module.cache.to_device()
        lo, hi = table.row_begin, table.row_end

        def own(x):                                      # the rows this handle owns: a contiguous view
            return None if x is None else x[lo:hi]

        scalars = {} if hyper is not None else dict(lr=self.lr, eps=self.eps, weight_decay=self.weight_decay,
                                                    grad_scale=grad_scale, step=self.t)
        if self.in_place:
            if hyper is None:
                scalars["seed"] = self.seed
            table.opt_step_lean(ids, rows, kind=self.kind, row_state=own(self.state2), rounding=self.rounding, ctl=ctl, n=n,
                                hyper=hyper, **scalars)
            return
        if self.kind == "rowwise_adagrad":
            table.opt_step_lean(ids, rows, kind=self.kind, master=own(module.weight.detach()), row_state=own(self.state2), ctl=ctl,
                                n=n, hyper=hyper, **scalars)
        else:
            if hyper is None:
                scalars["betas"] = self.betas
            table.opt_step(ids, rows, own(module.weight.detach()), kind=self.kind, state1=own(self.state1), state2=own(self.state2),
                           ctl=ctl, n=n, hyper=hyper, **scalars)
        module._touched = []                             # the served table is current: commit() has nothing to store

    def found_nonfinite(self) -> bool:
        """Whether the last ``step(...)`` that took a clipping / skipping argument found inf or NaN and skipped (with
        ``skip_nonfinite=True``; without it nothing is ever skipped).  SYNCHRONISES: it reads ``last_ctl.skip``.  For the loss
        scale's update and for skipping the caller's dense optimizers."""
        return self.last_ctl is not None and bool(self.last_ctl.skip.item())

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, *, max_norm: Optional[float] = None, extra_sqnorm=None,
             skip_nonfinite: bool = False) -> int:
        """One update from the gradient on the module (``None``: nothing happens, ``t`` stays).  ``grad_scale`` multiplies the
        gradient first (an un-scaling of a loss scale, a 1 / accumulation count).  Returns the number of rows listed.

        With ``max_norm``, ``extra_sqnorm`` or ``skip_nonfinite`` set, the step is clipped and guarded on the device, with no
        host synchronise: ``grad_sqnorm()``, then ``table.grad_ctl([that, *extra_sqnorm], grad_scale, max_norm,
        skip_nonfinite)`` -- kept as ``last_ctl`` -- then the ``_ctl`` step, whose kernel multiplies ``grad_scale`` by the block's
        ``coef = min(1, max_norm / (norm + 1e-6))`` (``torch.nn.utils.clip_grad_norm_``'s) and writes nothing when the block's
        ``skip`` is set.  ``extra_sqnorm``: the squared norm of the other gradients clipped together with the table's (the dense
        parameters', other shards'), at the SAME loss scale -- a 0-dim device tensor, a float, or a sequence of them.
        ``skip_nonfinite=True`` skips the step if any term is inf or NaN.  ``t`` ADVANCES ON A DEVICE-SKIPPED STEP TOO: the
        host does not know the outcome.  A caller who wants Adam's ``t`` unchanged by a skipped step calls
        :meth:`found_nonfinite` (a synchronise) and sets ``opt.t -= 1``.  With ``capturable=True`` there is nothing to correct:
        the count is on the device and ``t`` does NOT advance on a device-skipped step.  With none of the three set, the step is
        the plain one.

        ``capturable=True``: ``grad_scale`` is a float, a 0-dim float64 tensor on the table's device (copied into the block
        without a synchronise: a dynamic loss scale), or ``None`` (the block's ``hyper.grad_scale`` as it stands).  A
        hyper-parameter that is not finite on the device declines the step and sets ``hyper.bad``.

        Static mode (a module built with ``static_rows=``): the gradient is ``module.static_grad``, whose row count is on the
        device; the ``_dn`` calls read it there, the norm's scratch and the control block are kept on the optimizer, and nothing
        synchronises or allocates after the first step -- the step can be captured.  Returns the buffers' capacity (the count
        itself is ``module.static_grad[2]``).  While the stream is capturing, ``kind="adam"`` and ``rounding="stochastic"`` are
        refused (``ValueError``): their step-dependent scalars are launch arguments, which a replay repeats as captured.
        Eagerly both work; with ``capturable=True`` both are captured.  A backward that overflowed ``static_rows`` left
        ``n = 0``: the step changes nothing (:meth:`rows_overflowed`)."""
        ctl_road = max_norm is not None or extra_sqnorm is not None or bool(skip_nonfinite)
        if self.fused_backward:                          # (never capturable, never a static module: _set_fused)
            if ctl_road:
                raise ValueError("FGramOptimizer.step: max_norm / extra_sqnorm / skip_nonfinite need the gradient's norm before the "
                                 "first row is written, and fused_backward=True has updated the rows in the backward; use the "
                                 "default road (fused_backward=False)")
            n, self._fused_rows = self._fused_rows, 0    # the backwards have updated the rows already
            return n
        # the roads differ in where (ids, rows, n) and the control block come from, and in where the scalars live
        static = getattr(self.module, "static_grad", None)
        hyper = self.hyper if self.capturable else None
        capturing = (hyper is not None or static is not None) and torch.cuda.is_current_stream_capturing()
        if capturing and hyper is None:
            # the step-dependent scalars are launch arguments: a replayed graph would repeat them as captured
            if self.kind == "adam":
                raise ValueError("FGramOptimizer.step under capture: Adam's bias correction depends on the step count, which a "
                                 "replayed graph would repeat as captured; use sgd, adagrad or rowwise_adagrad, or step eagerly")
            if self.rounding == "stochastic":
                raise ValueError("FGramOptimizer.step under capture: stochastic rounding draws its bits from the step count, which "
                                 "a replayed graph would repeat as captured; use rounding='nearest', or step eagerly")
        table = self.module.cache.to_device()
        if static is not None:                           # the triple of a static backward: the count is on the device
            ids, rows, n = static
        else:                                            # the gradient on the module
            if capturing:
                raise ValueError("FGramOptimizer.step under capture needs a module built with static_rows= (the default backward "
                                 "synchronises)")
            grad = self._current_grad()
            if grad is None:
                return 0
            ids, rows = grad
            n = None
            if hyper is not None:                        # the _dh calls read the count from a device word the optimizer keeps
                ids, rows = ids.contiguous(), rows.contiguous()
                n = self._n_word.fill_(ids.numel())
        if capturing:
            self._need_warm_up(ctl_road)
        if hyper is not None:
            if isinstance(grad_scale, torch.Tensor):
                if grad_scale.dtype != torch.float64 or grad_scale.numel() != 1 or grad_scale.device != table.device:
                    raise ValueError(f"FGramOptimizer.step: a grad_scale on the device must be one float64 on {table.device}")
                hyper.grad_scale.copy_(grad_scale.reshape(()))
            elif grad_scale is not None:
                hyper.grad_scale.fill_(float(grad_scale))
        ctl = None
        if ctl_road:
            if static is not None:
                out, sq, scratch = self._static_control(table, rows.shape[0])
                sq = table.grad_sqnorm(rows, scratch, n=n, out=sq)[0]
            else:
                out, sq = None, table.grad_sqnorm(rows)[0]
            scale = dict(grad_scale=grad_scale) if hyper is None else dict(hyper=hyper)
            ctl = table.grad_ctl([sq, *self._extra_terms(extra_sqnorm)], max_norm=max_norm, skip_nonfinite=skip_nonfinite, out=out,
                                 **scale)
            self.last_ctl = ctl
        if hyper is not None:
            table.opt_hyper_advance(hyper, self.kind, ctl)     # the count and the scalars: on the device
        else:
            self.t += 1
        self._ensure_state()
        self._launch_step(ids, rows, grad_scale=grad_scale, ctl=ctl, n=n, hyper=hyper)
        if hyper is not None and static is None:
            stream = torch.cuda.current_stream(table.device)
            ids.record_stream(stream)                    # they may be temporaries of the caller (the n= calls record nothing)
            rows.record_stream(stream)
        return int(ids.numel())

    def zero_grad(self, set_to_none: bool = True) -> None:
        if getattr(self.module, "_static", None) is not None:
            self.module.static_grad = None               # the buffers stay; the next backward fills them again
        if self.in_place:
            module = self.module
            if module.grad is not None and not set_to_none:
                ids, rows = module.grad
                module.grad = (ids[:0], rows[:0])
            else:
                module.grad = None
            return
        grad = self.module.weight.grad
        if grad is None:
            return
        if set_to_none:
            self.module.weight.grad = None
        else:
            shape = tuple(self.module.weight.shape)
            self.module.weight.grad = torch.sparse_coo_tensor(
                torch.zeros((1, 0), dtype=torch.int64, device=grad.device),
                torch.zeros((0, shape[1]), dtype=grad.dtype, device=grad.device), shape, is_coalesced=True)

    def state_dict(self) -> dict:
        """``capturable=True``: ``t`` and the hyper-parameters are the DEVICE's (a synchronise): what a schedule wrote into
        ``opt.hyper`` is what is saved."""
        if self.capturable:
            h = self.hyper.read()
            self._lr, self._betas, self._eps, self._weight_decay = h["lr"], (h["beta1"], h["beta2"]), h["eps"], h["weight_decay"]
            self._t = h["step"]
        return {"kind": self.kind, "t": self._t, "lr": self.lr, "betas": self.betas, "eps": self.eps,
                "weight_decay": self.weight_decay, "rounding": self.rounding, "seed": self.seed, "capturable": self.capturable,
                "fused_backward": self.fused_backward, "grad_scale": self.grad_scale,
                "state1": None if self.state1 is None else self.state1.clone(),
                "state2": None if self.state2 is None else self.state2.clone()}

    def load_state_dict(self, state: dict) -> None:
        if state["kind"] != self.kind:
            raise ValueError(f"state of a {state['kind']!r} optimizer loaded into a {self.kind!r} one")
        # (a state saved with either value of capturable loads into either optimizer: the mode is the constructor's)
        self._t, self._lr, self._eps, self._weight_decay = int(state["t"]), float(state["lr"]), float(state["eps"]), float(state["weight_decay"])
        self._betas = (float(state["betas"][0]), float(state["betas"][1]))
        rounding = state.get("rounding", "nearest")
        if rounding == "stochastic" and not (self.in_place and self.module.cache.to_device().fmt == _lib.FMT_BF16):
            raise ValueError("a state with stochastic rounding is for an InPlaceFGramTable on a bf16 cache")
        self.rounding, self.seed = rounding, int(state.get("seed", 0))
        self._set_fused(state.get("fused_backward", False))
        self.grad_scale = float(state.get("grad_scale", 1.0))
        if self.capturable:
            self._init_hyper(self._t)                    # the block: these values, seed, and t steps already applied
        table = self.module.cache.to_device()
        shape = (table.n_rows,) if self.kind == "rowwise_adagrad" else (table.n_rows, table.dim)
        for name in ("state1", "state2"):
            s = state[name]
            if s is not None:
                if tuple(s.shape) != shape:
                    raise ValueError(f"{name} must be {list(shape)}, got {list(s.shape)}")
                s = s.to(device=table.device, dtype=torch.float32).contiguous().clone()
            setattr(self, name, s)
