"""The stream contract of include/scone_hip.h, as one protocol that every case of tests/test_gpu_stream_order.py runs.

The header promises, call by call, "all device work is enqueued on the given stream" and either "no synchronisation" or
"synchronises the stream (once)".  A test that hands the library complete inputs on an idle device cannot see a kernel on the
wrong stream, a copy on stream 0, a dropped cross-stream wait or a count read back behind the wrong stream: the bits come out
right anyway.  Here every call runs on a side stream S of torch's pool (such streams do not block on the null stream) whose
producers are still in flight:

  1. Every device input exists twice, `truth` (the reference was computed from it) and `poison` (a VALID input of the same shape
     that gives another answer: ids in range, offsets monotone with the same total, id lists ascending, distinct and owned,
     finite values).  The input buffers hold the poison.  A violation therefore shows as wrong bits, never as an access out of
     range.
  2. Warm-up: the whole sequence once on S without the delay, then S.synchronize(); module loading, first-use workspace growth,
     the staging pipeline's stream pick and torch's per-stream allocator pool are out of the way.  Outputs of the warm-up are
     overwritten with NaN / -1, mutated state is restored from saved copies, the buffers are poisoned again.
  3. On S: a delay kernel | NaN into the outputs that exist | truth -> input buffers | `busy` recorded | THE CALL |
     `returned_early = not busy.query()` | poison -> input buffers (a kernel that runs later than S says reads it) | clones of
     every output and of all mutated state.
  4. S.synchronize(); the caller compares the clones with its reference, bit for bit.

A kernel on another stream runs during the delay and reads the poison (or is overwritten by the NaN fill); a kernel that is not
ordered before what follows on S reads the poison written back; a hidden synchronise shows as `returned_early == False` (class
A), a synchronise of the wrong stream as `returned_early == True` or a count of the poison (class S).

No host-time bound is asserted anywhere.  The delay is sizing, not a pass criterion, and the protocol validates it itself: a
class-A call that did not return early fails with the delay's measured length and the host time of the call in the message, so
a delay that was too short says so and never passes vacuously.
"""

import time

import numpy as np
import torch

DELAY_MS = 50.0          # the target; never more than MAX_DELAY_MS
MAX_DELAY_MS = 200.0
A, S = "A", "S"          # the two classes of call (the test quotes the header's sentence beside each entry point)

_cycles_per_ms = None
_chain = None
_streams = {}


# ------------------------------------------------------------------ the delay
def _calibrate_sleep():
    """Cycles of torch.cuda._sleep per millisecond on this device: one short delay timed with two events, once per session."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        probe = 2_000_000
        torch.cuda._sleep(1000)                                  # the kernel's module is loaded
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        ms = max(e0.elapsed_time(e1), 1e-3)
        _cycles_per_ms = probe / ms
    return _cycles_per_ms


def _lookup_chain():
    """Without torch.cuda._sleep: (a function that queues one large lookup on the current stream, lookups per DELAY_MS)."""
    global _chain
    if _chain is None:
        from scone_amd import EmbeddingCache, NGramExtractor
        from scone_amd import synthetic as SY
        keys, lens = SY.make_keys(100_000, SY.GPT2_VOCAB, 3, seed=11)
        cache = EmbeddingCache.from_synthetic(NGramExtractor.from_arrays(keys, lens, max_n=3), 768, table_format="int8", seed=3)
        tok = torch.from_numpy(SY.stream_uniform_ids(keys, lens, 256, 512, 5)).to("cuda", torch.int32)
        out = torch.empty(256, 512, 768, dtype=torch.float16, device="cuda")
        table = cache.table

        def one():
            table.embed(tok, out=out, out_dtype=torch.float16)
        for _ in range(2):                                       # every stream the chain will run on warms its own workspace
            one()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            one()
        e1.record()
        e1.synchronize()
        per = max(e0.elapsed_time(e1) / 8, 1e-3)
        _chain = (one, max(1, min(int(round(DELAY_MS / per)), int(MAX_DELAY_MS / per))), cache)
    return _chain


def delay(ms=DELAY_MS, use_sleep=None):
    """Queue about `ms` milliseconds of device work on the current stream (a bounded spin, or a chain of large lookups)."""
    ms = min(float(ms), MAX_DELAY_MS)
    if use_sleep is None:
        use_sleep = hasattr(torch.cuda, "_sleep")
    if use_sleep:
        torch.cuda._sleep(int(_calibrate_sleep() * ms))
    else:
        one, n, _ = _lookup_chain()
        for _ in range(max(1, int(round(n * ms / DELAY_MS)))):
            one()


def warm_delay(use_sleep=None):
    """Calibrate (and, for the lookup chain, warm the current stream's workspace) outside any measured sequence."""
    if use_sleep is None:
        use_sleep = hasattr(torch.cuda, "_sleep")
    if use_sleep:
        _calibrate_sleep()
    else:
        one = _lookup_chain()[0]
        one()
        torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------ streams
def side_stream(table, beside=(), tag="S"):
    """A stream of torch's pool on which the protocol can tell streams apart.  HIP multiplexes a process's streams onto a few
    hardware queues; two streams that share one run one after the other, so a kernel put on stream 0 by mistake would queue up
    behind the delay on S and a missing wait would go unnoticed.  The first of eight candidates whose kernels run beside
    those of the null stream and of every stream in `beside` (`SconeTable.streams_overlap`, both directions' worth: sharing a
    queue is symmetric) is kept for the session under `tag`; the first candidate if none passes."""
    key = (tag, tuple(int(b.cuda_stream) for b in beside))
    if key not in _streams:
        null = torch.cuda.default_stream(table.device)
        made = [torch.cuda.Stream(device=table.device) for _ in range(8)]
        taken = {int(s.cuda_stream) for s in _streams.values()}
        pick = None
        for s in made:
            if int(s.cuda_stream) in taken:
                continue
            if all(table.streams_overlap(s, o) for o in (null, *beside)):
                pick = s
                break
        _streams[key] = pick if pick is not None else made[0]
    return _streams[key]


# ------------------------------------------------------------------ inputs and state
class Input:
    """One device input: `buf` is what the call is given; it holds `poison` except between the delay and the call's own
    reads, when it holds `truth`."""

    def __init__(self, truth, poison, device="cuda"):
        t = truth if isinstance(truth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(truth))
        p = poison if isinstance(poison, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poison))
        assert t.shape == p.shape and t.dtype == p.dtype, "truth and poison of an input differ in shape or type"
        self.truth, self.poison = t.to(device).contiguous(), p.to(device).contiguous()
        if t.numel():
            same = torch.equal(self.truth.view(torch.uint8) if t.dtype != torch.bool else self.truth,
                               self.poison.view(torch.uint8) if t.dtype != torch.bool else self.poison)
            assert not same, "a poison that equals the truth poisons nothing"
        self.buf = self.poison.clone()

    def set_truth(self):
        self.buf.copy_(self.truth)

    def set_poison(self):
        self.buf.copy_(self.poison)


class TensorState:
    """A device tensor the call updates in place (master rows, optimizer state, a control block)."""

    def __init__(self, tensor):
        self.t = tensor
        self.saved = None

    def save(self):
        self.saved = self.t.clone()

    def restore(self):
        self.t.copy_(self.saved)

    def snapshot(self):
        return self.t.clone()


class TableState:
    """The served rows of a table: saved and restored as raw payload + scales through the host (outside the measured
    sequence), read INSIDE it by a lookup on the current stream -- `gather_rows` of every owned row, which is stream-ordered --
    so that the snapshot also shows the mutation ordered before its reader."""

    def __init__(self, table):
        self.table = table
        self.lo, self.n = table.row_begin, table.row_end - table.row_begin
        self.ids = torch.arange(self.lo, self.lo + self.n, dtype=torch.int64, device=table.device)
        self.saved = None

    def save(self):
        rows, scales = self.table.download(self.lo, self.n)
        self.saved = (rows.copy(), None if scales is None else scales.copy())

    def restore(self):
        self.table.upload(self.saved[0], self.saved[1], row0=self.lo)

    def snapshot(self):
        return self.table.gather_rows(self.ids)


class Result:
    def __init__(self):
        self.returned_early = None       # not busy.query(), read immediately after the call
        self.out = {}                    # name -> numpy array: clones of outputs and of mutated state, made on S
        self.host = None                 # whatever the call returned to the host (counts, status bits)
        self.delay_ms = None             # the delay as the device ran it
        self.call_ms = None              # host time inside the call
        self.status = None               # table.status() after the sequence

    def describe(self):
        return f"delay {self.delay_ms:.1f} ms on the device, {self.call_ms:.2f} ms of host time inside the call"


def _scrub(t):
    if t.numel() == 0:
        return
    if t.is_floating_point():
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(255)
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(-1)


def to_numpy(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def run(call, inputs=(), *, stream, state=(), outputs=(), table=None, reset=None, use_sleep=None, delay_ms=DELAY_MS):
    """The protocol of the module docstring.

    call()     runs the entry point(s) under test on the CURRENT stream and returns `(device, host)`: a dict name -> device
               tensor of what it produced (cloned afterwards; outputs it wrote into `outputs` need not be listed) and any host
               value (or None).
    inputs     the `Input`s whose buffers the call reads.
    state      name -> TensorState / TableState: what the call mutates in place.
    outputs    name -> device tensor allocated by the caller before the sequence and written by the call.
    table      the handle whose status is read (and cleared) after the warm-up and after the sequence.
    reset()    anything else to undo after the warm-up (host-side state of the objects under test).
    Returns a `Result`."""
    state, outputs = dict(state), dict(outputs)
    res = Result()
    torch.cuda.synchronize()                                     # whatever the caller prepared on other streams is complete
    with torch.cuda.stream(stream):
        warm_delay(use_sleep)
        for st in state.values():
            st.save()
        # ---- 2. warm-up: the same sequence, same shapes, truth inputs, no delay
        for x in inputs:
            x.set_truth()
        dev, _ = call()
        clones = [t.clone() for t in list(dev.values()) + list(outputs.values())] + [st.snapshot() for st in state.values()]
        stream.synchronize()
        for t in list(dev.values()) + clones + list(outputs.values()):
            _scrub(t)
        del dev, clones
        for st in state.values():
            st.restore()
        for x in inputs:
            x.set_poison()
        if reset is not None:
            reset()
        if table is not None:
            table.status()                                       # synchronises S and clears the bits of the warm-up
        stream.synchronize()
        # ---- 3. the measured sequence
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        busy = torch.cuda.Event()
        e0.record(stream)
        delay(delay_ms, use_sleep)
        e1.record(stream)
        for t in outputs.values():
            _scrub(t)
        for x in inputs:
            x.set_truth()
        busy.record(stream)
        t0 = time.perf_counter()
        dev, res.host = call()
        res.returned_early = not busy.query()
        res.call_ms = (time.perf_counter() - t0) * 1e3
        for x in inputs:
            x.set_poison()
        got = {k: v.clone() for k, v in dev.items()}
        got.update({k: v.clone() for k, v in outputs.items()})
        got.update({k: st.snapshot() for k, st in state.items()})
        # ---- 4.
        stream.synchronize()
        res.delay_ms = e0.elapsed_time(e1)
        res.out = {k: to_numpy(v) for k, v in got.items()}
        if table is not None:
            res.status = table.status()
    return res


def check_class(res, klass, who):
    """The class of the call, from the header's wording.  A: it returned while the delay was still running.  S: everything
    queued before it had completed when it returned."""
    assert DELAY_MS / 5 <= res.delay_ms <= 1.5 * MAX_DELAY_MS, (
        f"{who}: the delay ran {res.delay_ms:.1f} ms on the device, not about {DELAY_MS:.0f}: the calibration is off, and a delay "
        "that short orders nothing")
    if klass == A:
        assert res.returned_early, (
            f"{who} is documented as stream-ordered without a synchronisation, but the work queued in front of it had completed "
            f"when it returned ({res.describe()}): a hidden synchronisation -- or, if the host time is not far below the delay, "
            "a delay that was too short for this call on this machine (then this is a failure of the test's sizing, not a pass)")
    else:
        assert klass == S
        assert not res.returned_early, (
            f"{who} is documented as synchronising its stream, but it returned while the work queued in front of it on that "
            f"stream was still running ({res.describe()}): it waited for another stream, or for none")


def sync_debug_honoured():
    """Does this torch build raise on a synchronising call under torch.cuda.set_sync_debug_mode("error")?  (It sees torch's own
    synchronisations -- .item(), .cpu(), a blocking copy -- not the library's; those are what `busy` is for.)"""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        return False
    before = torch.cuda.get_sync_debug_mode()
    x = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            x.item()
        except RuntimeError:
            return True
        return False
    finally:
        torch.cuda.set_sync_debug_mode(before)
