"""Helpers of tests/test_gpu_streams.py: a device-side hold on a caller's stream, and a stream picker
that proves the picked stream runs beside the context's own stream and the null stream.

A hold is a delay kernel on a torch stream, the caller's "producer" operations behind it and an event
behind those.  While hold.pending() the producers have not run, so a call under test that returns with
the hold pending has not blocked the host on that stream, and whatever it queued on the stream runs
after the producers: results that show the producers' values prove the order.  A call that queued on
another stream ran at once, against the poison the test left in its inputs or before the producers'
clear of its outputs, and shows as wrong values.

The hold's length is not trusted: every use asserts pending() right after the call under test, so a
hold that is too short fails the test; it never passes it vacuously.

The calls under test take int device addresses (t.data_ptr()): the bindings of
cudavolumerenderer_amd/_lib.py synchronise torch's current stream when they are handed a tensor, which
would wait the hold out."""
import time

import torch

HOLD_MS = 200.0     # the holds of the ordering tests; the longest enqueue time observed on an MI355X host: 0.02 ms
CHECK_MS = 50.0     # the short hold of pick_stream's check
ENQUEUE_MS = {}     # what -> host ms of the call under test (the module's report prints the longest)

_delay = {}


def _calibrate():
    """("sleep", cycles per ms) with torch.cuda._sleep, else ("matmul", products per ms, operand): once
    per process, timed with two events around one delay on torch's current stream."""
    if _delay:
        return _delay
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)  # loads the kernel
        cycles = 1_000_000
        while True:
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0 or cycles >= 1 << 40:
                break
            cycles *= 8
        _delay.update(kind="sleep", per_ms=cycles / ms)
    else:
        a = torch.rand((2048, 2048), device="cuda")
        torch.mm(a, a)
        n = 8
        while True:
            e0.record()
            for _ in range(n):
                a = torch.mm(a, a).clamp_(0.0, 1.0)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0 or n >= 1 << 16:
                break
            n *= 4
        _delay.update(kind="matmul", per_ms=n / ms, operand=a)
    return _delay


def delay(ms):
    """A device-side delay of about `ms` on torch's current stream."""
    d = _calibrate()
    if d["kind"] == "sleep":
        torch.cuda._sleep(int(d["per_ms"] * ms))
    else:
        a = d["operand"]
        for _ in range(max(1, int(d["per_ms"] * ms))):
            a = torch.mm(a, a).clamp_(0.0, 1.0)


class Hold:
    """A delay of `ms` on `stream`, then producer() (torch operations, queued on `stream`), then an event."""

    def __init__(self, stream, producer=None, ms=HOLD_MS):
        _calibrate()  # (on the current stream, before anything is held)
        self.stream = stream
        self.event = torch.cuda.Event()
        with torch.cuda.stream(stream):
            delay(ms)
            if producer is not None:
                producer()
            self.event.record(stream)

    def pending(self):
        return not self.event.query()

    def call(self, fn, what):
        """fn(), the call under test: it must return with the hold still pending."""
        t0 = time.perf_counter()
        out = fn()
        ms = (time.perf_counter() - t0) * 1e3
        pending = self.pending()
        ENQUEUE_MS[what] = max(ms, ENQUEUE_MS.get(what, 0.0))
        assert pending, (f"{what}: the hold on the caller's stream ended before the call returned ({ms:.1f} ms on the "
                         f"host): the call waited for the stream, or the hold of {HOLD_MS} ms is too short")
        return out


def own_stream(cvr, ctx):
    """The context's own stream as a torch stream."""
    return torch.cuda.ExternalStream(cvr.load().cvr_own_stream(ctx._h))


def runs_beside(stream, others):
    """While a short hold is pending on `stream`, a clone queued on each of `others` completes."""
    src = torch.arange(1024, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    hold = Hold(stream, ms=CHECK_MS)
    done = []
    for o in others:
        with torch.cuda.stream(o):
            keep = src.clone()
            e = torch.cuda.Event()
            e.record(o)
        done.append((e, keep))
    for e, _ in done:
        e.synchronize()
    beside = hold.pending()
    stream.synchronize()
    return beside


def pick_stream(cvr, ctx, avoid=()):
    """A fresh torch stream that provably runs beside the context's own stream and the null stream: two
    HIP streams that share a hardware queue run one after the other, which would hide a launch on the
    wrong stream.  Up to 8 streams are tried; none qualifying is a failure, never a skip."""
    others = [own_stream(cvr, ctx), torch.cuda.default_stream()]
    taken = {int(o.cuda_stream) for o in others} | {int(s.cuda_stream) for s in avoid}
    tried = []
    for _ in range(8):
        s = torch.cuda.Stream()
        tried.append(s)  # (kept: a dropped stream's handle would come round again)
        if int(s.cuda_stream) in taken:
            continue
        if runs_beside(s, others):
            return s
    raise AssertionError("pick_stream: none of 8 fresh streams ran beside the context's own stream and the null "
                         "stream (they share hardware queues): the ordering tests would have no power")
