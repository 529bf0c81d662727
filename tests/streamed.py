"""The streamed mode of the framed harness (tests/framed.py, tests/test_framed_gpu.py): the stream contract of every C-ABI entry point
that takes a `void* stream` -- all work of the call starts after what the caller enqueued on that stream before it, and is finished, in
stream order, before what the caller enqueues next -- tested the way a real caller leans on it: inputs produced on a busy side stream
just before the call, outputs consumed just after it, no device-wide synchronisation in between.

StreamBed is a Bed whose case runs inside `with torch.cuda.stream(side)` on a fresh stream:

  veil            after put() has filled, poisoned and snapshotted an `in` / `inout` operand, the view's words are kept in a device copy
                  and overwritten with a veil: an ordinary NaN that is neither frame sentinel (floats), a fixed garbage word (int32).
                  `out` operands keep their sentinel.
  late reveal     the first st() enqueues a bounded delay on `side` (torch.cuda._sleep, calibrated to milliseconds with events; a chain
                  of matmuls where torch has no _sleep), then copies every kept view back, then hands out `side`.  The revealed bits are
                  the snapshot's, so the frame checks hold as they are.  A kernel, memset or copy of the call that is not ordered behind
                  `side` reads the veil or the sentinel: the value and "same bits as the packed call" checks fail.
  early consumer  directly after the C call returns, with no host synchronisation, every `out` / `inout` frame's whole buffer is cloned on
                  `side`.  After torch.cuda.synchronize() the clone must equal the final words: a word written after the clone belongs to
                  work that was never joined into the caller's stream (StreamError, located like a FrameError).

These checks can miss a fault (work that happens to finish early) and cannot raise a false alarm.  pg_alpha_nlml_async defers its join by
contract (csrc/capi.hip: join_side), so no early clone is taken after it; tests/test_streamed_gpu.py tests that join on its own.

Veil and EarlyClone work on CPU frames too (tests/test_streamed_cpu.py)."""
import ctypes as C

import torch

from framed import SENTINEL32, SENTINEL64, FrameError
from test_framed_gpu import Bed

VEIL64 = 0x7FF800000BAD5EED           # a quiet NaN (fp64) that is neither SENTINEL64 nor the poison NaN 0x7FF8000000000000
VEIL32 = 0x7FC05EED                   # the same for fp32
VEIL_INT = 0x0BADC0DE                 # int32 words: garbage that is neither SENTINEL32 nor the integer poison
TARGET_MS = 30.0                      # the delay aimed at per call ("some tens of milliseconds")
CAP_MS = 100.0                        # and what it may never exceed
DEFERRED = {"pg_alpha_nlml_async"}    # entry points whose join is deferred by contract: no early consumer directly behind them
assert len({VEIL64, SENTINEL64, 0x7FF8000000000000}) == 3 and len({VEIL32, VEIL_INT, SENTINEL32, 0x7FC00000, -0x5EA75EA8 & 0xFFFFFFFF}) == 5


class StreamError(FrameError):
    """A word of an output frame changed after the early consumer's clone: work of the call that was not joined into the caller's stream."""


def veil_word(f):
    if not f.dtype.is_floating_point:
        return VEIL_INT if f.item == 4 else VEIL64
    return VEIL64 if f.item == 8 else VEIL32


class Veil:
    """The kept views of the covered operands.  cover() after fill / poison / snapshot; reveal() puts the kept bits back."""

    def __init__(self):
        self.pending, self.done = [], []

    def cover(self, f):
        self.pending.append((f, f.wview.clone()))
        f.wview.fill_(veil_word(f))

    def reveal(self):
        for f, kept in self.pending:
            f.wview.copy_(kept)
        self.done += self.pending
        self.pending = []


class EarlyClone:
    """Whole-buffer clones of the given frames, taken on the current stream; check_final() after a device-wide synchronisation."""

    def __init__(self, frames):
        self.taken = [(f, f.words.clone()) for f in frames]

    def check_final(self):
        for f, clone in self.taken:
            bad = f.words != clone
            if bool(bad.any()):
                idx = torch.nonzero(bad.reshape(-1), as_tuple=False)
                where, region = f.locate(int(idx[0]))
                raise StreamError(f.name, "written after the consumer's clone (work not joined into the caller's stream)", idx.shape[0], where, region)


# ------------------------------------------------------------------------------------------- the delay
_DELAY = {}


def _spin(units):
    if _DELAY["kind"] == "sleep":
        torch.cuda._sleep(int(units))
    else:
        a = _DELAY["mat"]
        for _ in range(int(units)):
            torch.mm(a, a)


def _timed(units):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _spin(units)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibrate():
    """Once per session: the units (spin cycles of torch.cuda._sleep, or matmuls of the fallback chain) that last TARGET_MS, found by
    doubling until a run is long enough to time and scaling from there; measured again, and cut back if it came out above CAP_MS."""
    if "units" in _DELAY:
        return _DELAY
    if hasattr(torch.cuda, "_sleep"):
        _DELAY.update(kind="sleep")
        units = 1 << 12
    else:
        _DELAY.update(kind="matmul", mat=torch.ones(2048, 2048, device="cuda"))
        units = 1
    _timed(units)                                            # (warm-up: the first launch pays for loading the code)
    ms = _timed(units)
    while ms < 2.0 and units < 1 << 44:
        units *= 2
        ms = _timed(units)
    units = max(1, int(units * TARGET_MS / ms))
    ms = _timed(units)
    while ms > CAP_MS and units > 1:
        units = max(1, int(units * 0.5 * CAP_MS / ms))
        ms = _timed(units)
    _DELAY.update(units=units, ms=ms)
    print("streamed: delay of %.1f ms = %d %s" % (ms, units, "spin cycles" if _DELAY["kind"] == "sleep" else "matmuls"))
    return _DELAY


def delay():
    """Enqueue the calibrated delay on the current stream."""
    _spin(calibrate()["units"])


def probe_concurrent_streams():
    """No library call: veil a buffer, enqueue the delay and then the reveal on one stream, read the buffer on another.  True when the
    reader saw the veil everywhere (the streams run side by side) and the reveal arrived in the end."""
    calibrate()
    data = torch.arange(1 << 16, dtype=torch.float64, device="cuda")
    buf = torch.full_like(data, float("nan"))
    torch.cuda.synchronize()
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay()
        buf.copy_(data)
    with torch.cuda.stream(other):
        seen = buf.clone()
    torch.cuda.synchronize()
    assert bool((buf == data).all()), "the reveal never arrived"
    return bool(torch.isnan(seen).all())


# ------------------------------------------------------------------------------------------- the bed
_LIVE = []


def close_all():
    """Leave the side stream of every bed that a failed case left open."""
    for bed in list(_LIVE):
        bed.close()


class _Calls:
    """The library object as the cases see it (bed.lib): every call passes through; one that took the bed's stream is followed by the
    early consumer's clone."""

    def __init__(self, bed, lib):
        self._bed, self._lib = bed, lib

    def __getattr__(self, name):
        fn, bed = getattr(self._lib, name), self._bed

        def call(*args):
            rc = fn(*args)
            if bed.armed:
                bed.armed = False
                bed.calls.append(name)
                if name not in DEFERRED:
                    bed.consume()
            return rc

        return call


class StreamBed(Bed):
    null_stream = False       # sensitivity: hand the call the null stream while the reveal sits on `side`
    third_consumer = False    # sensitivity: take the early consumer's clone on an unrelated stream
    log = []                  # the entry points that took a StreamBed's stream, in order (read by tests/test_streamed_gpu.py)

    def __init__(self, ops, dtype, gapset):
        super().__init__(ops, dtype, gapset)
        assert self.framed
        self.lib = _Calls(self, ops.lib)
        self.side = torch.cuda.Stream()
        self.veil, self.early, self.armed, self.delayed, self.calls = Veil(), None, False, False, []
        self._scope = torch.cuda.stream(self.side)
        self._scope.__enter__()
        _LIVE.append(self)

    def close(self):
        if self in _LIVE:
            _LIVE.remove(self)
            self._scope.__exit__(None, None, None)

    def put(self, name, data=None, shape=None, dtype=None, role="in", written=None, scratch=None, poison=None, batch_gap=None):
        f = super().put(name, data=data, shape=shape, dtype=dtype, role=role, written=written, scratch=scratch, poison=poison, batch_gap=batch_gap)
        if role in ("in", "inout"):
            self.veil.cover(f)
        return f

    def st(self):
        with torch.cuda.stream(self.side):
            if not self.delayed:
                delay()
                self.delayed = True
            self.veil.reveal()
        self.armed = True
        return C.c_void_p(0 if self.null_stream else self.side.cuda_stream)

    def outputs(self):
        return [f for f, role, _, _ in self.items.values() if role != "in"]

    def consume(self, frames=None, stream=None):
        if stream is None:
            stream = torch.cuda.Stream() if self.third_consumer else self.side
        with torch.cuda.stream(stream):
            self.early = EarlyClone(self.outputs() if frames is None else frames)
        return self.early

    def check(self):
        torch.cuda.synchronize()
        self.close()
        StreamBed.log += self.calls
        assert self.calls, "no call took the bed's stream"
        if self.early is not None:
            self.early.check_final()
        super().check()
