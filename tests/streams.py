"""Stream-order checks for the device wrappers (a helper module, not a conftest; plain torch).

Every other GPU test runs on torch's default stream -- the null stream, which every blocking stream synchronises with -- so an internal step issued on the wrong
stream (a ``<<<g, b, 0, 0>>>`` launch, a ``hipMemset`` without ``Async``, a table converted on whatever stream was current when it was cached) still gives the
right answer there.  torch's pool streams are non-blocking: on them such a step is ordered with nothing.

* ``filler(stream, ms)``: queues roughly ``ms`` of fills of one large buffer on ``stream`` and returns an event recorded behind them.  Calibrated once per
  process with events on the default stream.
* ``delayed(stream, tensors)``: the DELAYED PRODUCER.  Every device-tensor input gets a twin that holds 0xFF bytes (``tests/guards.py``'s NaN pattern); the filler
  is queued on ``stream`` and ``twin.copy_(true)`` behind it.  A wrapper then called with the twins under ``torch.cuda.stream(stream)`` sees the true data only
  in steps that are ordered behind ``stream``; any other step reads poison.
* ``run_delayed(fn, tensors, stream)``: ``delayed``, the call, ``returned_early`` taken the moment the wrapper returns, and -- still on ``stream``, without any
  synchronisation -- a clone of every output (the CONSUMER: an internal step that is still running on another stream when the wrapper's last launch on
  ``stream`` has finished shows in the clone or in the output).  This check is deterministic.
* ``interleaved(calls, s1, s2)``: calls of growing and shrinking size issued alternately on two streams behind a filler on both, the assignment swapped between
  repetitions, each result compared bit for bit with the same call issued alone.  A temporary shared between the two streams is caught by this ONLY WITH SOME
  PROBABILITY per run: both streams must be inside the colliding steps at the same time.  The delayed producer is the deterministic check; this one adds
  coverage of per-stream arenas and plan-owned work buffers that no input or output reaches (what such memory carries from one call to the next ON ONE
  stream is the subject of tests/test_gpu_scratch.py: poisoned arenas and plan scratch, entries in each other's wake, plans after a NaN frame).

Out of reach: inputs a wrapper takes as HOST arrays (geometry, delay tables, filters, weights -- the list in tests/test_gpu_guards.py's halo section): they are
uploaded by the wrapper itself and have no producer to delay."""
from __future__ import annotations

import torch

from tests import guards as GD

_STATE = {}                       # the filler's buffer and its calibration (one per process)
_FILL_BYTES = 1 << 30


def bits(t):
    """the tensor's bit pattern as integers (NaN compares equal to itself)"""
    t = t.contiguous()
    if t.is_complex():
        t = t.reshape(-1).view(GD._REAL[t.dtype])
    return t.view(GD._INT[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def calibrate():
    """the filler's buffer (allocated once) and the number of fills per millisecond, measured with events on the default stream"""
    if not _STATE:
        buf = torch.empty(_FILL_BYTES, dtype=torch.uint8, device="cuda")
        for _ in range(3):
            buf.fill_(1)
        torch.cuda.synchronize()
        n = 40
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            buf.fill_(1)
        b.record()
        b.synchronize()
        _STATE["buf"], _STATE["per_ms"] = buf, n / max(a.elapsed_time(b), 1e-3)
    return _STATE


def filler(stream, ms):
    """queue roughly ``ms`` milliseconds of device work on ``stream``; returns an event recorded behind it"""
    st = calibrate()
    n = max(1, int(ms * st["per_ms"] + 0.999))
    with torch.cuda.stream(stream):
        for _ in range(n):
            st["buf"].fill_(1)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def returned_early(event):
    """True when the work in front of ``event`` is still running: take it the moment a wrapper returns"""
    return not event.query()


def _poisoned_twin(t):
    """an all-0xFF tensor with the shape, dtype and strides of ``t`` (a strided view stays one; the elements it skips are poison too)"""
    span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) if t.numel() else 0
    raw = torch.full((span * t.element_size(),), GD.FILL, dtype=torch.uint8, device=t.device)
    return raw.view(t.dtype).as_strided(tuple(t.shape), tuple(t.stride()))


def _copy(dst, src):
    if dst.dtype == torch.complex32:                          # (few operators take complex32: copy the halves)
        torch.view_as_real(dst).copy_(torch.view_as_real(src))
    else:
        dst.copy_(src)


def delayed(stream, tensors, ms):
    """``(twins, event)``: device tensors of ``tensors`` replaced by poisoned twins that receive the true data on ``stream`` behind a filler of ``ms``; anything
    else (None, host arrays, scalars) is passed through.  ``event`` is recorded behind the filler, in front of the copies."""
    twins = [_poisoned_twin(t) if isinstance(t, torch.Tensor) and t.is_cuda else t for t in tensors]
    torch.cuda.synchronize()                                  # the poison is in place before anything is queued
    ev = filler(stream, ms)
    with torch.cuda.stream(stream):
        for tw, t in zip(twins, tensors):
            if tw is not t:
                _copy(tw, t)
    return twins, ev


def _tup(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def run_delayed(fn, tensors, stream, ms):
    """``fn(*twins)`` under ``torch.cuda.stream(stream)`` behind the delayed producer.  Returns ``(outputs, clones, early)``: the outputs, their clones taken on
    ``stream`` directly behind the call, and whether the wrapper returned while the filler was still running.  Synchronised on return."""
    twins, ev = delayed(stream, tensors, ms)
    with torch.cuda.stream(stream):
        r = fn(*twins)
        early = returned_early(ev)
        clones = tuple(o.clone() for o in _tup(r))
    torch.cuda.synchronize()
    del twins
    return _tup(r), clones, early


def interleaved(calls, s1, s2, ms, reps=3, checks=None):
    """``calls``: at least four callables of growing and shrinking size, each returning a tensor (or a tuple of tensors).  Each is first issued alone on the
    default stream; then, ``reps`` times, all are issued alternately on ``s1`` / ``s2`` behind a filler on both streams (nothing runs until everything is queued, as
    long as the wrappers only enqueue), the assignment swapped between repetitions, every reference held until the synchronise.  Asserts bit equality with the
    lone calls -- or, for call ``k`` with ``checks[k]`` given (an entry that accumulates with float atomics), calls ``checks[k](result)``, the home file's own parity
    check.  Probabilistic for a shared temporary (module docstring)."""
    assert len(calls) >= 4
    checks = checks or [None] * len(calls)
    ref = []
    for c in calls:
        ref.append(tuple(o.clone() for o in _tup(c())))
        torch.cuda.synchronize()
    for rep in range(reps):
        filler(s1, ms)
        filler(s2, ms)
        out = []
        for k, c in enumerate(calls):
            with torch.cuda.stream(s1 if (k + rep) % 2 == 0 else s2):
                out.append(_tup(c()))
        torch.cuda.synchronize()
        for k, (got, want) in enumerate(zip(out, ref)):
            if checks[k] is not None:
                checks[k](got[0] if len(got) == 1 else got)
                continue
            assert len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want)), f"repetition {rep}, call {k}: differs from the same call issued alone"
        del out
