"""Pre-processing in front of the DAS path, on the device: ``hilbert`` (+ fused ``downmix``) of real RF traces.

Mirrors ``ChannelData.hilbert`` (reference src/ChannelData.m:935-966) and ``ChannelData.downmix`` (:757-766) for data whose time
axis is the first dimension.  The work is done by ``libqdas.so`` (qups_amd/csrc/pre.hip: a one-pass LDS-resident FFT kernel for
record lengths with prime factors up to 13, hipFFT passes for the rest); there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


# Plans by shape: a qdas_pre_plan owns its twiddles -- and, for record lengths the one-pass kernel does not take (a prime factor above 13, more than 8192
# samples), two hipFFT plans and three work buffers whose creation costs 11-15 ms (profiles/r04/general_time.txt) against 0.1-0.7 ms of transform.  A frame
# loop calls hilbert() with ONE shape: the last few plans are kept, destroyed on eviction and at interpreter exit.
_PLANS: "dict[tuple, _Entry]" = {}          # key -> entry (plan handle, the plan's own lock, use count, dead flag)
_PLAN_CACHE_MAX = 8
_plans_lock = __import__("threading").Lock()      # guards the DICTIONARY and the entries' use counts only (it used to be held across execute + stream synchronisation: every hilbert() of every device and thread in a row)


class _Entry:
    """One cached plan.  ``users`` counts the hilbert() calls between _pre_plan and _release; ``dead`` is set when the entry leaves the dictionary.  Both change
    under _plans_lock only, and the plan is destroyed by whoever finds ``dead and users == 0``: an eviction or clear_pre_plan_cache() between a caller's
    _pre_plan and its execute leaves the plan alive until that caller is done."""
    __slots__ = ("h", "lock", "users", "dead")

    def __init__(self, h):
        self.h, self.lock, self.users, self.dead = h, __import__("threading").Lock(), 0, False


def _destroy(e):
    with e.lock:                                  # (never under a running execute)
        try:
            _lib.lib().qdas_pre_plan_destroy(e.h)
        except Exception:                         # (interpreter exit: the HIP runtime may be gone before this hook runs)
            pass


def _retire(entries):
    """under _plans_lock: mark the entries dead; returns those nobody uses (to destroy once the lock is released)"""
    idle = []
    for e in entries:
        e.dead = True
        if e.users == 0:
            idle.append(e)
    return idle


def clear_pre_plan_cache():
    with _plans_lock:
        idle = _retire(list(_PLANS.values()))
        _PLANS.clear()
    for e in idle:
        _destroy(e)


def _at_exit():
    try:
        clear_pre_plan_cache()
    except Exception:
        pass


__import__("atexit").register(_at_exit)


def _pre_plan(key, d):
    """the entry of this shape with its use count raised (hand it back with _release): created on a miss, the oldest entry evicted beyond _PLAN_CACHE_MAX
    (destroyed once no hilbert() holds it)"""
    L = _lib.lib()
    with _plans_lock:
        e = _PLANS.pop(key, None)
        if e is None:
            h = C.c_void_p()
            _lib.check(L.qdas_pre_plan_create(C.byref(h), C.byref(d)))
            hilbert.plans_created = getattr(hilbert, "plans_created", 0) + 1
            e = _Entry(h)
        _PLANS[key] = e                                              # (most recently used last)
        e.users += 1
        evicted = []
        while len(_PLANS) > _PLAN_CACHE_MAX:
            evicted.append(_PLANS.pop(next(iter(_PLANS))))
        idle = _retire(evicted)
    for v in idle:
        _destroy(v)
    return e


def _release(e):
    with _plans_lock:
        e.users -= 1
        last = e.dead and e.users == 0
    if last:
        _destroy(e)


def hilbert(x, N: int | None = None, fdown: float = 0.0, t0: float = 0.0, fs: float | None = None, device=None):
    """Analytic signal along dim 0 of real ``x`` (``T x ...``; float32 or int16; numpy array or torch tensor), transform length
    ``N`` (default ``T``; zero-padded or truncated like MATLAB's ``hilbert(x, N)``); with ``fdown`` the result is also multiplied by
    ``exp(-2j*pi*fdown*(t0 + k/fs))``.  Returns a complex64 torch tensor ``N x ...`` on the device.

    Traces are transformed in pairs.  With the trailing dimensions flattened in row-major order (``k = n * M + m`` for ``T x N x M``), traces ``2j`` and ``2j + 1``
    ride ONE complex transform ``z = x1 + i x2`` (what makes this one pass over HBM); an odd count leaves the last trace alone, and with an odd channel count pairs
    straddle transmits.  What follows from that, and is tested (``tests/test_gpu_neighbours.py``):

    * the real part of every trace is its input, bit for bit (without ``fdown``), whatever its partner holds;
    * ``H x1 = Im(..) - x2`` and ``H x2 = x1 - Re(..)`` cancel against the partner, so the rounding error of a trace is relative to the LARGER of the two: measured at
      most 5.5e-7 of the pair's ``max|y|`` on an MI355X (each pair scaled as a unit by 2^0, 2^20, 2^-20 or 2^7) -- so a trace 2^10 below its partner carries about 1e-4 of its OWN maximum,
      one 2^20 below about 0.15 (a float32 restatement of the packing on the CPU gives 9.2e-5 .. 1.6e-4 and 0.14 .. 0.15 at N = 256 and 2816), and an all-zero trace
      gets its partner's rounding noise as imaginary part.  Scale a quiet trace up first if that matters;
    * a NaN or Inf sample turns the imaginary part of BOTH traces of its pair non-finite at all ``N`` samples, and changes no bit of any other pair;
    * scaling a pair by a power of two scales its result exactly.

    Lengths the one-pass kernel does not serve (a prime factor above 13, stages too wide, more than 8192 samples), and every length under
    ``QDAS_PRE_HIPFFT=1``, go through hipFFT trace by trace: there each trace depends on itself alone.  So whether two neighbours couple depends on ``N``.

    ``t0``, ``fs`` and ``fdown`` are constants of the underlying plan (``qdas_pre_desc``), so they are part of the plan cache's key: a frame loop whose ``t0`` changes
    per frame creates a plan per value (0.1 ms on the one-pass path, 11-15 ms where hipFFT plans are made) -- downmix with ``t0 = 0`` and multiply the frame by the
    scalar ``exp(-2j*pi*fdown*t0)`` instead."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("qups_amd: no HIP device visible -- hilbert has no CPU fallback")
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if xt.is_complex():
        raise ValueError("hilbert expects real data")
    if xt.dtype not in (torch.float32, torch.int16):
        xt = xt.to(torch.float32)
    T = int(xt.shape[0])
    rest = tuple(int(v) for v in xt.shape[1:])
    K = int(np.prod(rest)) if rest else 1
    N = T if N is None else int(N)
    if fdown and not fs:
        raise ValueError("Undefined sampling rate.")
    from .das_spec import _colmajor
    x2 = xt.to(dev).reshape(T, K)
    # already time-fastest (a MATLAB-ordered view; a CONTIGUOUS single trace): no copy.  A strided single trace -- hilbert(x[:, j]) of a
    # T x N tensor, x[::2] -- has K == 1 but stride(0) != 1: the library reads T consecutive elements, so it is copied like the rest.
    if T > 0 and ((K == 1 and x2.stride(0) == 1) or (K > 1 and x2.stride() == (1, T))):
        xc = x2.t()
    else:
        xc = _colmajor(x2.contiguous())                             # K x T: time fastest (MATLAB memory order of T x K)
    y = torch.empty((K, N), dtype=torch.complex64, device=dev)
    d = _lib.PreDesc(T, K, N, _lib.QDAS_PRE_I16 if xt.dtype == torch.int16 else _lib.QDAS_PRE_F32,
                     dev.index if dev.index is not None else torch.cuda.current_device(), float(fs or 0.0), float(t0), float(fdown))
    L = _lib.lib()
    key = (T, K, N, int(d.in_type), int(d.device), float(d.fs), float(d.t0), float(d.fdown), __import__("os").environ.get("QDAS_PRE_HIPFFT"))      # (the switch is read at plan creation: part of the key)
    e = _pre_plan(key, d)
    try:
        with torch.cuda.device(dev), e.lock:                        # (one execute at a time per PLAN: its hipFFT work buffers are the plan's; other shapes / devices run beside it)
            hilbert.last_one_pass = bool(L.qdas_pre_plan_one_pass(e.h))   # which path served the last call (tests / tools)
            _lib.check(L.qdas_pre_execute(e.h, C.c_void_p(xc.data_ptr()), C.c_void_p(y.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.current_stream().synchronize()
    finally:
        _release(e)                                                 # (an entry evicted meanwhile is destroyed here, by its last user)
    return y.t().reshape((N,) + rest)
