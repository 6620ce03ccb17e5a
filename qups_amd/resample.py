"""Rational-rate polyphase FIR on the device: ``upfirdn``, ``resample`` and the FIR ``filtfilt`` (the reference's ``resample`` and ``filtfilt``,
``src/ChannelData.m:1059-1094``, ``:890-909``) on ``csrc/resample.hip``.  ``include/qdas.h`` states the one contract behind all of them:

    out[j, ...] = sum_i h[off + j q - i p] X[i, ...],    over every integer i with 0 <= off + j q - i p < K

with ``X = x`` inside the record and zeros or the odd reflection outside.

* :func:`upfirdn` -- ``scipy.signal.upfirdn``: ``off = 0``, ``ceil(((T - 1) p + K) / q)`` outputs.
* :func:`resample` -- MATLAB's uniform ``resample(x, p, q, n, beta)`` / ``scipy.signal.resample_poly``: ``off = (K - 1) / 2``, ``ceil(T p / q)`` outputs,
  output ``j`` at input time ``j q / p``.  :func:`resample_taps` is its default design.
* :func:`filtfilt` -- MATLAB's and scipy's zero-phase ``filtfilt(b, 1, x)`` for an FIR ``b``: ONE convolution with ``b * flip(b)`` over the odd extension.

Time is along dim 0, tensors stay on the device and there is no CPU fallback: without the library or a device the call raises.

The package exports the FUNCTION under this module's name (``qups_amd.resample(x, p, q)``); the module is ``importlib.import_module("qups_amd.resample")``."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["upfirdn", "resample", "resample_taps", "resample_len", "upfirdn_len", "filtfilt", "filtfilt_taps", "polyphase", "MAX_TAPS", "MAX_RATE"]

MAX_TAPS, MAX_RATE = _lib.RESAMPLE_MAX_K, _lib.RESAMPLE_MAX_PQ


def resample_len(T: int, p: int, q: int) -> int:
    """``ceil(T p / q)``"""
    return -(-int(T) * int(p) // int(q))


def upfirdn_len(T: int, K: int, p: int, q: int) -> int:
    """``ceil(((T - 1) p + K) / q)``"""
    return -(-((int(T) - 1) * int(p) + int(K)) // int(q)) if T > 0 else 0


def _rate(p, q):
    if int(p) != p or int(q) != q or int(p) < 1 or int(q) < 1:
        raise DasError(f"the rate is p / q with positive integers, got p = {p}, q = {q}")
    g = math.gcd(int(p), int(q))
    return int(p) // g, int(q) // g


def resample_taps(p, q, n=10, beta=5.0):
    """MATLAB's documented default design of ``resample(x, p, q, n, beta)``: ``L = 2 n max(p, q) + 1`` taps,
    ``firls(L - 1, [0 2fc 2fc 1], [1 1 0 0]) .* kaiser(L, beta)'`` with ``fc = 1 / (2 max(p, q))``, scaled to ``p h / sum(h)``.  With its zero-width transition
    band the least-squares design is the truncated ideal low-pass, so the taps have the closed form ``sinc((k - (L - 1) / 2) / max(p, q)) kaiser[k]``, which
    is what this computes (float64).  There is no MATLAB to pin the taps against: the tests hold them to the closed form, to ``scipy.signal.firls`` times the
    window, to symmetry and to the sum ``p``.  ``p, q`` are reduced by their gcd; ``p = q`` has no band to design and is refused."""
    p, q = _rate(p, q)
    if p == q:
        raise DasError("resample_taps: p = q is the identity; there is no filter to design")
    n = int(n)
    if n < 1:
        raise DasError("resample_taps: n must be at least 1")
    pq = max(p, q)
    L = 2 * n * pq + 1
    k = np.arange(L, dtype=np.float64) - (L - 1) / 2
    g = np.sinc(k / pq) * np.kaiser(L, float(beta))
    return p * g / g.sum()


def filtfilt_taps(b):
    """``b * flip(b)`` in float64: the ``2 K - 1`` taps of the zero-phase filter, its centre at ``K - 1``"""
    b = np.asarray(b, np.float64).reshape(-1)
    return np.convolve(b, b[::-1])


def polyphase(h, x, p, q, off, J, edge="zero"):
    """The contract itself: ``x`` (``T x ...``, a device tensor: int16, float32, complex64, float64 or complex128), real taps ``h``, ``J`` outputs at rate
    ``p / q`` from tap offset ``off``; ``edge`` is ``'zero'`` or ``'odd'``.  The result is ``J x ...``, float32 for int16 data and of the data's type otherwise,
    time-fastest in memory like ``demod``'s; an ``x`` that is not time-fastest is brought there by ONE transposing copy, ``x.movedim(0, -1).contiguous()``.
    Queued on torch's current stream; nothing synchronises when ``h`` is already a device tensor."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise DasError("resample: x must be a device tensor (there is no CPU fallback in this package)")
    types = {torch.int16: _lib.RESAMPLE_I16, torch.float32: _lib.RESAMPLE_F32, torch.complex64: _lib.RESAMPLE_C64, torch.float64: _lib.RESAMPLE_F64,
             torch.complex128: _lib.RESAMPLE_C128}
    if x.dtype not in types:
        raise DasError(f"resample: x is int16, float32, complex64, float64 or complex128, got {str(x.dtype).replace('torch.', '')}")
    if x.ndim < 1:
        raise DasError("resample: x needs a time dimension")
    if edge not in ("zero", "odd"):
        raise DasError(f"resample: edge is 'zero' or 'odd', got {edge!r}")
    dbl = x.dtype in (torch.float64, torch.complex128)
    dev = x.device
    rdt = torch.float64 if dbl else torch.float32
    ht = h if isinstance(h, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(h, np.float64)))
    if ht.is_complex():
        raise DasError("resample: the taps must be real")
    ht = ht.reshape(-1).to(device=dev, dtype=rdt).contiguous()
    K = int(ht.numel())
    if K < 1:
        raise DasError("resample: the filter needs at least one tap")
    T = int(x.shape[0])
    rest = tuple(int(v) for v in x.shape[1:])
    Cn = int(np.prod(rest, dtype=np.int64)) if rest else 1
    J = int(J)
    xc = x.movedim(0, -1).contiguous().reshape(Cn, T)                # C x T, time fastest: a view when x already is, else the one copy
    odt = torch.float32 if x.dtype == torch.int16 else x.dtype
    y = torch.empty((Cn, J), dtype=odt, device=dev)
    d = _lib.ResampleDesc()
    d.T, d.C, d.K, d.J = T, Cn, K, J
    d.p, d.q, d.off = int(p), int(q), int(off)
    d.x_ld, d.out_ld = T, J
    d.in_type, d.edge = types[x.dtype], _lib.RESAMPLE_ODD if edge == "odd" else _lib.RESAMPLE_ZERO
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_resample(C.byref(d), C.c_void_p(xc.data_ptr()), C.c_void_p(ht.data_ptr()), C.c_void_p(y.data_ptr())))
    return y.t().reshape((J,) + rest)


def upfirdn(h, x, up=1, down=1):
    """``scipy.signal.upfirdn(h, x, up, down, axis=0)`` on the device: zero-stuff by ``up``, filter with ``h``, keep every ``down``-th sample -- without the
    zeros.  ``up, down`` are taken as given: they need not be coprime, and scipy does not reduce them either."""
    if int(up) != up or int(down) != down or int(up) < 1 or int(down) < 1:
        raise DasError(f"upfirdn: up and down are positive integers, got {up}, {down}")
    K = int(h.numel()) if hasattr(h, "numel") else int(np.size(h))
    T = int(x.shape[0]) if hasattr(x, "shape") and len(x.shape) else 0
    return polyphase(h, x, int(up), int(down), 0, upfirdn_len(T, K, up, down))


def resample(x, p, q, n=10, beta=5.0, h=None):
    """MATLAB's uniform ``resample(x, p, q, n, beta)`` / ``scipy.signal.resample_poly(x, p, q, window=h / p)`` along dim 0: ``ceil(T p / q)`` samples, output
    ``j`` at input time ``j q / p``, the filter's delay removed, zeros outside the record.  ``p, q`` are reduced by their gcd; ``p = q`` returns a copy.
    ``h``: odd-length taps to use instead of :func:`resample_taps` (already scaled by ``p``)."""
    import torch
    p, q = _rate(p, q)
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise DasError("resample: x must be a device tensor (there is no CPU fallback in this package)")
    if p == q:
        return x.clone()
    if h is None:
        h = resample_taps(p, q, n, beta)
    K = int(h.numel()) if hasattr(h, "numel") else int(np.size(h))
    if K % 2 != 1:
        raise DasError(f"resample: the taps must have odd length (the delay (K - 1) / 2 is removed), got {K}")
    return polyphase(h, x, p, q, (K - 1) // 2, resample_len(int(x.shape[0]), p, q))


def filtfilt(b, x):
    """Zero-phase filtering with the real FIR taps ``b`` along dim 0: MATLAB's ``filtfilt(b, 1, x)`` and ``scipy.signal.filtfilt(b, 1, x, padlen=3 (K - 1))``.
    For an FIR filter both are exactly one convolution with ``b * flip(b)`` over the record extended by odd reflection -- the pad of ``3 (K - 1)`` samples and
    the initial conditions never reach the samples that are kept -- so this is one pass, not two.  Needs ``T > 3 (K - 1)``, as MATLAB demands."""
    bb = (b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b))
    if np.iscomplexobj(bb):
        raise DasError("filtfilt: the taps b must be real")
    bb = np.asarray(bb, np.float64).reshape(-1)
    K = bb.size
    if K < 1:
        raise DasError("filtfilt: the filter needs at least one tap")
    T = int(x.shape[0]) if hasattr(x, "shape") and len(x.shape) else 0
    if T <= 3 * (K - 1):
        raise DasError(f"filtfilt: the record must have more than 3 (K - 1) = {3 * (K - 1)} samples, it has {T}")
    return polyphase(filtfilt_taps(bb), x, 1, 1, K - 1, T, edge="odd")
