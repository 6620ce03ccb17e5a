"""The frequency-domain adjoint beamformer: the host steps of the reference's ``bfAdjoint`` (``src/UltrasoundSystem.m:3770-4050``) and the call into
``qdas_adjoint`` (``libqdas.so``, ``csrc/adjoint.hip``), which replaces its ``parfor`` over frequency blocks.

``spectrum`` (remodulate, FFT, re-align the time axis), ``select_bins`` (the ``fthresh`` rule) and ``classify_apods`` (which apodization array goes
where) are torch / numpy code and run wherever their inputs live; ``adjoint`` is the thin call over device tensors on torch's current stream.  There
is no CPU fallback for it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["adjoint", "spectrum", "select_bins", "classify_apods", "APOD_TEXT"]

APOD_TEXT = ("Unable to apply apodization ({s}) due to size constraints. Apodization must be scalar in the transmit dimension, "
             "receive dimension, or all image dimensions.")


# ---------------------------------------------------------------------------------------------------------------- host steps (any device)
def spectrum(x, t0, fs, fmod=0.0, Nfft=None, t0_offset=0.0):
    """``X[k, n, v, ...] = FFT_K(x[t, n, v, ...] e^{+2 pi i fmod (t0_v + t / fs)})[k] e^{-2 pi i f_k (t0_v - t0_offset_v)}`` with ``f_k = k fs / K``
    (reference ``:3925-3932``).  ``x``: complex64 torch tensor ``T x N x V x ...``; ``t0`` / ``t0_offset``: scalars or one value per transmit.
    ``K >= T`` zero-pads.  The phase ramps are formed in float64, reduced to a fractional cycle, and applied in complex64."""
    import torch
    T, V = int(x.shape[0]), int(x.shape[2])
    K = T if Nfft is None else int(Nfft)
    if K < T:
        raise DasError(f"bfAdjoint: Nfft ({K}) must be at least the number of samples ({T})")
    dev = x.device
    vec = lambda a: torch.as_tensor(np.broadcast_to(np.asarray(a, np.float64).reshape(-1), (V,)).copy(), device=dev)
    t0v, offv = vec(t0), vec(t0_offset)
    tail = (1,) * (x.ndim - 3)
    ph = lambda cyc: torch.polar(torch.ones_like(cyc), 2.0 * math.pi * (cyc - torch.round(cyc))).to(torch.complex64)
    if fmod:
        t = torch.arange(T, dtype=torch.float64, device=dev).reshape(T, 1, 1) / fs + t0v.reshape(1, 1, V)
        x = x * ph(fmod * t).reshape((T, 1, V) + tail)
    X = torch.fft.fft(x, n=K, dim=0)
    f = torch.arange(K, dtype=torch.float64, device=dev) * (fs / K)
    return X * ph(-f.reshape(K, 1, 1) * (t0v - offv).reshape(1, 1, V)).reshape((K, 1, V) + tail)


def select_bins(X, fs, fthresh=-math.inf):
    """ascending 0-based indices of the frequency bins to evaluate (reference ``:3935-3938``): ``f_k < fs / 2`` and -- with ``fthresh > -inf`` -- some trace
    within ``fthresh`` dB of its own maximum at that bin"""
    import torch
    K = int(X.shape[0])
    keep = torch.arange(K, device=X.device, dtype=torch.float64) * (fs / K) < fs / 2
    if fthresh > -math.inf:
        mag = X.abs().reshape(K, -1)
        db = 20.0 * torch.log10(mag) - 20.0 * torch.log10(mag.amax(dim=0, keepdim=True))
        keep = keep & (db >= fthresh).any(dim=1)
    return np.flatnonzero(keep.cpu().numpy())


def classify_apods(apods, Isz, N, V):
    """``(a_n, a_m, a_mn)`` from apodization arrays broadcastable to ``I1 x I2 x I3 x N x V`` (reference ``:3947-3963``): an array with scalar image
    dimensions is ``a_mn`` (``N x V``, applied to the data), one with a scalar receive dimension is ``a_m`` (``I1 x I2 x I3 x V``), one with a scalar
    transmit dimension is ``a_n`` (``I1 x I2 x I3 x N``); several of one class multiply; ``None`` stands for 1.  Anything else raises the reference's text."""
    full = tuple(Isz) + (N, V)
    out = {"n": None, "m": None, "mn": None}
    for s, a in enumerate(apods, 1):
        a = np.asarray(a.cpu() if hasattr(a, "cpu") else a)
        if a.ndim > 5:
            raise DasError("bfAdjoint: an apodization array has at most 5 dimensions")
        a = a.reshape(a.shape + (1,) * (5 - a.ndim))
        if any(d not in (1, f) for d, f in zip(a.shape, full)):
            raise DasError(f"bfAdjoint: apodization ({s}) of size {a.shape} does not broadcast to {full}")
        if a.shape[:3] == (1, 1, 1):
            key, v = "mn", np.broadcast_to(a[0, 0, 0], (N, V))
        elif a.shape[3] == 1:
            key, v = "m", np.broadcast_to(a[:, :, :, 0, :], tuple(Isz) + (V,))
        elif a.shape[4] == 1:
            key, v = "n", np.broadcast_to(a[:, :, :, :, 0], tuple(Isz) + (N,))
        else:
            raise DasError(APOD_TEXT.format(s=s))
        out[key] = v if out[key] is None else out[key] * v
    return out["n"], out["m"], out["mn"]


# ---------------------------------------------------------------------------------------------------------------- device
def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("qups_amd: no HIP device visible -- the adjoint beamformer has no CPU fallback")
    return torch


def adjoint(X, freq, Pi, Pr, Pt, cinv, del_tx, apod_tx, a_n=None, a_m=None, keep_rx=False, keep_tx=False):
    """``b = I x [N] x [V]`` (complex64 device tensor, pixel fastest in memory) from the selected spectrum ``X`` (``Ksel x V x N`` complex64, contiguous).

    ``freq``: the ``Ksel`` frequencies [Hz]; ``Pi`` / ``Pr`` / ``Pt``: ``3 x I`` / ``3 x N`` / ``3 x M`` positions; ``cinv``: 1 or ``I`` reciprocal sound speeds;
    ``del_tx`` (``M x V``, with ``t0Offset`` added) and ``apod_tx`` (``M x V``); ``a_n`` (``I x N``) / ``a_m`` (``I x V``) or ``None``.  Arrays may be numpy or
    torch; they are put on ``X``'s device in the memory order ``qdas_adjoint`` reads.  The formulas are in ``include/qdas.h``."""
    torch = _torch()
    if not (hasattr(X, "is_cuda") and X.is_cuda):
        raise DasError("adjoint: X must be a device tensor")
    if X.dtype != torch.complex64:
        raise DasError(f"adjoint: complex64 data only, got {str(X.dtype).replace('torch.', '')}")
    if X.ndim != 3:
        raise DasError("adjoint: X must be Ksel x V x N")
    dev = X.device
    X = X.contiguous()
    Ksel, V, N = (int(v) for v in X.shape)
    freq = np.ascontiguousarray(np.asarray(freq, np.float64).reshape(-1))
    if freq.size != Ksel:
        raise DasError(f"adjoint: {freq.size} frequencies for {Ksel} spectrum planes")

    def colmajor(a, dtype, shape, what):                   # a `shape` array -> the device tensor whose memory has the FIRST index fastest
        t = (a if hasattr(a, "is_cuda") else torch.from_numpy(np.array(a))).to(dev, dtype)
        if tuple(t.shape) != tuple(shape):
            raise DasError(f"adjoint: {what} must be {' x '.join(str(v) for v in shape)}, got {tuple(t.shape)}")
        return t.t().contiguous()

    Pi_t = (Pi if hasattr(Pi, "is_cuda") else torch.from_numpy(np.asarray(Pi, np.float64))).to(dev, torch.float32)
    if Pi_t.ndim != 2 or Pi_t.shape[0] != 3:
        raise DasError("adjoint: Pi must be 3 x I")
    I = int(Pi_t.shape[1])
    Pi_t = Pi_t.t().contiguous()
    Pr_t = colmajor(Pr, torch.float32, (3, N), "Pr")
    M = int(np.shape(Pt)[1]) if np.ndim(Pt) == 2 else -1
    Pt_t = colmajor(Pt, torch.float32, (3, M), "Pt")
    cv = (cinv if hasattr(cinv, "is_cuda") else torch.from_numpy(np.asarray(cinv, np.float64).reshape(-1))).to(dev, torch.float32).reshape(-1).contiguous()
    if cv.numel() not in (1, I):
        raise DasError(f"adjoint: cinv holds 1 or I = {I} values, got {cv.numel()}")
    del_t = colmajor(del_tx, torch.float64, (M, V), "del_tx")
    apod_t = colmajor(apod_tx, torch.float32, (M, V), "apod_tx")
    an_t = None if a_n is None else colmajor(a_n, torch.float32, (I, N), "a_n")
    am_t = None if a_m is None else colmajor(a_m, torch.float32, (I, V), "a_m")
    shape = ((V,) if keep_tx else ()) + ((N,) if keep_rx else ()) + (I,)
    b = torch.empty(shape, dtype=torch.complex64, device=dev)
    d = _lib.AdjointDesc()
    d.I, d.N, d.M, d.V, d.Ksel = I, N, M, V, Ksel
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d.Pi, d.Pr, d.Pt, d.cinv, d.cinv_count = ptr(Pi_t), ptr(Pr_t), ptr(Pt_t), ptr(cv), cv.numel()
    d.freq = freq.ctypes.data_as(C.c_void_p)
    d.del_tx, d.apod_tx, d.a_n, d.a_m = ptr(del_t), ptr(apod_t), ptr(an_t), ptr(am_t)
    d.keep_rx, d.keep_tx, d.dtype = int(bool(keep_rx)), int(bool(keep_tx)), _lib.QDAS_F32
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_adjoint(C.byref(d), C.c_void_p(X.data_ptr()), C.c_void_p(b.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return b.permute(*reversed(range(b.ndim)))
