"""REFoCUS: channel data of a transmit sequence (plane waves, focused beams, a coded aperture) back to full-synthetic-aperture (FSA) data -- the reference's
``UltrasoundSystem.refocus`` (``src/UltrasoundSystem.m:3505-3768``), the inverse of ``focusTx``.

``decoder`` builds the decoding pages ``Hi_k`` (``M x V`` per frequency) on the host in float64: they depend on the sequence only, so a stream of frames
pays them once (``Decoder`` keeps the device copy).  ``refocus`` applies them per frame with ``qdas_refocus`` (``libqdas.so``, ``csrc/refocus.hip``: time FFT in
LDS, the per-frequency products on the f32 matrix cores, inverse FFT in LDS); ``compose`` is the same contract from ``torch.fft`` and ``torch.einsum`` -- the
route for complex128 data and for record lengths the kernels do not take, and the baseline ``tools/refocus_time.py`` measures.  There is no CPU fallback.

With ``f_k = k fs / T`` for ``k = 0 .. T-1`` (``ChannelData.fftaxis``, ``src/ChannelData.m:1491``: NOT wrapped to negative frequencies -- this matters for every
non-integer ``tau fs`` and ``t0 fs``), ``tau`` and ``apd`` the sequence's delays and apodization (``M x V``: elements x pulses):

    H_k[v, m] = apd[m, v] exp(-2 pi i f_k tau[m, v])                  w_k = sigma_max(H_k)^-2
    adjoint:   Hi_k = w_k H_k^T                                       (the plain transpose, as in the reference)
    tikhonov:  Hi_k = (H_k^H H_k + gamma w_k I_M) \\ H_k^T            (default gamma = 10 (N / 10)^2, N the receiver count: the reference's code, not its help text)
    pinv:      Hi_k = w_k pinv(H_k)                                   (MATLAB's cutoff max(V, M) eps(sigma_max))
    a page with sigma_max = 0 gives Hi_k = 0                          (the reference's NaN -> 0)
    X = FFT_t(x) exp(-2 pi i f_k t0[v]);   Y_k[n, m] = sum_v Hi_k[m, v] X_k[n, v];   y = IFFT_t(Y exp(+2 pi i f_k min(t0)))

The reference writes ``eye(chd.N)`` and loops to ``chd.N`` where the element count ``M`` is meant (it only runs when ``N == M``); ``M`` is used here.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["decoder", "Decoder", "refocus", "fused", "compose", "takes", "default_gamma", "METHODS"]

METHODS = ("tikhonov", "adjoint", "pinv")


def default_gamma(N):
    """``10 (N / 10)^2`` with ``N`` the receiver count (reference ``:3677``)"""
    return 10.0 * (float(N) / 10.0) ** 2


# ---------------------------------------------------------------------------------------------------------------- the decoder (numpy, float64)
def _tau_apd(tau, apd):
    tau = np.asarray(tau, np.float64)
    if tau.ndim != 2:
        raise DasError(f"refocus: tau must be M x V (elements x pulses), got shape {tau.shape}")
    try:
        apd = np.broadcast_to(np.asarray(apd, np.float64 if not np.iscomplexobj(apd) else np.complex128), tau.shape)
    except ValueError:
        raise DasError(f"refocus: the apodization {np.shape(apd)} does not broadcast to the delays {tau.shape}") from None
    return tau, apd


def encoding(tau, apd, T, fs):
    """``H`` (``T x V x M``, complex128): the encoding pages ``H_k[v, m] = apd[m, v] exp(-2 pi i f_k tau[m, v])``"""
    tau, apd = _tau_apd(tau, apd)
    f = np.arange(int(T)) * float(fs) / int(T)
    return apd.T[None] * np.exp(-2j * np.pi * f[:, None, None] * tau.T[None])


def decoder(tau, apd, T, fs, method="tikhonov", gamma=None, N=None):
    """``Hi`` (``M x V x T``, complex128) from the sequence's ``tau`` and ``apd`` (``M x V``), the record length ``T`` and ``fs``.  ``gamma`` defaults to
    ``10 (N / 10)^2`` (``N``: the receiver count, default ``M``) and is read by ``tikhonov`` only.  Batched over frequency; ``pinv`` loops."""
    if method not in METHODS:
        raise DasError(f"refocus: method must be one of {METHODS}, got {method!r}")
    H = encoding(tau, apd, T, fs)                                       # T x V x M
    T, V, M = H.shape
    if gamma is None:
        gamma = default_gamma(M if N is None else N)
    gamma = float(gamma)
    if not gamma >= 0.0:
        raise DasError("refocus: gamma must be non-negative")
    Ht = np.swapaxes(H, 1, 2)                                           # T x M x V: the plain transpose
    G = np.conj(Ht) @ H if M <= V or method == "tikhonov" else H @ np.conj(Ht)      # H^H H (M x M), or H H^H (V x V) when that is the smaller one
    lmax = np.linalg.eigvalsh(G)[:, -1] if T else np.zeros(0)           # sigma_max^2: the largest eigenvalue of the Gram matrix (a third of the time of an SVD of H)
    live = lmax > 0
    w = np.zeros(T)
    w[live] = 1.0 / lmax[live]
    if method == "adjoint":
        Hi = Ht * w[:, None, None]
    elif method == "tikhonov":
        A = G + (gamma * w)[:, None, None] * np.eye(M)                  # H^H H + gamma w I
        A[~live] = np.eye(M)
        Hi = np.linalg.solve(A, Ht)
        Hi[~live] = 0
    else:
        Hi = np.zeros((T, M, V), np.complex128)
        for k in np.flatnonzero(live):
            U, s, Vh = np.linalg.svd(H[k], full_matrices=False)
            keep = s > max(V, M) * np.spacing(s[0])
            Hi[k] = w[k] * (np.conj(Vh[keep].T) * (1.0 / s[keep])) @ np.conj(U[:, keep].T)
    return np.ascontiguousarray(np.transpose(Hi, (1, 2, 0)))


_build = decoder         # (`refocus` has a parameter of the function's name)


class Decoder:
    """The decoding pages of one sequence: ``Hi`` (``M x V x T`` complex128, host) and, made on first use and kept, the complex64 device copy in the order
    ``qdas_refocus`` reads (``m`` fastest, then ``v``, then ``k``).  ``device_copy``: a caller's own ``T x V x M`` contiguous complex64 device tensor to use
    instead (a producer on another stream may still be writing it)."""

    def __init__(self, Hi, device_copy=None):
        Hi = np.asarray(Hi)
        if Hi.ndim != 3:
            raise DasError(f"refocus: Hi must be M x V x T, got shape {Hi.shape}")
        self.Hi = Hi.astype(np.complex128, copy=False)
        self.M, self.V, self.T = (int(v) for v in Hi.shape)
        self._dev = {}
        self._lock = threading.Lock()
        if device_copy is not None:
            if tuple(device_copy.shape) != (self.T, self.V, self.M) or not device_copy.is_contiguous() or str(device_copy.dtype) != "torch.complex64":
                raise DasError("refocus: device_copy must be a contiguous T x V x M complex64 tensor")
            self._dev[(str(device_copy.device), device_copy.dtype)] = device_copy

    def on(self, device, dtype=None):
        """the ``T x V x M`` contiguous device tensor (complex64 unless ``dtype`` says complex128), for work queued on torch's CURRENT stream of ``device``.
        The copy lies in the allocator pool of the stream that built it and the caller never sees it: every call tells the allocator that the current stream
        reads it too (``record_stream``, no host wait), so that a Decoder that is dropped while a call is still queued on another stream -- the one
        ``UltrasoundSystem.refocus`` keeps, when its key changes -- does not hand the block to the next allocation before that call has passed."""
        import torch
        dtype = dtype or torch.complex64
        key = (str(device), dtype)
        with self._lock:
            t = self._dev.get(key)
            if t is None:
                h = np.ascontiguousarray(np.transpose(self.Hi, (2, 1, 0)))
                t = self._dev[key] = torch.from_numpy(h).to(device=device, dtype=dtype).contiguous()
            if t.is_cuda:
                t.record_stream(torch.cuda.current_stream(t.device))
            return t


# ---------------------------------------------------------------------------------------------------------------- device
def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("qups_amd: no HIP device visible -- refocus has no CPU fallback")
    return torch


def takes(T):
    """whether ``qdas_refocus`` runs this record length in LDS (asked of the library itself: its dedicated return code; needs no device)"""
    d = _lib.RefocusDesc()
    d.T, d.N, d.V, d.M, d.frames, d.fs, d.device, d.one_t0 = int(T), 1, 1, 1, 1, 1.0, -1, 1
    return _lib.lib().qdas_refocus(C.byref(d), None, None, None, None, 0) != _lib.QDAS_ENOTLDS


_T0 = {}            # the last per-pulse t0 on a device: (device, bytes) -> tensor
_T0_LOCK = threading.Lock()


def _t0_device(t0, dev):
    """per-pulse start times as a device tensor, for work queued on torch's current stream of ``dev``.  A host array has no stream: the first upload of a table
    is a pageable copy that returns when the caller's stream has reached it; the copy is then kept, so that a stream of frames with the same ``t0`` only
    enqueues work (its content is complete for any stream: the upload had finished when it returned).  The copy belongs to the allocator pool of the stream
    that built it: every use records the consuming stream (``record_stream``, as ``interpd._shift_tables`` does), so that a table evicted by another ``t0`` is
    not handed out again -- and overwritten by the next upload -- before the call queued here has read it.  Lookup, eviction and insert are one critical section."""
    import torch
    key = (str(dev), t0.tobytes())
    with _T0_LOCK:
        t = _T0.get(key)
        if t is None:
            _T0.clear()
            t = _T0[key] = torch.from_numpy(np.ascontiguousarray(t0)).to(dev)
        t.record_stream(torch.cuda.current_stream(t.device))
        return t


def _args(x, t0, dec=None):
    torch = _torch()
    if not (hasattr(x, "is_cuda") and x.is_cuda):
        raise DasError("refocus: x must be a device tensor")
    if x.dtype in (torch.float16, torch.bfloat16, torch.complex32):
        raise DasError("refocus: half precision is insufficient for frequency-domain processing (complex64 or complex128 data)")
    if x.dtype == torch.float32:
        x = x.to(torch.complex64)
    elif x.dtype == torch.float64:
        x = x.to(torch.complex128)
    if x.dtype not in (torch.complex64, torch.complex128):
        raise DasError(f"refocus: floating-point data only, got {str(x.dtype).replace('torch.', '')}")
    if x.ndim < 3:
        x = x.reshape(tuple(x.shape) + (1,) * (3 - x.ndim))
    T, N, V = (int(v) for v in x.shape[:3])
    t0 = np.asarray(t0, np.float64).reshape(-1)
    if t0.size not in (1, V) or not np.all(np.isfinite(t0)):
        raise DasError(f"refocus: t0 holds 1 or V = {V} finite values, got {t0.size}")
    if dec is not None and (dec.V, dec.T) != (V, T):
        raise DasError(f"refocus: the decoder is for {dec.V} pulses and {dec.T} samples, the data has {V} and {T}")
    return torch, x, T, N, V, t0


def fused(x, t0, fs, dec):
    """``y`` (``T x N x M x frames...`` complex64) from ``x`` (``T x N x V x frames...`` complex64 device tensor) and a ``Decoder``: ``qdas_refocus`` on torch's
    current stream; the work space is a ``torch.empty``.  Record lengths outside the in-LDS path raise ``QdasError`` with code ``QDAS_ENOTLDS``."""
    torch, x, T, N, V, t0 = _args(x, t0, dec)
    if x.dtype != torch.complex64:
        raise DasError(f"refocus: the fused path takes complex64 data, got {str(x.dtype).replace('torch.', '')}")
    dev = x.device
    Fsz = tuple(int(v) for v in x.shape[3:])
    frames = int(np.prod(Fsz)) if Fsz else 1
    M = dec.M
    xc = x.permute(*reversed(range(x.ndim))).contiguous()      # memory: time fastest, then n, v, frames
    if 0 in (T, N, V, M, frames):                              # no elements, or an empty sum over the pulses: the library launches nothing
        return torch.zeros((T, N, M) + Fsz, dtype=torch.complex64, device=dev)
    y = torch.empty(Fsz[::-1] + (M, N, T), dtype=torch.complex64, device=dev)
    Hi = dec.on(dev)
    t0_t = None if t0.size == 1 else _t0_device(t0, dev)       # (one value: the two phases cancel and the library reads none)
    d = _lib.RefocusDesc()
    d.T, d.N, d.V, d.M, d.frames = T, N, V, M, frames
    d.fs, d.t0_out, d.one_t0 = float(fs), float(t0.min()), int(t0.size == 1)
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.t0 = None if t0_t is None else C.c_void_p(t0_t.data_ptr())
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    nbytes = C.c_uint64()
    _lib.check(L.qdas_refocus_work_bytes(C.byref(d), C.byref(nbytes)))
    work = torch.empty(max(1, (nbytes.value + 7) // 8), dtype=torch.complex64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.qdas_refocus(C.byref(d), C.c_void_p(xc.data_ptr()), C.c_void_p(Hi.data_ptr()), C.c_void_p(y.data_ptr()),
                                  C.c_void_p(work.data_ptr()), work.numel() * 8))
    return y.permute(*reversed(range(y.ndim)))


def compose(x, t0, fs, dec):
    """the same contract from ``torch.fft`` and ``torch.einsum`` in the data's precision (float32 / float64 data become complex)"""
    torch, x, T, N, V, t0 = _args(x, t0, dec)
    dev = x.device
    Fsz = tuple(int(v) for v in x.shape[3:])
    xr = x.reshape(T, N, V, -1)
    Hi = dec.on(dev, x.dtype)                                   # T x V x M
    X = torch.fft.fft(xr, dim=0)
    if t0.size > 1:
        f = np.arange(T) * float(fs) / T
        turns = f[:, None] * t0[None, :]
        turns -= np.rint(turns)
        X = X * torch.from_numpy(np.exp(-2j * np.pi * turns)).to(dev, x.dtype).reshape(T, 1, V, 1)
    Y = torch.einsum("tvm,tnvf->tnmf", Hi, X)
    if t0.size > 1:
        turns = f * t0.min()
        turns -= np.rint(turns)
        Y = Y * torch.from_numpy(np.exp(2j * np.pi * turns)).to(dev, x.dtype).reshape(T, 1, 1, 1)
    return torch.fft.ifft(Y, dim=0).reshape((T, N, dec.M) + Fsz)


def refocus(x, t0, fs, tau=None, apd=None, method="tikhonov", gamma=None, decoder=None):
    """``(y, t0_out, Hi)``: the FSA data ``y`` (``T x N x M x frames...``, complex, on ``x``'s device), the time of its sample 0 ``min(t0)`` and the decoding
    pages ``Hi`` (``M x V x T`` complex128, host).  ``x``: ``T x N x V x frames...`` device tensor (float32 is cast to complex64, float64 to complex128; half
    precision is refused); ``t0``: a scalar or one value per pulse; ``tau`` / ``apd``: the sequence's delays and apodization (``M x V``), or a ready ``Decoder``.
    complex64 data of a length ``takes`` accepts runs ``fused``; complex128 data and every other length run ``compose``.

    As measured today (``profiles/refocus_time.txt``) ``fused`` is about level with ``compose`` at ``N = M = 64, V = 32`` (1.05 x) and SLOWER at
    ``N = M = V = 128`` (0.81 x): where speed matters at large ``M`` and ``V``, ``compose(x, t0, fs, Decoder(...))`` is currently the faster call, with the
    same result to 6e-7.  The route stays on the kernels (a missing kernel is an error, never a quiet composition); DESIGN.md 9 lists what closes the gap."""
    torch, x, T, N, V, t0 = _args(x, t0, decoder)
    dec = decoder if decoder is not None else Decoder(_build(tau, apd, T, fs, method, gamma, N))
    if x.dtype == torch.complex64 and takes(T):
        y = fused(x, t0, fs, dec)
    else:
        y = compose(x, t0, fs, dec)
    return y, float(t0.min()), dec.Hi
