"""Plane-wave Stolt f-k migration: the host steps of the reference's ``bfMigration`` (``src/UltrasoundSystem.m:4675-4887``), the call into
``qdas_migration`` (``libqdas.so``, ``csrc/migration.hip``: four passes, FFTs resident in LDS) and the same contract composed from ``torch.fft``
and ``qups_amd.wsinterpd`` -- the route for transform lengths the kernels do not take, and the baseline ``tools/migration_time.py`` measures.

``axes``, ``stolt_indices`` and ``gamma`` are numpy float64; ``migrate`` and ``compose`` work on device tensors on torch's current stream.
There is no CPU fallback.

The Stolt index is evaluated as ``j0 = j - floor(F/2)``, ``a = kx cs F / fs``, ``kkz = sign(j0) sqrt(a^2 + j0^2) + floor(F/2)``: algebraically the
reference's ``(fkz - f(1)) F / fs``, but exact on the ``kx = 0`` column and the ``f = 0`` row.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["axes", "stolt_indices", "gamma", "migrate", "compose", "bmode", "takes"]


# ---------------------------------------------------------------------------------------------------------------- host steps (numpy, float64)
def axes(F, K, fs, pitch):
    """``(f, kx)``: the shifted frequency axes ``((0:F-1) - floor(F/2)) / F * fs`` and ``((0:K-1) - floor(K/2)) / K / pitch`` (reference ``:4773-4774``)"""
    F, K = int(F), int(K)
    return (np.arange(F) - F // 2) / F * fs, (np.arange(K) - K // 2) / K / pitch


def stolt_indices(F, K, fs, pitch, c0):
    """``kkz`` (``F x K``, float64): the 0-based fractional index into the shifted spectrum at which output frequency ``j`` of column ``k`` is sampled"""
    F, K = int(F), int(K)
    j0 = (np.arange(F) - F // 2).astype(np.float64)[:, None]
    _, kx = axes(F, K, fs, pitch)
    a = (kx * (c0 / math.sqrt(2.0)) * F / fs)[None, :]
    return np.sign(j0) * np.sqrt(a * a + j0 * j0) + F // 2


def gamma(normals):
    """``sin(theta) / (2 - cos(theta))`` per plane wave from the ``3 x M`` unit normals (reference ``:4792``, array azimuth 0)"""
    n = np.asarray(normals, float)
    th = np.arctan2(n[0], n[2])
    return np.sin(th) / (2.0 - np.cos(th))


def _nfft(Nfft, T, N):
    if Nfft is None:
        return T, N
    v = np.atleast_1d(np.asarray(Nfft))
    if v.size not in (1, 2) or not np.all(np.isfinite(v.astype(float))) or np.any(v != np.floor(v)) or np.any(v <= 0):
        raise DasError(f"bfMigration: Nfft must be one or two positive integers, got {Nfft!r}")
    return int(v[0]), int(v[-1])


# ---------------------------------------------------------------------------------------------------------------- device
def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("qups_amd: no HIP device visible -- the migration beamformer has no CPU fallback")
    return torch


def _args(x, tau, gam, Nfft, interp):
    torch = _torch()
    if interp not in _lib.INTERP_FLAGS:
        raise DasError("Interp option not recognized: " + str(interp))
    if not (hasattr(x, "is_cuda") and x.is_cuda):
        raise DasError("migration: x must be a device tensor")
    if x.dtype != torch.complex64:
        raise DasError(f"migration: complex64 data only, got {str(x.dtype).replace('torch.', '')}")
    if x.ndim < 3:
        x = x.reshape(tuple(x.shape) + (1,) * (3 - x.ndim))
    T, N, M = (int(v) for v in x.shape[:3])
    F, K = _nfft(Nfft, T, N)
    tau = np.asarray(tau, np.float64)
    gam = np.asarray(gam, np.float64).reshape(-1)
    if tau.shape != (N, M) or gam.size != M:
        raise DasError(f"migration: tau must be {N} x {M} and gamma hold {M} values, got {tau.shape} and {gam.size}")
    return torch, x, T, N, M, F, K, tau, gam


def takes(F, K):
    """whether ``qdas_migration`` runs these transform lengths in LDS (asked of the library itself: its dedicated return code; needs no device)"""
    d = _lib.MigrationDesc()
    d.T = d.N = d.M = d.frames = 1
    d.F, d.K, d.fs, d.c0, d.pitch, d.flag, d.device = int(F), int(K), 1.0, 1.0, 1.0, 1, -1
    return _lib.lib().qdas_migration(C.byref(d), None, None, None) != _lib.QDAS_ENOTLDS


def migrate(x, t0, fs, tau, gamma, pitch, c0, Nfft=None, fmod=0.0, interp="cubic", jacobian=True, keep_tx=False):
    """``b`` (``min(T,F) x min(N,K) x [M] x frames...``, complex64) from ``x`` (``T x N x M x frames...`` complex64 device tensor): ``qdas_migration``.
    ``tau``: ``N x M`` transmit delays at ``c0``; ``gamma``: ``M`` lateral scalings.  Lengths outside the in-LDS path raise ``QdasError`` with code
    ``QDAS_ENOTLDS`` (``compose`` serves them)."""
    torch, x, T, N, M, F, K, tau, gam = _args(x, tau, gamma, Nfft, interp)
    dev = x.device
    Fsz = tuple(int(v) for v in x.shape[3:])
    frames = int(np.prod(Fsz)) if Fsz else 1
    xc = x.permute(*reversed(range(x.ndim))).contiguous()      # memory: time fastest, then n, m, frames
    Tn, Nn = min(T, F), min(N, K)
    shape = Fsz[::-1] + ((M,) if keep_tx else ()) + (Nn, Tn)
    b = torch.empty(shape, dtype=torch.complex64, device=dev)
    tau_t = torch.from_numpy(np.ascontiguousarray(tau.T)).to(dev)
    gam_t = torch.from_numpy(np.ascontiguousarray(gam)).to(dev)
    d = _lib.MigrationDesc()
    d.T, d.N, d.M, d.frames, d.F, d.K = T, N, M, frames, F, K
    d.fs, d.fmod, d.t0, d.c0, d.pitch = float(fs), float(fmod), float(t0), float(c0), float(pitch)
    d.flag, d.keep_tx, d.jacobian = _lib.INTERP_FLAGS[interp], int(bool(keep_tx)), int(bool(jacobian))
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.tau, d.gamma = C.c_void_p(tau_t.data_ptr()), C.c_void_p(gam_t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_migration(C.byref(d), C.c_void_p(xc.data_ptr()), C.c_void_p(b.data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return b.permute(*reversed(range(b.ndim)))


def compose(x, t0, fs, tau, gamma, pitch, c0, Nfft=None, fmod=0.0, interp="cubic", jacobian=True, keep_tx=False, bsize=None):
    """the same contract from ``torch.fft`` and ``qups_amd.wsinterpd`` (fp32 sample indices, as that entry takes them), in transmit blocks of ``bsize``"""
    from .interpd import wsinterpd
    torch, x, T, N, M, F, K, tau, gam = _args(x, tau, gamma, Nfft, interp)
    dev = x.device
    Fsz = tuple(int(v) for v in x.shape[3:])
    x = x.reshape(T, N, M, -1)
    Tn, Nn = min(T, F), min(N, K)
    if bsize is None:
        bsize = max(1, (1 << 27) // (F * K * x.shape[3]))       # 1 GiB of complex64 per block
    f, kx = axes(F, K, fs, pitch)
    cs = c0 / math.sqrt(2.0)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ph = lambda turns: torch.polar(torch.ones_like(turns), 2.0 * math.pi * (turns - torch.round(turns))).to(torch.complex64)
    ft, kxt = td(f).reshape(F, 1, 1, 1), td(kx).reshape(1, K, 1, 1)
    kkz = td(stolt_indices(F, K, fs, pitch, c0)).reshape(F, K, 1, 1)
    if jacobian:
        fkz = cs * np.sign(f)[:, None] * np.sqrt(kx[None, :] ** 2 + f[:, None] ** 2 / cs ** 2)
        jac = td(((f[:, None] / cs) / (fkz + np.finfo(float).eps)).astype(np.float32)).reshape(F, K, 1, 1)
    z = td(c0 / 2.0 * (t0 + np.arange(F) / fs)).reshape(F, 1, 1, 1)
    up = ph(fmod * td(t0 + np.arange(T) / fs)).reshape(T, 1, 1, 1) if fmod else None
    out = [] if keep_tx else 0
    for m0 in range(0, M, bsize):
        xb = x[:, :, m0:m0 + bsize]
        if up is not None:
            xb = xb * up
        X = torch.fft.fftshift(torch.fft.fft(xb, n=F, dim=0), dim=0)
        X = X * ph(-ft * (t0 + td(tau[:, m0:m0 + bsize]).reshape(1, N, -1, 1)))
        X = torch.fft.fftshift(torch.fft.fft(X, n=K, dim=1), dim=1)
        y = wsinterpd(X, kkz, 1, 1, None, interp, 0.0)
        if jacobian:
            y = y * jac
        y = y * ph(ft * t0)
        b = torch.fft.ifft(torch.fft.ifftshift(y, dim=0), dim=0)
        b = b * ph(kxt * td(gam[m0:m0 + bsize]).reshape(1, 1, -1, 1) * z)
        b = torch.fft.ifft(torch.fft.ifftshift(b, dim=1), dim=1)[:Tn, :Nn]
        if keep_tx:
            out.append(b)
        else:
            out = out + b.sum(dim=2)
    b = torch.cat(out, dim=2) if keep_tx else out
    return b.reshape((Tn, Nn) + ((M,) if keep_tx else ()) + Fsz)


def bmode(x, t0, fs, tau, gamma, pitch, c0, Nfft=None, fmod=0.0, interp="cubic", jacobian=True, keep_tx=False, bsize=None):
    """``migrate`` where the kernels take the transform lengths, ``compose`` elsewhere: the routing of ``UltrasoundSystem.bfMigration``"""
    T, N = int(x.shape[0]), int(x.shape[1]) if x.ndim > 1 else 1
    if takes(*_nfft(Nfft, T, N)):
        return migrate(x, t0, fs, tau, gamma, pitch, c0, Nfft, fmod, interp, jacobian, keep_tx)
    return compose(x, t0, fs, tau, gamma, pitch, c0, Nfft, fmod, interp, jacobian, keep_tx, bsize)
