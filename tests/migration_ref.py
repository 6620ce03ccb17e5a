"""Float64 numpy restatement of plane-wave Stolt f-k migration (what ``UltrasoundSystem.bfMigration`` computes; reference
``src/UltrasoundSystem.m:4675-4887``), steps 1-10:

    1. x *= e^{2 pi i fmod (t0 + t/fs)};  X = fftshift(fft(x, F))                     f  = ((0:F-1) - floor(F/2)) / F fs
    2. X *= e^{-2 pi i f (t0 + tau[n,m])}
    3. X  = fftshift(fft(X, K) along n)                                                kx = ((0:K-1) - floor(K/2)) / K / pitch
    4. y[j,k] = wsinterpd(X[:,k], kkz[j,k]) (extrapolation value 0)                    kkz = sign(j0) sqrt(a^2 + j0^2) + floor(F/2)
    5. y *= (f / cs) / (fkz + eps)                                                     fkz = cs sign(f) sqrt(kx^2 + f^2/cs^2), cs = c0 / sqrt 2
    6. y *= e^{+2 pi i f t0};  b = ifft(ifftshift(y))
    7. b *= e^{2 pi i kx gamma_m z},  z = c0/2 (t0 + (0:F-1)/fs)
    8. b = ifft(ifftshift(b) along kx);  9. crop to min(T,F) x min(N,K);  10. sum over m unless keep_tx

The sampling is ``oracle.das_oracle.wsinterpd``; the delays ``oracle.das_oracle.sequence_delays``.  No package code is used."""
import numpy as np

from oracle import das_oracle as O


def axes(F, K, fs, pitch):
    return (np.arange(F) - F // 2) / F * fs, (np.arange(K) - K // 2) / K / pitch


def stolt_indices(F, K, fs, pitch, c0):
    """the index form of DESIGN.md 4.8: j0 = j - floor(F/2), a = kx cs F / fs"""
    j0 = (np.arange(F) - F // 2).astype(np.float64)[:, None]
    a = (axes(F, K, fs, pitch)[1] * (c0 / np.sqrt(2.0)) * F / fs)[None, :]
    return np.sign(j0) * np.sqrt(a * a + j0 * j0) + F // 2


def stolt_indices_reference(F, K, fs, pitch, c0):
    """the reference's own expression (:4821-4822): (fkz - f(1)) F / fs"""
    f, kx = axes(F, K, fs, pitch)
    cs = c0 / np.sqrt(2.0)
    fkz = cs * np.sign(f)[:, None] * np.sqrt(kx[None, :] ** 2 + f[:, None] ** 2 / cs ** 2)
    return (fkz - f[0]) * F / fs


def gamma(angles_deg):
    th = np.deg2rad(np.asarray(angles_deg, float))
    return np.sin(th) / (2.0 - np.cos(th))


def pw_normals(angles_deg):
    th = np.deg2rad(np.asarray(angles_deg, float))
    return np.stack([np.sin(th), 0 * th, np.cos(th)])


def pw_delays(elem_pos, angles_deg, c0):
    return O.sequence_delays("PW", elem_pos, pw_normals(angles_deg), c0)


def spectrum(x, t0, fs, tau, Nfft=None, fmod=0.0):
    """steps 1-3: F x K x M x frames (complex128)"""
    x = np.asarray(x).astype(np.complex128)
    x = x.reshape(x.shape + (1,) * (4 - x.ndim)) if x.ndim < 4 else x.reshape(x.shape[:3] + (-1,))
    T, N = x.shape[:2]
    F, K = (T, N) if Nfft is None else (int(Nfft[0]), int(Nfft[-1]))
    f, _ = axes(F, K, fs, 1.0)
    t = (t0 + np.arange(T) / fs).reshape(T, 1, 1, 1)
    X = np.fft.fftshift(np.fft.fft(x * np.exp(2j * np.pi * fmod * t), n=F, axis=0), axes=0)
    X = X * np.exp(-2j * np.pi * f.reshape(F, 1, 1, 1) * t0) * np.exp(-2j * np.pi * f.reshape(F, 1, 1, 1) * np.asarray(tau, float)[None, :, :, None])
    return np.fft.fftshift(np.fft.fft(X, n=K, axis=1), axes=1)


def resample(X, fs, pitch, c0, interp="cubic", jacobian=True):
    """steps 4-5"""
    F, K = X.shape[:2]
    f, kx = axes(F, K, fs, pitch)
    cs = c0 / np.sqrt(2.0)
    kkz = stolt_indices(F, K, fs, pitch, c0)
    y = O.wsinterpd(X, kkz.reshape(F, K, 1, 1), 1, 1, None, interp, 0.0)
    if jacobian:
        fkz = cs * np.sign(f)[:, None] * np.sqrt(kx[None, :] ** 2 + f[:, None] ** 2 / cs ** 2)
        y = (y * (f / cs).reshape(F, 1, 1, 1)) / (fkz + np.finfo(float).eps).reshape(F, K, 1, 1)
    return y


def migrate(x, t0, fs, tau, gam, pitch, c0, Nfft=None, fmod=0.0, interp="cubic", jacobian=True, keep_tx=False):
    """b: min(T,F) x min(N,K) x [M] x frames... (complex128)"""
    x = np.asarray(x)
    x = x.reshape(x.shape + (1,) * (3 - x.ndim)) if x.ndim < 3 else x
    T, N, M = x.shape[:3]
    Fsz = x.shape[3:]
    X = spectrum(x, t0, fs, tau, Nfft, fmod)
    F, K = X.shape[:2]
    f, kx = axes(F, K, fs, pitch)
    y = resample(X, fs, pitch, c0, interp, jacobian) * np.exp(2j * np.pi * f * t0).reshape(F, 1, 1, 1)
    b = np.fft.ifft(np.fft.ifftshift(y, axes=0), axis=0)
    z = c0 / 2.0 * (t0 + np.arange(F) / fs)
    b = b * np.exp(2j * np.pi * kx.reshape(1, K, 1, 1) * np.asarray(gam, float).reshape(1, 1, M, 1) * z.reshape(F, 1, 1, 1))
    b = np.fft.ifft(np.fft.ifftshift(b, axes=1), axis=1)[:min(T, F), :min(N, K)]
    if not keep_tx:
        b = b.sum(axis=2)
    return b.reshape(b.shape[:(3 if keep_tx else 2)] + tuple(Fsz))


def bscan_axes(T, N, F, K, t0, fs, c0, pitch, x0, offset_z=0.0):
    """(x, z) of the output scan: the reference's regularised axes (:4842-4843, :4861-4870)"""
    Tn, Nn = min(T, F), min(N, K)
    z = offset_z + (c0 / 2.0 * (t0 + np.arange(F) / fs))[:Tn]
    return x0 + pitch * np.arange(Nn), z[0] + (np.mean(np.diff(z)) if Tn > 1 else 0.0) * np.arange(Tn)


def discontinuity_margin(F, K, fs, pitch, c0, interp):
    """smallest distance [samples] of any kkz -- the exact kx = 0 column and f = 0 row left out -- from a discontinuity of the interpolator:
    the support edges (where the first or the last tap crosses 0 or F - 1, and kkz = 0), plus every half-integer for 'nearest'"""
    kkz = stolt_indices(F, K, fs, pitch, c0)
    keep = np.ones((F, K), bool)
    keep[:, K // 2] = False
    keep[F // 2, :] = False
    v = kkz[keep]
    if interp == "nearest":
        return float(np.abs(v + 0.5 - np.round(v + 0.5)).min())           # half-integers (among them the edges -1/2 and F - 1/2)
    lo, hi = (0, 1) if interp == "linear" else (1, 2)                    # taps floor - lo .. floor + hi: in support iff lo <= kkz < F - hi
    return float(min(np.abs(v - lo).min(), np.abs(v - (F - hi)).min(), np.abs(v).min()))


def gaussian_echoes(T, elem_pos, angles_deg, scat, t0, fs, c0, fc=5e6, sigma=0.2e-6):
    """analytic Gaussian-pulse echoes of one scatterer under plane waves: T x N x M complex128"""
    p = np.asarray(elem_pos, float)
    sc = np.asarray(scat, float)
    nv = pw_normals(angles_deg)
    d = (nv * sc[:, None]).sum(0)[None, None, :] / c0 + (np.linalg.norm(p - sc[:, None], axis=0) / c0)[None, :, None]
    t = (t0 + np.arange(T) / fs)[:, None, None]
    return np.exp(-0.5 * ((t - d) / sigma) ** 2) * np.exp(2j * np.pi * fc * (t - d))
