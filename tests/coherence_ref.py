"""Float64 numpy restatement of the MATLAB branches of the reference's kern/slsc.m, kern/dmas.m, kern/cohfac.m and kern/pcf.m (TEST
INFRASTRUCTURE; never imported by qups_amd).  Dimensions are 0-based here; the reduced axes stay as singletons."""
from __future__ import annotations

import numpy as np


def _take(x, i, axis):
    return np.take(x, [i], axis=axis)


def _lags(L, N, scalar_means_range=True):
    L = np.atleast_1d(np.asarray(L)).ravel()
    return np.arange(1, int(L[0]) + 1) if L.size == 1 and scalar_means_range else L.astype(np.int64)


def slsc(x, axis, L=None, method="average", kaxis=None):
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    x = x.astype(np.complex128 if cplx else np.float64)
    shp = list(x.shape)
    if kaxis is None:
        kaxis = x.ndim
    while kaxis >= x.ndim:
        x = x[..., None]
    A = x.shape[axis]
    if L is None:
        L = max(1, A // 4)
    lags = _lags(L, A)
    M, Nn = np.meshgrid(np.arange(A), np.arange(A), indexing="ij")
    H = np.abs(M - Nn)
    S = np.isin(H, lags)
    nL = lags.size
    with np.errstate(invalid="ignore", divide="ignore"):
        if method == "average":
            nrm = np.sqrt(np.sum(np.abs(x) ** 2, axis=kaxis, keepdims=True))
            xh = x / nrm
            xh[np.isnan(xh)] = 0
            W = S / (A - H) / 2 / nL
            z = 0
            for i in range(A):
                w = W[i].reshape([-1 if d == axis else 1 for d in range(x.ndim)])
                t = w * np.conj(_take(xh, i, axis)) * xh
                z = z + np.nansum(t, axis=(axis, kaxis), keepdims=True)
        else:
            mn = np.nanmean(np.sqrt(np.sum(np.abs(x) ** 2, axis=axis, keepdims=True)))
            x = x * 2.0 ** np.ceil(np.log2(1 / mn)) if np.isfinite(1 / mn) and mn > 0 else x * np.inf
            z = a = b = 0
            for i in range(A):
                w = S[i].reshape([-1 if d == axis else 1 for d in range(x.ndim)])
                xc = _take(x, i, axis)
                z = z + np.nansum(w * np.conj(xc) * x, axis=(axis, kaxis), keepdims=True)
                a = a + np.nansum(w * np.conj(x) * x, axis=(axis, kaxis), keepdims=True)
                b = b + np.nansum(w * np.conj(xc) * xc, axis=(axis, kaxis), keepdims=True)
            a, b = np.real(a), np.real(b)                   # (MATLAB drops their all-zero imaginary parts: rsqrt(0) = Inf, and 0 * Inf = NaN)
            f = (1 / np.sqrt(a)) * (1 / np.sqrt(b))
            f[np.isnan(f)] = 0
            z = z * f
    shp[axis] = 1
    if kaxis < len(shp):
        shp[kaxis] = 1
    z = np.asarray(z).reshape(shp)
    return z if cplx else z.real


def dmas(x, axis, L=None):
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    x = x.astype(np.complex128 if cplx else np.float64)
    N = x.shape[axis]
    if L is None:
        lags = np.arange(1, N)
    elif np.asarray(L).size == 1:
        lags = np.arange(1, int(np.asarray(L).ravel()[0]) + 1)
    else:
        lags = np.intersect1d(np.arange(1, N), np.asarray(L))
    shp = list(x.shape)
    shp[axis] = 1
    b = np.zeros(shp, x.dtype)
    for i in lags:
        if i >= N:
            continue
        b = b + np.sum(np.take(x, np.arange(0, N - i), axis) * np.take(x, np.arange(i, N), axis), axis=axis, keepdims=True)
    return b


def dmas_compress(b):
    """exp(i angle(b)) sqrt(|b|) (real input: sign(b) sqrt(|b|))"""
    if np.iscomplexobj(b):
        return np.exp(1j * np.angle(b)) * np.sqrt(np.abs(b))
    return np.sign(b) * np.sqrt(np.abs(b))


def dmas_pairs_abs(x, axis):
    """sum over the pairs n < m of |x_n| |x_m| (the accuracy scale of DMAS)"""
    a = np.abs(np.asarray(x, np.complex128))
    s = np.sum(a, axis=axis, keepdims=True)
    return (s * s - np.sum(a * a, axis=axis, keepdims=True)) / 2


def cohfac(b, axes):
    b = np.asarray(b)
    b = b.astype(np.complex128 if np.iscomplexobj(b) else np.float64)
    axes = tuple(np.atleast_1d(axes))
    n = np.prod([b.shape[a] for a in axes])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(np.sum(b, axis=axes, keepdims=True)) ** 2 / np.sum(np.abs(b) ** 2, axis=axes, keepdims=True) / n


def pcf(b, axis, gamma=1.0):
    b = np.asarray(b)
    if not np.iscomplexobj(b):
        raise ValueError("Input must be complex.")
    b = b.astype(np.complex128)
    phi = np.angle(b)
    phi[np.isnan(b)] = np.nan

    def pstd(p):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.nanmean(p, axis=axis, keepdims=True)
            return np.sqrt(np.nanmean((p - m) ** 2, axis=axis, keepdims=True))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        s0 = pstd(phi)
        sa = pstd(phi - np.pi * np.sign(phi))
    sf = np.fmin(s0, sa)
    w = 1 - (gamma / np.sqrt(np.pi / 3)) * sf
    w = np.where(np.isnan(w), 0.0, np.maximum(0.0, w))
    return w, sf
