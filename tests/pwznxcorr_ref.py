"""Float64 numpy restatement of the reference's kern/pwznxcorr.m, base-MATLAB branch (iflt = false): ``convn(., w, 'same')``, a manual zero
pad of ``ceil(max|lags|)`` samples at the end of the time dimension, ``circshift`` per lag.  Written from the reference's code, line by line:

* ``conv_same`` is MATLAB's ``'same'``: the central part of the full convolution starting at offset ``floor(W/2)`` (numpy / scipy start
  at ``(W-1)//2``, which differs for even W).
* ``core`` is kern/pwznxcorr.m:241-299 for integer lags, U = 1, multi = false.
* ``pwznxcorr`` is the argument handling in front of it (:162-229): lag expansion, the window, the pad, the choice of the right traces.
"""
from __future__ import annotations

import numpy as np


def conv_same(a, w):
    """``convn(a, w(:), 'same')`` along axis 0: out[s] = sum_k w[k] a[s + floor(W/2) - k], a = 0 outside."""
    a = np.asarray(a)
    w = np.asarray(w, dtype=np.float64).ravel()
    W, n = w.size, a.shape[0]
    h = W // 2
    if n == 0:
        return np.zeros(a.shape, dtype=np.result_type(a.dtype, np.float64))
    # a between W - 1 - h zeros in front and h behind: window s holds a[s + h - (W - 1)] .. a[s + h], i.e. the taps k = W - 1 .. 0
    ap = np.concatenate([np.zeros((W - 1 - h,) + a.shape[1:], a.dtype), a, np.zeros((h,) + a.shape[1:], a.dtype)], 0)
    win = np.lib.stride_tricks.sliding_window_view(ap, W, axis=0)        # n x ... x W
    return win @ w[::-1]


def core(xl, xr, w, lags, zero=True, norm=True, pad=True):
    """xl: T x N x ..., xr: T x (N | 1) x ... (broadcast against xl), time first.  Returns T x N x ... x L (lag last)."""
    xl = np.asarray(xl, dtype=np.complex128 if np.iscomplexobj(xl) else np.float64)
    xr = np.asarray(xr, dtype=np.complex128 if np.iscomplexobj(xr) else np.float64)
    lags = [int(l) for l in lags]
    T = xl.shape[0]
    P = max([abs(l) for l in lags], default=0) if pad else 0
    if P:                                                    # x = cat(tdim, x, zeros(P, ...))  (:195-204)
        xl = np.concatenate([xl, np.zeros((P,) + xl.shape[1:], xl.dtype)], 0)
        xr = np.concatenate([xr, np.zeros((P,) + xr.shape[1:], xr.dtype)], 0)
    K = lambda a: conv_same(a, w)                            # kernfun
    xlz = xl - K(xl) if zero else xl                         # :242
    if norm:
        xln = K((xlz * np.conj(xlz)).real)                   # :243
    out = []
    for l in lags:
        c = np.conj(np.roll(xr, -l, axis=0))                 # conj(circshift(xr, -l, tdim))  (:189, :253)
        cz = c - K(c) if zero else c                         # :260
        y = K(xlz * cz)                                      # :268
        if norm:
            xrn = K((cz * np.conj(cz)).real)                 # :274
            with np.errstate(invalid="ignore", divide="ignore"):
                y = y / (np.sqrt(xln) * np.sqrt(xrn))        # :280-284 (Wn = 1)
        out.append(y[:T])                                    # :299
    if not out:
        return np.zeros(np.broadcast_shapes(xl[:T].shape, xr[:T].shape) + (0,), xl.dtype)
    return np.stack(out, axis=-1)


def expand_lags(lags):
    a = np.atleast_1d(np.asarray(lags, dtype=np.float64)).ravel()
    if a.size == 1:
        return list(range(-int(a[0]), int(a[0]) + 1))        # isscalar: -L:L (empty for L < 0)
    return [int(v) for v in a]


def window(W, lags):
    if W is None:
        m = max([abs(l) for l in lags], default=0)
        W = max(-(-m // 2), 1)                               # max(ceil(max|lags| / 2), 1)
    if np.ndim(W) == 0:
        return np.ones(int(W))
    return np.asarray(W, dtype=np.float64).ravel()


def pwznxcorr(x, lags, W=None, *, pad=True, zero=True, norm=True, ref="neighbor", stride=1, x0=None, tdim=1, ndim=2, ldim=None):
    """The reference's call, 1-based dimensions.  The result has x's shape with the channel dimension N - stride (neighbor) or N, and the
    lags along ``ldim`` (default ``x.ndim + 1``; a dimension of x named by ``ldim`` must have size 1)."""
    x = np.asarray(x)
    lags = expand_lags(lags)
    w = window(W, lags)
    D = max(x.ndim, tdim, ndim)
    x = x.reshape(x.shape + (1,) * (D - x.ndim))
    t, n = tdim - 1, ndim - 1
    rest = [d for d in range(D) if d not in (t, n)]
    xm = np.transpose(x, [t, n] + rest)                      # T x N x rest
    N = xm.shape[1]
    if ref == "neighbor":
        xl, xr = xm[:, :max(N - stride, 0)], xm[:, stride:]
    elif ref == "center":
        mid = (N + 1) / 2                                    # (N + 1 - C + 1) / 2 + (0 : C - 1) with C = 1, 1-based
        idx = sorted({int(np.floor(mid)) - 1, int(np.ceil(mid)) - 1})
        xl, xr = xm, xm[:, idx].mean(axis=1, keepdims=True)
    elif ref == "x0":
        x0 = np.asarray(x0)
        x0 = x0.reshape(x0.shape + (1,) * (D - x0.ndim))
        xl, xr = xm, np.transpose(x0, [t, n] + rest)
    else:
        raise ValueError(ref)
    y = core(xl, xr, w, lags, zero, norm, pad)               # T x Nout x rest x L
    if not (np.iscomplexobj(xl) or np.iscomplexobj(xr)):
        y = y.real
    # back to x's dimension order, the lag dimension at ldim
    inv = np.argsort([t, n] + rest)
    y = np.transpose(y, list(inv) + [D])                     # x's order, lag last (dimension D + 1)
    ldim = D + 1 if ldim is None else ldim
    if ldim <= D:
        assert y.shape[ldim - 1] == 1, "ldim must name a singleton dimension of x"
        y = np.moveaxis(y, D, ldim - 1)                      # L lands at ldim, the singleton moves behind it ...
        y = y.reshape(y.shape[:ldim] + y.shape[ldim + 1:])   # ... and is dropped
    else:
        y = y.reshape(y.shape[:D] + (1,) * (ldim - D - 1) + (y.shape[D],))
    return y
