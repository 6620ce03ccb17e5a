"""The restatement the demodulator is tested against (a helper module, not a test): numpy float64, written from the three reference methods it fuses --
``downmix`` (``src/ChannelData.m:757-807``: ``data .* exp(-2i*pi*fc*time)``, ``time = t0 + (0:T-1)' / fs``), ``filter`` (``:857-888``: MATLAB's causal
``filter(D, x)`` along time, then ``t0 -= filtord / 2 / fs``) and ``downsample`` (``:1042-1058``: every ``ratio``-th sample from the first, ``fs / ratio``).

``x`` is ``T x ...`` (time first); ``t0`` a scalar or an array that broadcasts against ``x`` with a leading 1 (one start time per transmit)."""
import numpy as np


def frac(v):
    return v - np.floor(v)


def downmix(x, fc, fs, t0):
    x = np.asarray(x)
    T = x.shape[0]
    n = np.arange(T, dtype=np.float64).reshape((T,) + (1,) * (x.ndim - 1))
    cyc = fc * (np.asarray(t0, np.float64) + n / fs)
    return x.astype(np.complex128) * np.exp(-2j * np.pi * frac(cyc))


def causal_filter(x, b):
    """``y[t] = sum_k b[k] x[t - k]``, terms before the record omitted"""
    x = np.asarray(x)
    b = np.asarray(b, np.float64).reshape(-1)
    y = np.zeros(x.shape, np.result_type(x.dtype, np.float64))
    T = x.shape[0]
    for k, bk in enumerate(b[:T]):
        y[k:] += bk * x[:T - k]
    return y


def downsample(x, ratio):
    return np.asarray(x)[::ratio]


def demod(x, fc, fs, t0, b, ratio):
    """the composition, float64: ``ceil(T / ratio) x ...`` complex128"""
    return downsample(causal_filter(downmix(x, fc, fs, t0), b), ratio)


def demod_loops(x, fc, fs, t0, b, ratio):
    """the contract of include/qdas.h as a direct triple loop over (trace, output, tap); ``x`` is ``T x C``, ``t0`` a scalar or ``C`` values"""
    x = np.asarray(x)
    T, C = x.shape
    K, J = len(b), -(-T // ratio)
    t0 = np.broadcast_to(np.asarray(t0, np.float64).reshape(-1), (C,))
    out = np.zeros((J, C), np.complex128)
    for c in range(C):
        for j in range(J):
            s = 0j
            for k in range(K):
                i = j * ratio - k
                if i < 0:
                    continue
                cyc = fc * (t0[c] + i / fs)
                s += b[k] * x[i, c] * np.exp(-2j * np.pi * (cyc - np.floor(cyc)))
            out[j, c] = s
    return out


def time_axis(t0, fs, K, ratio):
    """``(t0', fs')`` of the result"""
    return np.asarray(t0, np.float64) - (K - 1) / 2.0 / fs, fs / ratio


def bound(K, b, xmax, fct_max, double=False):
    """the per-element bound of the issue: ``((K + 8) eps + 8 pi eps64 max|fc t|) sum|b| max|x|``, eps = 2^-24 (2^-53 for double data)"""
    eps = 2.0 ** -53 if double else 2.0 ** -24
    return ((K + 8) * eps + 8 * np.pi * 2.0 ** -53 * fct_max) * float(np.sum(np.abs(b))) * float(xmax)


def nan_reach(i, K, ratio, J):
    """outputs a NaN at ``x[i]`` reaches: ``0 <= j R - i < K``"""
    return [j for j in range(J) if 0 <= j * ratio - i < K]
