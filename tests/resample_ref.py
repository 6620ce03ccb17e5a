"""The float64 restatement of qdas_resample (TEST INFRASTRUCTURE), straight from the formula of include/qdas.h:

    out[j] = sum_i h[off + j q - i p] X[i],  0 <= off + j q - i p < K      <=>      for j: n = off + j*q; for k in range(n % p, K, p): y[j] += h[k] * X((n - k) // p)

with ``X = x`` inside the record, zeros (``edge='zero'``) or the odd reflection (``edge='odd'``) outside; and the four functions it gives."""
import numpy as np


def extended(x, i, edge):
    """``X[i]`` for a record ``x`` (``T x ...``)"""
    T = x.shape[0]
    if 0 <= i < T:
        return x[i]
    if edge == "odd":
        if -(T - 1) <= i < 0:
            return 2 * x[0] - x[-i]
        if T - 1 < i <= 2 * (T - 1):
            return 2 * x[T - 1] - x[2 * (T - 1) - i]
        raise IndexError(f"index {i} is beyond the odd reflection's reach for T = {T}")
    return np.zeros_like(x[0])


def polyphase(h, x, p, q, off, J, edge="zero"):
    h = np.asarray(h, np.float64)
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    K = h.size
    y = np.zeros((J,) + x.shape[1:], x.dtype)
    for j in range(J):
        n = off + j * q
        for k in range(n % p, K, p):
            y[j] += h[k] * extended(x, (n - k) // p, edge)
    return y


def polyphase_fast(h, x, p, q, off, J, edge="zero"):
    """the same sum, one numpy statement per tap instead of one per term (tests/test_resample_host.py holds it to :func:`polyphase`): tap k meets the outputs
    j with (off + j q - k) mod p = 0"""
    h = np.asarray(h, np.float64)
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    T = x.shape[0]
    y = np.zeros((J,) + x.shape[1:], x.dtype)
    n = off + np.arange(J) * q
    for k in range(h.size):
        hit = np.nonzero((n - k) % p == 0)[0]
        i = (n[hit] - k) // p
        ins = (i >= 0) & (i < T)
        y[hit[ins]] += h[k] * x[i[ins]]
        if edge == "odd" and not ins.all():
            lo, hi = i < 0, i >= T
            if (i[lo] < -(T - 1)).any() or (i[hi] > 2 * (T - 1)).any():
                raise IndexError("beyond the odd reflection's reach")
            y[hit[lo]] += h[k] * (2 * x[0] - x[-i[lo]])
            y[hit[hi]] += h[k] * (2 * x[T - 1] - x[2 * (T - 1) - i[hi]])
    return y


def upfirdn_len(T, K, p, q):
    return -(-((T - 1) * p + K) // q)


def resample_len(T, p, q):
    return -(-T * p // q)


def upfirdn(h, x, p, q):
    return polyphase(h, x, p, q, 0, upfirdn_len(np.shape(x)[0], np.size(h), p, q))


def resample(x, p, q, h):
    K = np.size(h)
    assert K % 2 == 1
    return polyphase(h, x, p, q, (K - 1) // 2, resample_len(np.shape(x)[0], p, q))


def filtfilt(b, x):
    b = np.asarray(b, np.float64)
    return polyphase(np.convolve(b, b[::-1]), x, 1, 1, b.size - 1, np.shape(x)[0], "odd")


def taps_closed_form(p, q, n=10, beta=5.0):
    """``sinc((k - (L-1)/2) / max(p, q)) kaiser(L, beta)[k]``, scaled to the sum ``p``"""
    pq = max(p, q)
    L = 2 * n * pq + 1
    g = np.sinc((np.arange(L) - (L - 1) / 2) / pq) * np.kaiser(L, beta)
    return p * g / g.sum()


def reads(i, K, p, q, off, J):
    """the outputs ``j`` with ``0 <= off + j q - i p < K``: where a NaN at ``x[i]`` arrives"""
    j = np.arange(J)
    k = off + j * q - i * p
    return j[(k >= 0) & (k < K)]


def bound(h, p, xmax, double=False, odd=False):
    """per element (real and imaginary part separately): ``(M + 4) eps S X``, ``M = ceil(K / p)``, ``S = max_phi sum_m |h[phi + m p]|``, ``X = max|x|`` (three
    times that with the odd edge): M products and sums of one rounding each, the tap's rounding to the compute precision, the two roundings of the reflected
    sample, one more for slack"""
    h = np.asarray(h, np.float64)
    K = h.size
    M = -(-K // p)
    S = max(np.abs(h[phi::p]).sum() for phi in range(min(p, K)))
    eps = 2.0 ** -53 if double else 2.0 ** -24
    return (M + 4) * eps * S * (3.0 if odd else 1.0) * xmax
