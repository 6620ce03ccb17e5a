"""Float64 numpy restatement of the frequency-domain adjoint beamformer (what ``UltrasoundSystem.bfAdjoint`` computes): the spectrum with its
phase ramps, the frequency selection, the routing of the apodization classes, and the loop over frequencies with one matrix product per side.

    X[k,n,v] = FFT_K(x[t,n,v] e^{+2 pi i fmod (t0_v + t/fs)})[k] e^{-2 pi i f_k t0_v} e^{+2 pi i f_k t0off_v},      f_k = k fs / K
    S[m,v]   = apod_tx[m,v] e^{-2 pi i f_k tau_foc[m,v]}                    tau_foc = del_tx + t0off
    A[i,v]   = sum_m e^{-2 pi i f_k tau_tx(i,m)} S[m,v],    Ahat = A / ||A[i,:]||_2
    R[i,v]   = sum_n a_n(i,n) e^{+2 pi i f_k tau_rx(i,n)} a_mn(n,v) X[k,n,v]
    b[i]     = sum_k sum_v a_m(i,v) R[i,v] conj(Ahat[i,v])

Everything is an array argument: no package code is used, so the oracle shares nothing with what it checks."""
import numpy as np


def t0_offset(seq_type, focus, c0):
    """one value per transmit: 0 for FSA / PW, -|focus| / c0 for FC / VS, +|focus| / c0 for DV"""
    if seq_type in ("FSA", "PW"):
        return np.zeros(1)
    r = np.linalg.norm(np.asarray(focus, float), axis=0) / c0
    return {"FC": -r, "VS": -r, "DV": r}[seq_type]


def spectrum(x, t0, fs, fmod=0.0, K=None, t0off=0.0):
    """K x N x V (x frames) complex128"""
    x = np.asarray(x).astype(np.complex128)
    T, V = x.shape[0], x.shape[2]
    K = T if K is None else K
    assert K >= T
    tail = (1,) * (x.ndim - 3)
    t0 = np.broadcast_to(np.asarray(t0, float).reshape(-1), (V,)).reshape((1, 1, V) + tail)
    off = np.broadcast_to(np.asarray(t0off, float).reshape(-1), (V,)).reshape((1, 1, V) + tail)
    t = np.arange(T).reshape((T, 1, 1) + tail) / fs
    X = np.fft.fft(x * np.exp(2j * np.pi * fmod * (t0 + t)), n=K, axis=0)
    f = (np.arange(K) * (fs / K)).reshape((K, 1, 1) + tail)
    return X * np.exp(-2j * np.pi * f * t0) * np.exp(2j * np.pi * f * off)


def select_bins(X, fs, fthresh=-np.inf):
    """ascending 0-based bins: below fs / 2 and, with a finite threshold, some trace within fthresh dB of its own maximum there"""
    K = X.shape[0]
    keep = np.arange(K) * (fs / K) < fs / 2
    if fthresh > -np.inf:
        mag = np.abs(X).reshape(K, -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            db = 20 * np.log10(mag) - 20 * np.log10(mag.max(axis=0, keepdims=True))
        keep &= (db >= fthresh).any(axis=1)
    return np.flatnonzero(keep)


def delays(P, Pi, cinv):
    """I x n travel times |P_n - Pi| cinv(i)"""
    d = np.linalg.norm(np.asarray(Pi, float)[:, :, None] - np.asarray(P, float)[:, None, :], axis=0)
    return d * np.asarray(cinv, float).reshape(-1, 1)


def transmit_field(f, tau_tx, tau_foc, apod_tx):
    """A: I x V at frequency f"""
    return np.exp(-2j * np.pi * f * tau_tx) @ (apod_tx * np.exp(-2j * np.pi * f * tau_foc))


def adjoint(X, bins, fs, Pi, Pr, Pt, cinv, tau_foc, apod_tx, a_n=None, a_m=None, a_mn=None, keep_tx=False, keep_rx=False):
    """b: I x [N] x [V] (kept dimensions only) from the spectrum X (K x N x V) over the bins `bins`"""
    K, N, V = X.shape
    I = np.asarray(Pi).shape[1]
    tau_rx, tau_tx = delays(Pr, Pi, cinv), delays(Pt, Pi, cinv)
    a_n = np.ones((I, N)) if a_n is None else np.asarray(a_n, float)
    a_m = np.ones((I, V)) if a_m is None else np.asarray(a_m, float)
    a_mn = np.ones((N, V)) if a_mn is None else np.asarray(a_mn, float)
    b = np.zeros((I,) + ((N,) if keep_rx else ()) + ((V,) if keep_tx else ()), np.complex128)
    for k in bins:
        f = k * (fs / K)
        A = transmit_field(f, tau_tx, tau_foc, apod_tx)
        Ah = A / np.linalg.norm(A, axis=1, keepdims=True)
        G = a_n * np.exp(2j * np.pi * f * tau_rx)                                # I x N
        Xk = a_mn * X[k]                                                        # N x V
        if keep_rx:
            y = (a_m * np.conj(Ah))[:, None, :] * G[:, :, None] * Xk[None]      # I x N x V
        else:
            y = a_m * (G @ Xk) * np.conj(Ah)                                    # I x V
        b += y if keep_tx else y.sum(-1)
    return b
