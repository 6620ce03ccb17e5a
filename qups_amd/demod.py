"""Demodulation on the device: the reference's recipe for baseband imaging, ``downmix(chd, fc)`` -> ``filter(chd, D)`` -> ``downsample(chd, ratio)``
(``src/ChannelData.m:757-807``, ``:857-888``, ``:1042-1058``), as ONE pass over the record on ``csrc/demod.hip``.  ``include/qdas.h`` states the contract:

    out[j, ...] = sum_k b[k] x[j R - k, ...] exp(-2j pi fc (t0 + (j R - k) / fs)),    j = 0 .. ceil(T / R) - 1,  terms before the record omitted

-- by definition ``chd.downmix(fc).filter(b).downsample(R)``.  The new time axis is ``t0 - (K - 1) / 2 / fs``, ``fs / R``; the phase uses the original
``t0``.  For real ``x`` the result carries HALF the analytic amplitude, exactly as the composition does: pass ``2 * b`` to restore it.

* :func:`demod` -- torch tensors in, time along dim 0.
* :func:`lowpass_taps`, :func:`passband_taps` -- the window designs behind ``ChannelData.getLowpassFilter`` / ``getPassbandFilter``.

There is no CPU fallback: without the library or a device the call raises.

The package exports the FUNCTION under this module's name (``qups_amd.demod(x, ...)``, as the other entries), so the attribute ``qups_amd.demod`` is the
function and ``import qups_amd.demod as m`` binds it too; the module is ``importlib.import_module("qups_amd.demod")`` or ``from qups_amd.demod import ...``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["demod", "demod_len", "lowpass_taps", "passband_taps", "MAX_TAPS", "MAX_RATIO", "TILE"]

MAX_TAPS, MAX_RATIO, TILE = _lib.DEMOD_MAX_K, _lib.DEMOD_MAX_R, _lib.DEMOD_TILE


def demod_len(T: int, ratio: int) -> int:
    """``ceil(T / ratio)``: the samples ``downsample`` keeps"""
    return -(-int(T) // int(ratio))


def start_cycles(fc, t0):
    """``frac(fc * t0)`` in float64: the start phases the kernel takes, in cycles"""
    c = float(fc) * np.asarray(t0, np.float64)
    return c - np.floor(c)


def start_groups(t0, rest):
    """``(values, gdiv, G)`` for a ``t0`` that broadcasts against the trace dimensions ``rest`` (row-major trace index ``c``): trace ``c`` starts at
    ``values[(c // gdiv) % G]``.  A scalar gives ``G = 1``; one non-singleton dimension (one start time per transmit) its size; anything else one value per trace."""
    t0 = np.asarray(t0, np.float64)
    if t0.size == 1:
        return t0.reshape(1), 1, 1
    shape = (1,) * (len(rest) - t0.ndim) + tuple(t0.shape)
    if len(shape) != len(rest) or any(a not in (1, b) for a, b in zip(shape, rest)):
        raise DasError(f"demod: t0 must be a scalar or broadcast against the trace dimensions {tuple(rest)}, got {tuple(t0.shape)}")
    big = [q for q, n in enumerate(shape) if n > 1]
    if len(big) == 1:
        q = big[0]
        return t0.reshape(-1), int(np.prod(rest[q + 1:], dtype=np.int64)), int(shape[q])
    full = np.ascontiguousarray(np.broadcast_to(t0.reshape(shape), rest)).reshape(-1)
    return full, 1, int(full.size)


def demod(x, fc, fs, t0, b, ratio, out_half=False):
    """``x`` (``T x ...``, a device tensor: int16, float32, complex64, float64 or complex128) mixed down by ``fc``, filtered by the real FIR taps ``b`` and
    decimated by the integer ``ratio``, in one launch: ``ceil(T / ratio) x ...``, complex64 (complex128 for double data), or with ``out_half`` complex32 --
    interleaved half pairs, what ``DAS(..., prec='halfT')`` takes.  ``t0`` is a scalar or an array that broadcasts against ``x`` with a leading 1 (one start
    time per transmit, as in ``downmix``).  The result is time-fastest in memory like ``hilbert``'s; an ``x`` that is not time-fastest
    (a row-major ``T x N x M`` tensor, a permuted view) is brought there by ONE transposing copy, ``x.movedim(0, -1).contiguous()``.  Real ``x``: half the analytic amplitude, as the composition; ``2 * b`` restores it.
    Queued on torch's current stream; nothing synchronises when ``b`` is already a device tensor and ``t0`` a scalar."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise DasError("demod: x must be a device tensor (there is no CPU fallback in this package)")
    types = {torch.int16: _lib.DEMOD_I16, torch.float32: _lib.DEMOD_F32, torch.complex64: _lib.DEMOD_C64, torch.float64: _lib.DEMOD_F64,
             torch.complex128: _lib.DEMOD_C128}
    if x.dtype not in types:
        raise DasError(f"demod: x is int16, float32, complex64, float64 or complex128, got {str(x.dtype).replace('torch.', '')}")
    dbl = x.dtype in (torch.float64, torch.complex128)
    if out_half and dbl:
        raise DasError("demod: out_half goes with int16, float32 and complex64 data")
    ratio = int(ratio)
    if ratio < 1:
        raise DasError("ratio must be a positive integer")
    if x.ndim < 1:
        raise DasError("demod: x needs a time dimension")
    dev = x.device
    rdt = torch.float64 if dbl else torch.float32
    bt = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(b, np.float64)))
    if bt.is_complex():
        raise DasError("demod: the taps b must be real")
    bt = bt.reshape(-1).to(device=dev, dtype=rdt).contiguous()
    K = int(bt.numel())
    if K < 1:
        raise DasError("demod: the filter needs at least one tap")
    T = int(x.shape[0])
    rest = tuple(int(v) for v in x.shape[1:])
    Cn = int(np.prod(rest, dtype=np.int64)) if rest else 1
    J = demod_len(T, ratio)
    t0a = np.asarray(t0, np.float64)
    if t0a.size > 1:
        if t0a.ndim == x.ndim and t0a.shape[0] == 1:
            t0a = t0a.reshape(t0a.shape[1:])
        elif t0a.ndim >= x.ndim:
            raise DasError("demod: t0 must not vary along time")
    vals, gdiv, G = start_groups(t0a, rest)
    cyc0 = torch.from_numpy(np.ascontiguousarray(start_cycles(fc, vals))).to(dev)
    xc = x.movedim(0, -1).contiguous().reshape(Cn, T)                # C x T, time fastest: a view when x already is, else the one copy
    if out_half:
        y = torch.empty((Cn, J, 2), dtype=torch.float16, device=dev)
    else:
        y = torch.empty((Cn, J), dtype=torch.complex128 if dbl else torch.complex64, device=dev)
    d = _lib.DemodDesc()
    d.T, d.C, d.K, d.R = T, Cn, K, ratio
    d.x_ld, d.out_ld = T, J
    d.in_type, d.out_half = types[x.dtype], int(bool(out_half))
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.fc_over_fs, d.step = float(fc) / float(fs), float(fc) * ratio / float(fs)
    d.cyc0 = C.c_void_p(cyc0.data_ptr())
    d.gdiv, d.G = gdiv, G
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_demod(C.byref(d), C.c_void_p(xc.data_ptr()), C.c_void_p(bt.data_ptr()), C.c_void_p(y.data_ptr())))
    if out_half:
        y = torch.view_as_complex(y)
    return y.t().reshape((J,) + rest)


# ---- the two window designs of ChannelData.getLowpassFilter / getPassbandFilter
def lowpass_taps(cutoff, fs, N=25):
    """``N + 1`` taps of the Hamming-window low-pass with the 6 dB point at ``cutoff`` [Hz] (``scipy.signal.firwin``): ``sinc`` times the window, scaled to
    unit gain at DC"""
    from scipy.signal import firwin
    if not 0 < cutoff < fs / 2:
        raise DasError("the cutoff must lie between 0 and fs / 2")
    return firwin(int(N) + 1, float(cutoff), window="hamming", pass_zero=True, fs=float(fs))


def passband_taps(band, fs, N=25):
    """``N + 1`` taps of the Hamming-window band-pass with the 6 dB points at ``band = (f1, f2)`` [Hz] (``scipy.signal.firwin``): the difference of two
    windowed sincs, scaled to unit gain at the band centre"""
    from scipy.signal import firwin
    f1, f2 = (float(v) for v in band)
    if not 0 < f1 < f2 < fs / 2:
        raise DasError("the band edges must satisfy 0 < f1 < f2 < fs / 2")
    return firwin(int(N) + 1, [f1, f2], window="hamming", pass_zero=False, fs=float(fs))
