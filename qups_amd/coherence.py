"""Aperture-reduction images of a receive-kept image on the device: ``slsc``, ``dmas``, ``cohfac`` and ``pcf`` (reference kern/slsc.m,
kern/dmas.m, kern/cohfac.m, kern/pcf.m; the MATLAB branch of each).

They take what ``UltrasoundSystem.DAS(chd, keep_rx=True)`` returns -- an ``I1 x I2 x I3 x F... x N`` device tensor -- and reduce the receive
aperture.  ``dim`` and ``kdim`` are 1-based as in the reference (and as in :func:`qups_amd.convd`); by default ``dim`` is the last
non-singleton dimension.  The output has the input's shape with the reduced dimension(s) set to 1.

The work is one ``qdas_coherence`` launch (``libqdas.so``, ``csrc/coherence.hip``) on torch's current stream; there is no CPU fallback.
The kernel reads the input where it lies: any layout whose pixels, after sorting by stride and merging dimensions that continue each other,
form at most three (size, stride) groups and are faster than the reduced dimension(s) -- the view ``DAS`` returns among them -- is passed
without a copy.  Other layouts are transposed first: a dense tensor with the reduced dimension(s) fastest (a contiguous ``... x N`` tensor)
through ``qdas_permute3``, anything else by one contiguous copy in torch.  ``cohfac`` over more than two dimensions makes that copy too.
float16 / complex32 data is computed in single precision and cast back, as the reference casts its result ``'like'`` the input.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

__all__ = ["slsc", "dmas", "cohfac", "pcf", "pixel_groups"]


# ---------------------------------------------------------------------------------------------------------------- layout (pure, no device)
def pixel_groups(shape, strides, reduced):
    """Map a strided array onto ``qdas_coherence``'s canonical layout.

    ``shape`` / ``strides`` in elements, ``reduced``: the 0-based reduced dimensions.  Returns ``(groups, order)``: ``groups`` three
    ``(size, stride)`` pixel groups, fastest first (``(1, 0)`` pads unused ones), ``order`` the non-reduced dimensions in memory order --
    the order of the output's memory.  Returns ``None`` where the layout cannot be expressed: more than three groups, or a reduced
    dimension faster than every pixel dimension (the caller transposes)."""
    red = [r for r in reduced if r < len(shape)]
    pix = [d for d in range(len(shape)) if d not in red]
    order = sorted(pix, key=lambda d: (strides[d], d))
    live = [d for d in order if shape[d] > 1]
    groups = []
    for d in live:
        if groups and groups[-1][0] * groups[-1][1] == strides[d]:
            groups[-1] = (groups[-1][0] * shape[d], groups[-1][1])
        else:
            groups.append((shape[d], strides[d]))
    if len(groups) > 3:
        return None
    if live:
        fastest = min(strides[d] for d in live)
        if any(shape[r] > 1 and strides[r] < fastest for r in red):
            return None
    groups += [(1, 0)] * (3 - len(groups))
    return groups, order


def _dense_reduced_first(shape, strides, reduced):
    """(A, C) when the array is one dense block whose fastest dimensions are exactly the reduced ones: an A x C row-major matrix
    (C = the reduced extent) that ``qdas_permute3`` turns pixel-fastest; else None."""
    live = sorted((d for d in range(len(shape)) if shape[d] > 1), key=lambda d: (strides[d], d))
    expect = 1
    for d in live:
        if strides[d] != expect:
            return None
        expect *= shape[d]
    nred = sum(1 for r in reduced if shape[r] > 1)
    if set(live[:nred]) != {r for r in reduced if shape[r] > 1}:
        return None
    Cn = math.prod(shape[r] for r in reduced)
    return expect // max(Cn, 1), Cn


def _to_canonical(x, reduced):
    """x (device) in a layout ``pixel_groups`` accepts: returns (tensor, how) with how in {'none', 'permute3', 'copy'}."""
    import torch
    shape, strides = tuple(x.shape), tuple(x.stride())
    if pixel_groups(shape, strides, reduced) is not None:
        return x, "none"
    ac = _dense_reduced_first(shape, strides, reduced)
    if ac is not None and ac[0] > 1 and (ac[0] + 63) // 64 <= 65535:
        A, Cn = ac
        y = torch.empty(x.numel(), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().qdas_permute3(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), A, 1, Cn, x.element_size(),
                                            C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        red = set(reduced)
        nst = [strides[d] * A if d in red else strides[d] // Cn for d in range(len(shape))]
        return y.as_strided(shape, nst), "permute3"
    # one contiguous copy: pixels fastest in dimension order, then the reduced dimensions in the order given
    mem = [d for d in range(len(shape)) if d not in reduced] + list(reduced)
    perm = mem[::-1]
    inv = [perm.index(d) for d in range(len(shape))]
    return x.permute(perm).contiguous().permute(inv), "copy"


# ---------------------------------------------------------------------------------------------------------------- arguments (no device)
def _shape_of(x):
    return tuple(int(v) for v in x.shape)


def _last_nonsingleton(shape):
    ds = [k for k, v in enumerate(shape) if v != 1]
    return ds[-1] + 1 if ds else None


def _check_dim(d, what):
    if isinstance(d, bool) or not float(d).is_integer() or int(d) < 1:
        raise ValueError(f"{what} must be a positive integer")
    return int(d)


def _is_complex(x):
    return bool(x.is_complex()) if hasattr(x, "is_complex") else np.iscomplexobj(x)


def _lag_spec(L, what):
    """scalar L -> ('range', 1, L); vector -> ('table', int64 array).  Empty sets and negative or non-integer lags raise."""
    a = np.asarray(L.cpu() if hasattr(L, "cpu") else L, dtype=np.float64).ravel()
    if a.size == 0:
        raise ValueError(f"{what}: the lag set is empty")
    if not np.all(np.isfinite(a)) or np.any(a != np.round(a)) or np.any(a < 0):
        raise ValueError(f"{what}: lags must be non-negative integers")
    if a.size == 1:                                          # MATLAB isscalar: lags = 1:L
        if a[0] < 1:
            raise ValueError(f"{what}: the lag set 1:{int(a[0])} is empty")
        return ("range", 1, int(a[0]))
    t = a.astype(np.int64)
    if np.all(np.diff(t) == 1):                              # consecutive, no duplicates: a range with the same L
        return ("range", int(t[0]), int(t[-1]))
    return ("table", np.ascontiguousarray(t))


def _work_dtypes(dt):
    """(dtype the kernel computes in, dtype of the result or None to keep)"""
    import torch
    if dt in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        return dt, None
    if dt in (torch.float16, torch.bfloat16):
        return torch.float32, dt
    if dt == torch.complex32:
        return torch.complex64, dt
    return torch.float64, None


# ---------------------------------------------------------------------------------------------------------------- the launch
def _device_of(x):
    import torch
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device(f"cuda:{torch.cuda.current_device()}")


def _run(fname, method, x, reduced, D, lags=None, gamma=1.0):
    """x: tensor or array; reduced: 0-based dims (< D); returns (y, y2) with the reference's shape (reduced dims 1), ndim = x.ndim."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"qups_amd: no HIP device visible -- {fname} has no CPU fallback")
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    nd0 = xt.ndim
    dev = _device_of(xt)
    work, back = _work_dtypes(xt.dtype)
    xt = xt.to(device=dev, dtype=work)
    if D > xt.ndim:
        xt = xt.reshape(tuple(xt.shape) + (1,) * (D - xt.ndim))
    cplx = xt.is_complex()
    rdt = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(work, work)
    if method == _lib.COH_COHFAC and sum(1 for r in reduced if xt.shape[r] > 1) > 2:
        mem = [d for d in range(D) if d not in reduced] + list(reduced)
        perm = mem[::-1]
        xt = xt.permute(perm).contiguous().permute([perm.index(d) for d in range(D)])
        merged = True
    else:
        xt, _ = _to_canonical(xt, reduced)
        merged = False
    shape, strides = _shape_of(xt), tuple(xt.stride())
    groups, order = pixel_groups(shape, strides, reduced)
    P = math.prod(shape[d] for d in order)
    oshape = list(shape)
    for r in reduced:
        oshape[r] = 1
    ost, run = [0] * D, 1
    for d in order:
        ost[d] = run
        run *= shape[d]
    for r in reduced:
        ost[r] = run
    odt = work if method in (_lib.COH_SLSC_AVERAGE, _lib.COH_SLSC_ENSEMBLE, _lib.COH_DMAS) else rdt
    y = torch.empty_strided(tuple(oshape), tuple(ost), dtype=odt, device=dev)
    y2 = torch.empty_strided(tuple(oshape), tuple(ost), dtype=rdt, device=dev) if method == _lib.COH_PCF else None
    if merged:
        N, sN, K, sK = math.prod(shape[r] for r in reduced), P, 1, 0
    else:
        N, sN = shape[reduced[0]], strides[reduced[0]]
        K, sK = (shape[reduced[1]], strides[reduced[1]]) if len(reduced) > 1 else (1, 0)
    if P and N:
        d = _lib.CoherenceDesc()
        d.method = method
        d.dtype = _lib.QDAS_F64 if rdt == torch.float64 else _lib.QDAS_F32
        d.cplx = int(cplx)
        d.device = dev.index if dev.index is not None else torch.cuda.current_device()
        d.N, d.K, d.strideN, d.strideK = N, K, sN, sK
        for i, (s, st) in enumerate(groups):
            d.size[i], d.stride[i] = s, st
        keep = None
        if lags is not None:
            if lags[0] == "range":
                d.lag_lo, d.lag_hi = lags[1], lags[2]
            else:
                keep = lags[1]
                d.lags = keep.ctypes.data_as(C.POINTER(C.c_int64))
                d.nlags = keep.size
        d.gamma = float(gamma)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().qdas_coherence(C.byref(d), C.c_void_p(xt.data_ptr()), C.c_void_p(y.data_ptr()),
                                                 C.c_void_p(y2.data_ptr() if y2 is not None else 0),
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        del keep
    elif N == 0:
        raise ValueError(f"{fname}: the reduced dimension is empty")

    def fin(t):
        if t is None:
            return None
        if back is not None:
            t = t.to(back if t.is_complex() or back in (torch.float16, torch.bfloat16) else torch.float16)
        return t.reshape(t.shape[:nd0]) if t.ndim > nd0 else t
    return fin(y), fin(y2)


# ---------------------------------------------------------------------------------------------------------------- public functions
def slsc(x, dim=None, L=None, method="average", kdim=None):
    """Short-lag spatial coherence across dimension ``dim`` (reference kern/slsc.m, MATLAB branch).

    ``L``: a scalar means lags ``1:L``, a vector exactly those lags; default ``max(1, floor(N/4))``.  The pairs are those whose lag
    ``|m - n|`` is in the set (duplicates count once); the normaliser ``L`` is the number of lags as given, duplicates and lags >= N
    included.  Lag 0 counts the diagonal once, as the MATLAB branch does (the reference's OpenCL kernel counts it twice): a fully
    coherent ``x`` with ``L = [0, 5]`` gives 3/4.

    ``method="average"``: ``x`` is normalised by its 2-norm over ``kdim`` (0/0 -> 0), then ``z = sum_S xh_n conj(xh_m) / (2 L (N - |m-n|))``
    over ``dim`` and ``kdim``.  ``method="ensemble"``: ``z = sum_S conj(x_m) x_n / a`` with ``a = sum_S |x_n|^2``, NaN samples omitted; an
    all-zero pixel gives NaN (MATLAB's ``0 * Inf``).  The reference's power-of-two pre-scaling of the ensemble estimator only guards the
    range of its sums and is not applied: fp32 sums of ``|x|^2`` neither overflow nor underflow for amplitudes between about 1e-18 and 1e15.

    ``kdim``: a second reduced dimension, the time kernel (pixels shifted in ``t0``, concatenated).  The result is complex for complex
    input, with an imaginary part that is zero in exact arithmetic (written as 0), and real for real input."""
    shape = _shape_of(x)
    if method not in ("average", "ensemble"):
        raise ValueError('method must be one of {"average", "ensemble"}')
    if dim is None:
        dim = _last_nonsingleton(shape) or 1
    dim = _check_dim(dim, "dim")
    kdim = _check_dim(kdim, "kdim") if kdim is not None else max(len(shape), dim) + 1
    if kdim == dim:
        raise ValueError("kdim must differ from dim")
    D = max(len(shape), dim, kdim)
    N = shape[dim - 1] if dim <= len(shape) else 1
    lags = _lag_spec(max(1, N // 4) if L is None else L, "slsc")
    red = [dim - 1] + ([kdim - 1] if kdim <= len(shape) and shape[kdim - 1] > 1 else [])
    m = _lib.COH_SLSC_AVERAGE if method == "average" else _lib.COH_SLSC_ENSEMBLE
    return _run("slsc", m, x, red, D, lags=lags)[0]


def dmas(bn, dim=None, L=None):
    """Delay-multiply-and-sum across dimension ``dim`` (reference kern/dmas.m): ``b = sum_lags sum_n x_n x_{n+l}`` (no conjugate), returned
    as ``exp(i angle(b)) sqrt(|b|)``.  A scalar ``L`` means lags ``1:L``, a vector ``intersect(1:N-1, L)``; default ``1:N-1`` (computed as
    ``((sum x)^2 - sum x^2) / 2``).  Real input gives the real ``sign(b) sqrt(|b|)``; MATLAB's result differs from it only by an imaginary
    part of the size of ``sin(pi)`` times the value."""
    shape = _shape_of(bn)
    if dim is None:
        dim = _last_nonsingleton(shape) or 1
    dim = _check_dim(dim, "dim")
    N = shape[dim - 1] if dim <= len(shape) else 1
    lags = ("range", 1, N - 1) if L is None else _lag_spec(L, "dmas")
    return _run("dmas", _lib.COH_DMAS, bn, [dim - 1], max(len(shape), dim), lags=lags)[0]


def cohfac(b, dim=None):
    """Coherence factor ``|sum b|^2 / sum |b|^2 / prod(size(b, dim))`` (reference kern/cohfac.m).  ``dim`` names one or more dimensions
    (1-based); more than two are reduced after one contiguous copy of the input.  Real output; 0/0 stays NaN."""
    shape = _shape_of(b)
    if dim is None:
        dim = _last_nonsingleton(shape) or 1
    dims = [_check_dim(d, "dim") for d in np.atleast_1d(np.asarray(dim)).ravel().tolist()]
    if not dims:
        raise ValueError("dim must name at least one dimension")
    if len(set(dims)) != len(dims):
        raise ValueError("dim must not repeat a dimension")
    D = max([len(shape)] + dims)
    red = [d - 1 for d in dims if d <= len(shape) and shape[d - 1] > 1] or [dims[0] - 1]
    return _run("cohfac", _lib.COH_COHFAC, b, red, D)[0]


def pcf(b, dim=None, gamma=1.0):
    """Phase coherence factor across dimension ``dim`` (reference kern/pcf.m, 'auxiliary' unwrapping): ``s0`` is the population standard
    deviation of ``angle(b)``, ``sa`` that of ``angle(b) - pi sign(angle(b))``, both omitting NaN; ``sf = min(s0, sa)`` and
    ``w = max(0, 1 - gamma / sqrt(pi/3) * sf)``.  Returns ``(w, sf)``, real.  Complex input only."""
    if not _is_complex(b):
        raise ValueError("Input must be complex. (QUPS:pcf:realInput)")
    shape = _shape_of(b)
    if dim is None:
        dim = max(1, _last_nonsingleton(shape) or 1)
    dim = _check_dim(dim, "dim")
    if not math.isfinite(float(gamma)):
        raise ValueError("gamma must be a real number")
    return _run("pcf", _lib.COH_PCF, b, [dim - 1], max(len(shape), dim), gamma=gamma)
