"""Pair-wise windowed zero-normalized cross-correlation on the device: ``pwznxcorr`` (reference kern/pwznxcorr.m, the base-MATLAB branch:
``iflt = false``, i.e. ``convn(., w, 'same')``, a zero pad at the end of the record and ``circshift`` per lag).

It estimates time shifts between neighbouring channels, or between every channel and a reference trace -- of channel data or of what
``UltrasoundSystem.DAS(chd, keep_rx=True)`` returns (``tdim=1``, ``ndim`` the receive dimension).  ``tdim``, ``ndim`` and ``ldim`` are 1-based
as in the reference (and as ``dim`` in :mod:`qups_amd.coherence`).

The work is one ``qdas_pwznxcorr`` launch (``libqdas.so``, ``csrc/pwznxcorr.hip``) for all lags on torch's current stream; there is no CPU
fallback.  The kernel reads the input where it lies whenever the time dimension is contiguous and the remaining (batch) dimensions merge into
at most two (size, stride) groups -- the view ``DAS`` returns among them; any other layout gets one contiguous copy with time fastest.
float16 / bfloat16 / complex32 data is computed in single precision and cast back.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .coherence import _check_dim, _device_of, _is_complex, _shape_of, _work_dtypes

__all__ = ["pwznxcorr", "record_layout", "TIME_TILE", "MAX_LAGS", "LDS_LIMIT", "lds_bytes"]

TIME_TILE = 256          # output times per workgroup (include/qdas.h QDAS_PWZNXCORR_TIME_TILE)
MAX_LAGS = 1024          # lags per call (QDAS_PWZNXCORR_MAX_LAGS)
LDS_LIMIT = 64 * 1024    # LDS of one workgroup [bytes]


def lds_bytes(itemsize, cplx, W, span):
    """LDS one workgroup needs [bytes] for a window of W samples and lags spanning ``span = max - min``; ``itemsize``: of the REAL type.
    Mirrors ``qdas_pwznxcorr_lds_bytes``; calls above :data:`LDS_LIMIT` are refused (``QDAS_EUNSUPPORTED``)."""
    es = itemsize * (2 if cplx else 1)
    nA, nraw = TIME_TILE + W - 1, TIME_TILE + 2 * (W - 1)
    return (2 * nA + nraw + nraw + span) * es + nA * itemsize


# ---------------------------------------------------------------------------------------------------------------- layout (pure, no device)
def record_layout(shape, strides, t, n, others=()):
    """Map a strided array of records onto ``qdas_pwznxcorr``'s layout.

    ``shape`` / ``strides`` in elements; ``t`` / ``n``: the 0-based time and channel dimensions.  ``others``: stride tuples of further operands
    that share the index space (a stride of 0 broadcasts).  Returns ``(groups, order)``: ``groups`` two batch groups
    ``(size, stride, other_strides, first_dim)``, fastest first (``(1, 0, (0, ...), None)`` pads unused ones), ``order`` the batch dimensions
    of size > 1 in memory order.  Returns ``None`` where the layout cannot be passed in place: the time dimension is not contiguous in some
    operand, or the batch dimensions do not merge into two groups in every operand at once (the caller copies)."""
    if shape[t] > 1 and (strides[t] != 1 or any(o[t] != 1 for o in others)):
        return None
    batch = [d for d in range(len(shape)) if d not in (t, n) and shape[d] > 1]
    order = sorted(batch, key=lambda d: (strides[d], d))
    groups = []
    for d in order:
        g = groups[-1] if groups else None
        if g and g[0] * g[1] == strides[d] and all(g[0] * go == o[d] for go, o in zip(g[2], others)):
            g[0] *= shape[d]
        else:
            groups.append([shape[d], strides[d], tuple(o[d] for o in others), d])
    if len(groups) > 2:
        return None
    groups += [[1, 0, tuple(0 for _ in others), None]] * (2 - len(groups))
    return [tuple(g) for g in groups], order


def _time_fastest(x, t, n):
    """one contiguous copy with time fastest, then the channels, then the other dimensions in order"""
    mem = [t, n] + [d for d in range(x.ndim) if d not in (t, n)]
    perm = mem[::-1]
    return x.permute(perm).contiguous().permute([perm.index(d) for d in range(x.ndim)])


def _bcast_strides(x0):
    return tuple(0 if x0.shape[d] == 1 else x0.stride(d) for d in range(x0.ndim))


def _prepare(x, x0, t, n):
    """x (and the reference traces x0, or None) in a layout :func:`record_layout` accepts: returns (x, x0, (groups, order), how), how in
    {'none', 'copy'} telling whether x itself was copied."""
    how = "none"
    if record_layout(_shape_of(x), tuple(x.stride()), t, n) is None:
        x, how = _time_fastest(x, t, n), "copy"
    if x0 is None:
        return x, None, record_layout(_shape_of(x), tuple(x.stride()), t, n), how
    lay = record_layout(_shape_of(x), tuple(x.stride()), t, n, [_bcast_strides(x0)])
    if lay is None:
        x0 = _time_fastest(x0, t, n)
        lay = record_layout(_shape_of(x), tuple(x.stride()), t, n, [_bcast_strides(x0)])
    if lay is None:                                         # broadcast batch dimensions that split x's groups: x0 in full, both dense
        full = [x0.shape[d] if d in (t, n) else x.shape[d] for d in range(x.ndim)]
        x, x0, how = _time_fastest(x, t, n), _time_fastest(x0.expand(full), t, n), "copy"
        lay = record_layout(_shape_of(x), tuple(x.stride()), t, n, [_bcast_strides(x0)])
    return x, x0, lay, how


# ---------------------------------------------------------------------------------------------------------------- arguments (no device)
def expand_lags(lags):
    """the reference's lag list: a scalar integer L means -L:L; returns an int64 array.  Non-integer lags (the reference interpolates) raise."""
    a = np.atleast_1d(np.asarray(lags.cpu() if hasattr(lags, "cpu") else lags, dtype=np.float64)).ravel()
    if not np.all(np.isfinite(a)):
        raise ValueError("pwznxcorr: lags must be finite")
    if np.any(a != np.floor(a)):
        raise NotImplementedError("pwznxcorr: non-integer lags (the reference's interpolated branch) are not built")
    if a.size == 1:
        return np.arange(-int(a[0]), int(a[0]) + 1, dtype=np.int64)
    return np.ascontiguousarray(a.astype(np.int64))


def default_window(lags):
    """``max(ceil(max|lags| / 2), 1)``"""
    m = int(np.max(np.abs(lags))) if lags.size else 0
    return max(-(-m // 2), 1)


def parse_window(W, lags, tdim, ndim, norm):
    """the time-window weights as a float64 vector.  ``W``: None (the default length), a scalar length (``ones(W)``, not scaled to a mean),
    a vector, or an array that is non-scalar along ``tdim`` only."""
    if W is None:
        W = default_window(lags)
    a = np.asarray(W.cpu() if hasattr(W, "cpu") else W)
    if np.iscomplexobj(a):
        raise ValueError("pwznxcorr: the window weights must be real")
    if a.ndim == 0:
        if not float(a).is_integer() or int(a) < 1:
            raise ValueError("pwznxcorr: a scalar W is the window length, a positive integer")
        return np.ones(int(a), np.float64)
    if a.ndim > 1:
        sz = list(a.shape) + [1] * (max(tdim, ndim) - a.ndim)
        if any(v != 1 for d, v in enumerate(sz) if d not in (tdim - 1, ndim - 1)):
            raise ValueError(f"The filter weights w must be scalar in all dimensions except time ({tdim}) and channel ({ndim}). "
                             "(QUPS:pwznxcorr:incompatibleWeightSize)")
        if sz[ndim - 1] != 1:
            raise NotImplementedError("pwznxcorr: a window that is non-scalar along the channel dimension (the reference's multi-channel form) is not built")
    w = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if w.size == 0:
        raise ValueError("pwznxcorr: the window is empty")
    if norm and np.any(w < 0):
        raise ValueError("pwznxcorr: a negative weight with norm=True makes the reference's denominator complex; pass norm=False")
    return w


def center_channels(N):
    """0-based channels whose mean is the reference trace of ``ref='center'``: channel (N+1)/2 for odd N, N/2 and N/2 + 1 for even N (1-based)"""
    mid = (N + 1) / 2
    return sorted({int(math.floor(mid)) - 1, int(math.ceil(mid)) - 1})


def plan(shape, lags, W=None, U=1, *, pad=True, zero=True, norm=True, ref="neighbor", stride=1, x0_shape=None, tdim=1, ndim=2, ldim=None,
         multi=False, lvec=True, iflt=False):
    """Everything :func:`pwznxcorr` decides before it touches data (no device needed): returns a dict with the expanded ``lags``, the weights
    ``w``, the padded number of dimensions ``D``, 0-based ``t`` / ``n``, 1-based ``ldim``, the channel count ``Nout`` and the result's ``shape``."""
    del lvec                                                 # (accepted and ignored: every lag is computed by the same launch)
    if isinstance(U, bool) or not float(U).is_integer() or int(U) < 1:
        raise ValueError("pwznxcorr: U must be a positive integer")
    if int(U) > 1:
        raise NotImplementedError("pwznxcorr: upsampling (U > 1) is not built")
    if multi:
        raise NotImplementedError("pwznxcorr: multi=True is not built")
    if iflt:
        raise NotImplementedError("pwznxcorr: iflt=True (imfilter, Image Processing Toolbox) is not built; the base-MATLAB branch is")
    if ref not in ("neighbor", "center", "x0"):
        raise ValueError('pwznxcorr: ref must be one of {"neighbor", "center", "x0"}')
    tdim, ndim = _check_dim(tdim, "tdim"), _check_dim(ndim, "ndim")
    if tdim == ndim:
        raise ValueError("pwznxcorr: tdim must differ from ndim")
    if isinstance(stride, bool) or not float(stride).is_integer() or int(stride) < 1:
        raise ValueError("pwznxcorr: stride must be a positive integer")
    lags = expand_lags(lags)
    w = parse_window(W, lags, tdim, ndim, norm)
    shape = tuple(int(v) for v in shape)
    D = max(len(shape), tdim, ndim)
    full = shape + (1,) * (D - len(shape))
    t, n = tdim - 1, ndim - 1
    N = full[n]
    if ref == "x0":
        if x0_shape is None:
            raise ValueError('pwznxcorr: ref="x0" needs the reference traces x0')
        xs = tuple(int(v) for v in x0_shape)
        if len(xs) > D:
            raise ValueError("pwznxcorr: x0 has more dimensions than x")
        xs = xs + (1,) * (D - len(xs))
        if xs[t] != full[t]:
            raise ValueError(f"pwznxcorr: x0 must have x's time length {full[t]}, not {xs[t]}")
        if any(xs[d] not in (1, full[d]) for d in range(D) if d != t):
            raise ValueError("pwznxcorr: the channel and batch dimensions of x0 must be 1 or equal to those of x")
    Nout = max(N - int(stride), 0) if ref == "neighbor" else N
    ldim = D + 1 if ldim is None else _check_dim(ldim, "ldim")
    if ldim <= D and full[ldim - 1] != 1:
        raise ValueError(f"pwznxcorr: ldim = {ldim} names a dimension of x of size {full[ldim - 1]}; the lag dimension must be new or singleton")
    if ldim - 1 in (t, n):
        raise ValueError("pwznxcorr: ldim must differ from tdim and ndim")
    core = list(full)
    core[n] = Nout
    if ldim <= D:
        out = core[:ldim - 1] + [lags.size] + core[ldim:]
    else:
        out = core + [1] * (ldim - D - 1) + [lags.size]
    return {"lags": lags, "w": w, "D": D, "t": t, "n": n, "ldim": ldim, "N": N, "Nout": Nout, "stride": int(stride), "shape": tuple(out),
            "P": (int(np.max(np.abs(lags))) if lags.size and pad else 0)}


# ---------------------------------------------------------------------------------------------------------------- the launch
def _launch(xl, xr, rsN, lay, T, Nout, t, n, w, lags, zero, norm, pad, dev):
    """xl / xr: tensors whose data pointers are the first left / right record; returns y with xl's dimensions (Nout channels) and the lags
    as a last dimension, time fastest in memory."""
    import torch
    groups, order = lay
    D = xl.ndim
    work = xl.dtype
    rdt = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(work, work)
    oshape = [xl.shape[d] for d in range(D)]
    oshape[n] = Nout
    ost, run = [0] * D, T
    ost[t] = 1
    ost[n] = run
    run *= Nout
    for d in order:
        ost[d] = run
        run *= oshape[d]
    for d in range(D):                                       # (singleton dimensions: any stride)
        if d not in (t, n) and d not in order:
            ost[d] = run
    y = torch.empty_strided(tuple(oshape) + (lags.size,), tuple(ost) + (run,), dtype=work, device=dev)
    wt = torch.from_numpy(w).to(device=dev, dtype=rdt)
    d = _lib.PwznxcorrDesc()
    d.dtype = _lib.QDAS_F64 if rdt == torch.float64 else _lib.QDAS_F32
    d.cplx = int(work.is_complex)
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.zero, d.norm, d.pad = int(bool(zero)), int(bool(norm)), int(bool(pad))
    d.T, d.N, d.W, d.nlags = T, Nout, w.size, lags.size
    d.xl_strideN, d.xr_strideN, d.y_strideN, d.y_strideL = (xl.stride(n) if Nout > 1 else 0), (rsN if Nout > 1 else 0), ost[n], run
    for i, (size, st, other, first) in enumerate(groups):
        d.bsize[i] = size
        d.xl_bstride[i] = st
        d.xr_bstride[i] = other[0] if other else st
        d.y_bstride[i] = ost[first] if first is not None else 0
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_pwznxcorr(C.byref(d), C.c_void_p(xl.data_ptr()), C.c_void_p(xr.data_ptr()), C.c_void_p(wt.data_ptr()),
                                             lags.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(y.data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return y


def pwznxcorr(x, lags, W=None, U=1, *, pad=True, zero=True, norm=True, ref="neighbor", stride=1, x0=None, tdim=1, ndim=2, ldim=None,
              multi=False, lvec=True, iflt=False):
    """Pair-wise windowed zero-normalized cross-correlation (reference kern/pwznxcorr.m, ``iflt = false``).

    ``x``: real or complex data with time along ``tdim`` and channels along ``ndim`` (1-based); every other dimension is a batch.  For each
    channel pair, lag ``l`` and time ``s`` the result is the windowed inner product of the left trace with the conjugate of the right trace
    advanced by ``l`` samples, each optionally debiased (``zero``) and normalised (``norm``) within the window::

        K(a)[s] = sum_k w[k] a[s + floor(W/2) - k]                       (MATLAB's conv 'same'; a = 0 outside the padded record)
        xlz = xl - K(xl);  c = conj(circshift(xr, -l));  cz = c - K(c)
        y_l = K(xlz cz) / (sqrt(K(|xlz|^2)) sqrt(K(|cz|^2)))

    ``lags``: a scalar integer ``L`` means ``-L:L``, a vector exactly those lags (any order, duplicates allowed).  ``W``: a scalar window length
    (``ones(W)``) or the weights themselves; default ``max(ceil(max|lags| / 2), 1)``.  As in the reference, ``zero=True`` subtracts the
    weighted window SUM -- a scalar ``W`` is not scaled to a mean; pass ``ones(W) / W`` for the usual zero-normalized cross-correlation.
    ``pad=True`` appends ``max|lags|`` zeros to the records, on which the shift is circular; in that pad region ``xlz`` is ``-K(xl)``, and for a
    positive lag the first ``l`` samples wrap into it, both as in the reference.  With ``norm`` a 0/0 stays NaN.

    ``ref="neighbor"`` pairs channel ``n`` with ``n + stride`` (``N - stride`` pairs; none when ``N <= stride``: an empty result, nothing is
    launched); ``ref="center"`` pairs every channel with channel ``(N+1)/2`` (odd ``N``) or the mean of channels ``N/2`` and ``N/2 + 1`` (even
    ``N``, 1-based); ``ref="x0"`` with the traces ``x0``, whose time length is that of ``x`` and whose other dimensions are 1 or equal to
    those of ``x``.  The lags lie along ``ldim`` (default: a new last dimension; a dimension of ``x`` it names must have size 1).
    ``lvec`` is accepted and ignored.  Complex input gives complex output, real input real output.

    Not built (``NotImplementedError``): ``U > 1``, non-integer lags, ``multi=True``, a window that is non-scalar along the channel dimension,
    ``iflt=True``.  ``ValueError``: complex weights, a negative weight with ``norm=True`` (the reference's denominator turns complex), a
    window that is non-scalar outside ``tdim`` (QUPS:pwznxcorr:incompatibleWeightSize).  Windows and lag spans beyond the kernel's LDS budget
    (:func:`lds_bytes` > :data:`LDS_LIMIT`; ``W = 256`` with ``L = 256`` in complex double is inside) raise ``QdasError``."""
    import torch
    x0c = _is_complex(x0) if x0 is not None and ref == "x0" else False
    if not (_is_complex(x) or (x.dtype.is_floating_point if isinstance(x, torch.Tensor) else np.issubdtype(np.asarray(x).dtype, np.floating))):
        raise ValueError("pwznxcorr: x must be a floating-point array")
    p = plan(_shape_of(x), lags, W, U, pad=pad, zero=zero, norm=norm, ref=ref, stride=stride,
             x0_shape=_shape_of(x0) if x0 is not None and ref == "x0" else None, tdim=tdim, ndim=ndim, ldim=ldim, multi=multi, lvec=lvec, iflt=iflt)
    D, t, n, ldim, lg = p["D"], p["t"], p["n"], p["ldim"], p["lags"]
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    work, back = _work_dtypes(xt.dtype)
    if x0c and not work.is_complex:
        work = torch.complex128 if work == torch.float64 else torch.complex64
    if math.prod(p["shape"]) == 0:                           # no pairs, no samples or no lags: nothing is launched, no device needed
        return torch.zeros(p["shape"], dtype=back or work, device=xt.device)
    if not torch.cuda.is_available():
        raise RuntimeError("qups_amd: no HIP device visible -- pwznxcorr has no CPU fallback")
    dev = _device_of(xt)
    xt = xt.to(device=dev, dtype=work)
    xt = xt.reshape(tuple(xt.shape) + (1,) * (D - xt.ndim))
    N, S = p["N"], p["stride"]
    xr = None
    if ref == "center":
        xr = xt.index_select(n, torch.tensor(center_channels(N), device=dev)).mean(dim=n, keepdim=True)
    elif ref == "x0":
        xr = x0 if isinstance(x0, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x0))
        xr = xr.to(device=dev, dtype=work)
        xr = xr.reshape(tuple(xr.shape) + (1,) * (D - xr.ndim))
    xt, xr, lay, _ = _prepare(xt, xr, t, n)
    if xr is None:                                           # neighbours: two views of x, S channels apart
        xl, xr, rsN = xt.narrow(n, 0, N - S), xt.narrow(n, S, N - S), xt.stride(n)
    else:
        xl, rsN = xt, (0 if xr.shape[n] == 1 else xr.stride(n))
    y = _launch(xl, xr, rsN, lay, xt.shape[t], p["Nout"], t, n, p["w"], lg, zero, norm, pad, dev)
    if ldim <= D:
        y = y.movedim(D, ldim - 1).squeeze(ldim)
    else:
        for _ in range(ldim - D - 1):
            y = y.unsqueeze(D)
    if back is not None:
        y = y.to(back)
    return y
