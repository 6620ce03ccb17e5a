"""Scan conversion on the device: the reference's ``ScanPolar.scanConvert`` (``src/ScanPolar.m:143-201``) and ``ScanSpherical.scanConvert``
(``src/ScanSpherical.m:121-188``) on ``csrc/scanconvert.hip`` -- an image on a polar grid (``R x A x pages``) or a volume on a spherical grid
(``R x A x E x pages``) onto a Cartesian raster, with the envelope / log compression the reference's examples apply just before (``mod2db``) fused into the
same launch (``pre``).  ``include/qdas.h`` states the contract: float64 geometry, closed boundaries, the cell and lerp order, ``fill`` outside.

* :func:`scan_convert` -- polar: ``b[R x A x ...]`` -> ``Z x X x ...``.
* :func:`scan_convert3` -- spherical: ``b[R x A x E x ...]`` -> ``Z x X x Y x ...``.

Angles are in DEGREES, as in the reference, and are converted on the host with ``a * pi / 180``.  ``b`` is a device tensor (float32, float64, complex64 or
complex128; half precision is not built) and is READ IN PLACE through its strides -- the ``I1``-fastest view ``UltrasoundSystem.DAS`` returns and a row-major
tensor alike.  The trailing dimensions are the pages: they collapse into one page stride when they lie in memory like a column-major array (first page
dimension fastest, as in what ``DAS`` returns) or when there is at most one of them; otherwise ``b`` is copied once into that order.  The result has ``Z``
fastest in memory, then ``X`` (``Y``), then the pages in the order of ``b``'s trailing dimensions, first fastest.

Source orders other than ``'RAY'`` / ``'RAE'`` and angle wrap are not built (the reference has neither).  Everything is queued on torch's current stream of
``b``'s device; with host axes (or ``check_grid=False``) nothing synchronises.  There is no CPU fallback: without the library or a device the calls raise."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from . import geometry as G
from .das_spec import DasError

__all__ = ["scan_convert", "scan_convert3", "PRE"]

PRE = {"none": _lib.SC_PRE_NONE, "abs": _lib.SC_PRE_ABS, "db": _lib.SC_PRE_DB}


def _torch():
    import torch
    return torch


def deg2rad(a_deg):
    """``a * pi / 180`` in float64 (the conversion the C ABI's radians come from, on the host)"""
    return np.asarray(a_deg, np.float64) * np.pi / 180


def _is_dev(v):
    torch = _torch()
    return isinstance(v, torch.Tensor) and v.is_cuda


def _host(v):
    torch = _torch()
    return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)


def _axis(v, name, who, dev, check, angle=False, least=2):
    """a float64 device vector of an axis (angles: degrees in, radians out).  A host array is checked on the host, for free; a device tensor costs one
    synchronisation, which ``check_grid=False`` leaves out: then finite, strictly increasing axes are the caller's promise, as in the C ABI."""
    torch = _torch()
    if not _is_dev(v):
        h = _host(v)
        if h.size < least:
            raise DasError(f"{who}: the {name} axis needs at least {least} node{'s' if least > 1 else ''}, got {h.size}")
        if check:
            if not (np.all(np.isfinite(h)) and np.all(np.diff(h) > 0)):
                raise DasError(f"{who}: the {name} axis must be finite and strictly increasing")
            if angle and not (h[0] > -180.0 and h[-1] <= 180.0):
                raise DasError(f"{who}: the angles of {name} must lie in (-180, 180] degrees (there is no angle wrap)")
        return torch.from_numpy(deg2rad(h) if angle else h).to(dev)
    t = v.reshape(-1).to(device=dev, dtype=torch.float64)
    if t.numel() < least:
        raise DasError(f"{who}: the {name} axis needs at least {least} node{'s' if least > 1 else ''}, got {t.numel()}")
    if check:
        ok = torch.isfinite(t).all() & (t[1:] > t[:-1]).all()
        if angle:
            ok = ok & (t[0] > -180.0) & (t[-1] <= 180.0)
        if not bool(ok.item()):
            raise DasError(f"{who}: the {name} axis must be finite and strictly increasing" + (", its angles in (-180, 180] degrees" if angle else ""))
    return (t * math.pi / 180 if angle else t).contiguous()


def page_stride(shape, strides):
    """``(P, sp)`` when pages of the given trailing ``shape`` / ``strides`` (elements) lie ``sp`` apart in column-major page order (the first dimension
    fastest), else ``(P, None)``.  Dimensions of size 1 do not count; no page dimension at all: ``(1, 0)``."""
    P = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    dims = [(int(n), int(s)) for n, s in zip(shape, strides) if n != 1]
    if P == 0 or not dims:
        return P, 0
    sp, run = dims[0][1], dims[0][1] * dims[0][0]
    for n, s in dims[1:]:
        if s != run:
            return P, None
        run *= n
    return P, sp


def _colmajor_empty(shape, dtype, dev):
    torch = _torch()
    return torch.empty(tuple(reversed(shape)), dtype=dtype, device=dev).permute(*reversed(range(len(shape))))


def _convert(who, b, src_axes, origin, out_axes, pre, db_floor, fill, check_grid):
    """src_axes: [(values, name, is_angle)] for r, a[, e]; out_axes: [(values, name)] for x, [y,] z, all given"""
    torch = _torch()
    nd = len(src_axes)
    if not (isinstance(b, torch.Tensor) and b.is_cuda):
        raise DasError(f"{who}: b must be a device tensor (there is no CPU fallback in this package)")
    if b.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        raise DasError(f"{who}: b is float32, float64, complex64 or complex128 (half-precision images are not built), got {str(b.dtype).replace('torch.', '')}")
    if pre not in PRE:
        raise DasError(f"{who}: pre is 'none', 'abs' or 'db', got {pre!r}")
    og = np.asarray(origin, np.float64).reshape(-1)
    if og.size != 3 or not np.all(np.isfinite(og)):
        raise DasError(f"{who}: origin is 3 finite values (x, y, z)")
    if db_floor != db_floor:
        raise DasError(f"{who}: db_floor is NaN")
    dev = b.device
    src = [_axis(v, name, who, dev, check_grid, angle) for v, name, angle in src_axes]
    out = [_axis(v, name, who, dev, check_grid, least=1) for v, name in out_axes]
    if b.ndim < nd or tuple(b.shape[:nd]) != tuple(t.numel() for t in src):
        raise DasError(f"{who}: b is {' x '.join(n for _, n, _ in src_axes)} x ... = {' x '.join(str(t.numel()) for t in src)} x ..., got {tuple(b.shape)}")
    pshape = tuple(b.shape[nd:])
    P, sp = page_stride(pshape, b.stride()[nd:])
    if sp is None:                                                   # the pages do not lie one stride apart: one copy, column-major
        c = _colmajor_empty(tuple(b.shape), b.dtype, dev)
        c.copy_(b)
        b = c
        P, sp = page_stride(pshape, b.stride()[nd:])
    cplx = b.is_complex()
    real = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(b.dtype, b.dtype)
    odtype = b.dtype if pre == "none" else real
    oshape = (out[-1].numel(), out[0].numel()) + ((out[1].numel(),) if nd == 3 else ()) + pshape      # Z, X[, Y], pages
    res = _colmajor_empty(oshape, odtype, dev)
    d = _lib.ScanconvertDesc()
    d.R, d.A, d.E = src[0].numel(), src[1].numel(), (src[2].numel() if nd == 3 else 0)
    d.X, d.Z, d.Y = out[0].numel(), out[-1].numel(), (out[1].numel() if nd == 3 else 0)
    d.P = P
    d.sr, d.sa, d.se, d.sp = b.stride(0), b.stride(1), (b.stride(2) if nd == 3 else 0), sp
    d.dtype = _lib.QDAS_F32 if real == torch.float32 else _lib.QDAS_F64
    d.cplx, d.pre = int(cplx), PRE[pre]
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.origin[0], d.origin[1], d.origin[2] = og
    d.fill, d.db_floor = float(fill), float(db_floor)
    d.r, d.a = C.c_void_p(src[0].data_ptr()), C.c_void_p(src[1].data_ptr())
    d.x, d.z = C.c_void_p(out[0].data_ptr()), C.c_void_p(out[-1].data_ptr())
    if nd == 3:
        d.e, d.y = C.c_void_p(src[2].data_ptr()), C.c_void_p(out[1].data_ptr())
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_scanconvert(C.byref(d), C.c_void_p(b.data_ptr()), C.c_void_p(res.data_ptr())))
    return res


def _given(v, default):
    return default if v is None else (v if _is_dev(v) else _host(v))


def scan_convert(b, r, a_deg, origin=(0.0, 0.0, 0.0), x=None, z=None, *, pre="none", db_floor=-math.inf, fill=math.nan, check_grid=True):
    """``(b_cart, (x, y, z))``: the image(s) ``b`` (``R x A x ...``, a device tensor) of the polar scan ``r`` [m], ``a_deg`` [degrees] about ``origin`` on
    the Cartesian axes ``x``, ``z`` -- ``Z x X x ...``, ``Z`` fastest in memory.  With ``x`` / ``z`` absent the grid is
    :func:`qups_amd.geometry.cartesian_of_polar`'s (device axes are then fetched once); ``y`` is that function's single value.

    ``pre``: ``"none"`` (the result has ``b``'s type), ``"abs"`` (``|b|``) or ``"db"`` (``max(20 log10 |b|, db_floor)``), applied to the corner samples
    BEFORE the interpolation (``scanConvert(scan, mod2db(b))``); the result of ``"abs"`` / ``"db"`` is real.  ``db_floor = -inf`` is the reference's
    behaviour; images from ``DAS`` carry exact zeros outside their support, which is what the floor is for.  Outside the sector the result is ``fill``
    (NaN as in the reference; complex: ``fill + 0i``).  ``check_grid``: axes must be finite and strictly increasing, the angles within (-180, 180]."""
    who = "scan_convert"
    gx = gz = None
    gy = np.array([np.asarray(origin, float).reshape(-1)[1]])
    if x is None or z is None:
        gx, gy, gz = G.cartesian_of_polar(_host(r), _host(a_deg), origin)
    x, z = _given(x, gx), _given(z, gz)
    res = _convert(who, b, [(r, "r", False), (a_deg, "a_deg", True)], origin, [(x, "x"), (z, "z")], pre, db_floor, fill, check_grid)
    return res, (x, gy, z)


def scan_convert3(b, r, a_deg, e_deg, origin=(0.0, 0.0, 0.0), x=None, y=None, z=None, *, pre="none", db_floor=-math.inf, fill=math.nan, check_grid=True):
    """``(b_cart, (x, y, z))``: the volume(s) ``b`` (``R x A x E x ...``) of the spherical scan ``r``, ``a_deg``, ``e_deg`` about ``origin`` on the
    Cartesian axes -- ``Z x X x Y x ...``, ``Z`` fastest.  Absent axes come from :func:`qups_amd.geometry.cartesian_of_spherical`.  Several volumes
    (trailing dimensions) are this package's extension; otherwise as :func:`scan_convert`."""
    who = "scan_convert3"
    gx = gy = gz = None
    if x is None or y is None or z is None:
        gx, gy, gz = G.cartesian_of_spherical(_host(r), _host(a_deg), _host(e_deg), origin)
    x, y, z = _given(x, gx), _given(y, gy), _given(z, gz)
    res = _convert(who, b, [(r, "r", False), (a_deg, "a_deg", True), (e_deg, "e_deg", True)], origin, [(x, "x"), (y, "y"), (z, "z")],
                   pre, db_floor, fill, check_grid)
    return res, (x, y, z)
