"""Straight-ray integrals over a rectilinear grid, on the device: the reference's ``kern/wbilerpg.m`` (bilinear ray weights), ``kern/rayPaths.m`` (the
tomography system matrix) and ``kern/globalAverageC.m`` (average sound speed from an aperture to every focal point) on ``csrc/raypaths.hip``.

A ray from ``a`` to ``b`` is cut at every crossing with a grid line ``x = xg[i]`` / ``z = zg[k]`` and at its end points; only the part inside the grid counts
(end points outside are clipped, without the reference's warning).  A segment of length ``l`` gives the four corners of its cell ``l`` times the mean of the
corner's bilinear hat function along the segment, so ``sum(w f)`` is the exact line integral of the bilinear interpolant of ``f`` and the weights of a ray sum
to its clipped length.  Rays of zero length, rays that miss the grid and rays with a non-finite coordinate give nothing.

* :func:`wbilerpg` -- the triplets ``(w, ix, iz)``, ``4 x (X + Z + 1)`` per ray (``qdas_raypaths_weights``).
* :func:`ray_integrals` -- ``sum(w map)`` and the clipped length per ray without ever forming a triplet (``qdas_raypaths_integrate``): the fused path.
* :func:`ray_backproject` -- the transposed product ``sum_j w_j r[j]`` onto the grid (and the column sums), a gather per node: no triplets, no atomics
  (``qdas_raypaths_backproject``).  MATLAB's ``w' * r`` on the matrix ``rayPaths`` returns.
* :func:`ray_sart` -- SART on the two operators: arrival times to a slowness map.
* :func:`rayPaths` -- the sparse system matrix, from the triplets, in chunks.
* :func:`globalAverageC` -- on :func:`ray_integrals`.

Everything is queued on torch's current stream of the data's device.  There is no CPU fallback: without the library or a device the calls raise.

MAP LAYOUT.  ``ord`` names the map's array dimensions as the reference does: with ``"ZX"`` a map has shape ``Z x X`` (``maps[..., iz, ix]``), with ``"XZ"``
``X x Z``; the tensor's own strides are used, whatever its memory layout.  The ROW INDEX of :func:`rayPaths` is the reference's (``rayPaths.m:225``):
``iz + Z ix`` for ``"ZX"``, ``ix + X iz`` for ``"XZ"`` -- MATLAB's column-major flattening of such an array; in torch the block of one ray reshapes to
``X x Z`` (``"ZX"``) or ``Z x X`` (``"XZ"``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["wbilerpg", "ray_integrals", "ray_backproject", "ray_sart", "rayPaths", "globalAverageC", "slots", "default_bsize"]


def _torch():
    import torch
    return torch


def slots(X, Z):
    """``X + Z + 1``: the slots of one ray (every crossing with a grid line and the two end points bound the segments)"""
    return int(X) + int(Z) + 1


def default_bsize(X, Z, M):
    """the reference's default chunk of rays (``rayPaths.m:68``): the triplets of one chunk stay near 4 GiB at 8 bytes per value"""
    return max(1, (1 << 32) // (max(1, int(M)) * slots(X, Z) * 4 * 4 * 8))


def _device_of(*ts):
    torch = _torch()
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise DasError("raypaths: no HIP device (there is no CPU fallback in this package)")
    return torch.device("cuda", torch.cuda.current_device())


def _dtype_of(*ts):
    """float32 when every floating-point input is single, else float64 (MATLAB would refuse the mix; numpy's rule is the useful one here)"""
    torch = _torch()
    kinds = []
    for t in ts:
        if isinstance(t, torch.Tensor):
            if t.dtype in (torch.float16, torch.bfloat16):
                raise DasError("raypaths: half precision is not built (float32 or float64)")
            if t.is_complex():
                raise DasError("raypaths: real data only")
            kinds.append(t.dtype == torch.float32)
        else:
            a = np.asarray(t)
            if np.iscomplexobj(a):
                raise DasError("raypaths: real data only")
            if a.dtype == np.float16:
                raise DasError("raypaths: half precision is not built (float32 or float64)")
            kinds.append(a.dtype == np.float32)
    return torch.float32 if kinds and all(kinds) else torch.float64


def _as(t, dtype, dev):
    torch = _torch()
    if isinstance(t, torch.Tensor):
        return t.to(device=dev, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64))).to(device=dev, dtype=dtype)


def _grid(g, name, dtype, dev, check):
    """a grid vector on the device, strictly increasing and finite (checked on the host for host arrays, for free; for a device tensor the check is one
    synchronisation, which ``check_grid=False`` leaves out: monotonicity is then the caller's promise, as in the C ABI)"""
    torch = _torch()
    on_dev = isinstance(g, torch.Tensor) and g.is_cuda
    if not on_dev:
        h = np.asarray(g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g, dtype=np.float64).reshape(-1)
        if h.size < 2:
            raise DasError(f"raypaths: the {name}-grid needs at least 2 nodes, got {h.size}")
        if not (np.all(np.isfinite(h)) and np.all(np.diff(h) > 0)):
            raise DasError(f"raypaths: the {name}-grid vector must be finite, sorted and strictly monotonic")
        return torch.from_numpy(h).to(device=dev, dtype=dtype)
    t = g.reshape(-1).to(device=dev, dtype=dtype).contiguous()
    if t.numel() < 2:
        raise DasError(f"raypaths: the {name}-grid needs at least 2 nodes, got {t.numel()}")
    if check and not bool((torch.isfinite(t).all() & (t[1:] > t[:-1]).all()).item()):
        raise DasError(f"raypaths: the {name}-grid vector must be finite, sorted and strictly monotonic")
    return t


def _points(p, name, dtype, dev):
    """``2 x J`` (or ``2``, ``2 x 1``: one point for every ray) -> a ``J x 2`` contiguous device tensor of (x, z) pairs and J"""
    t = _as(p, dtype, dev)
    if t.ndim == 1:
        t = t.reshape(-1, 1)
    if t.ndim != 2 or t.shape[0] != 2:
        raise DasError(f"raypaths: {name} is 2 x J (x; z), got {tuple(t.shape)}")
    return t.t().contiguous(), int(t.shape[1])


def _pair(pa, pb, dtype, dev):
    a, Ja = _points(pa, "pa", dtype, dev)
    b, Jb = _points(pb, "pb", dtype, dev)
    if Ja != Jb and 1 not in (Ja, Jb):
        raise DasError(f"raypaths: pa holds {Ja} points and pb {Jb}: equal counts, or one point against many")
    J = max(Ja, Jb) if min(Ja, Jb) > 0 else 0
    return a, b, J, (0 if Ja == 1 and J > 1 else 1), (0 if Jb == 1 and J > 1 else 1)


def _strides(ord, X, Z):
    if ord == "ZX":
        return Z, 1          # xstride, zstride
    if ord == "XZ":
        return 1, X
    raise DasError(f"raypaths: ord must be 'ZX' or 'XZ', got {ord!r}")


def _desc(xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride, F=0):
    torch = _torch()
    d = _lib.RaypathsDesc()
    d.X, d.Z, d.J, d.F = xg.numel(), zg.numel(), J, F
    d.xstride, d.zstride, d.pa_stride, d.pb_stride = xstride, zstride, sa, sb
    d.dtype = _lib.QDAS_F32 if dtype == torch.float32 else _lib.QDAS_F64
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.xg, d.zg, d.pa, d.pb = (C.c_void_p(t.data_ptr()) for t in (xg, zg, a, b))
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return d


def _weights(xg, zg, a, b, J, sa, sb, dtype, dev):
    """the triplet buffers of J rays, ``J x K x 4`` in memory (the library's 4 x K x J with the first dimension fastest)"""
    torch = _torch()
    K = slots(xg.numel(), zg.numel())
    w = torch.empty((J, K, 4), dtype=dtype, device=dev)
    ix = torch.empty((J, K, 4), dtype=torch.int32, device=dev)
    iz = torch.empty((J, K, 4), dtype=torch.int32, device=dev)
    d = _desc(xg, zg, a, b, J, sa, sb, dtype, dev, 1, 1)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_raypaths_weights(C.byref(d), C.c_void_p(w.data_ptr()), C.c_void_p(ix.data_ptr()), C.c_void_p(iz.data_ptr())))
    return w, ix, iz


def wbilerpg(x, y, xa, ya, xb, yb, r=None, check_grid=True):
    """``(cxy, ixo, iyo)``, each ``4 x N x size(xa)`` with ``N = X + Y + 1``: the bilinear weights of every segment of the rays ``(xa, ya) -> (xb, yb)`` and the
    indices of the grid nodes they belong to -- the four corners ``(ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1)`` of a slot's cell.  Indices are 0-based and
    -1 in an empty slot (the reference: 1-based, 0); every slot is written.  Which slot a segment lands in is not defined, the sum over equal indices is.
    ``xa, ya, xb, yb``: arrays of one shape, host or device; the result lives on the device.  The returned tensors are views of ``size(xa) x N x 4`` buffers.
    A non-empty ``r`` (segment subdivisions, which ``rayPaths`` does not use) is not built."""
    torch = _torch()
    if r is not None and np.size(r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else r) > 0:
        raise NotImplementedError("wbilerpg: segment subdivisions (a non-empty r, and the iro output) are not built")
    dev = _device_of(xa, ya, xb, yb, x, y)
    dtype = _dtype_of(x, y, xa, ya, xb, yb)
    xg, zg = _grid(x, "x", dtype, dev, check_grid), _grid(y, "y", dtype, dev, check_grid)
    e = [_as(t, dtype, dev) for t in (xa, ya, xb, yb)]
    shape = tuple(e[0].shape)
    if any(tuple(t.shape) != shape for t in e):
        raise DasError("wbilerpg: all end-point coordinates must have the same size")
    a = torch.stack((e[0].reshape(-1), e[1].reshape(-1)), dim=1).contiguous()
    b = torch.stack((e[2].reshape(-1), e[3].reshape(-1)), dim=1).contiguous()
    J = a.shape[0]
    w, ix, iz = _weights(xg, zg, a, b, J, 1, 1, dtype, dev)
    nd = len(shape)
    perm = (nd + 1, nd) + tuple(range(nd))
    K = w.shape[1]
    return tuple(t.reshape(shape + (K, 4)).permute(perm) for t in (w, ix, iz))


def _integrate_into(y, ln, maps3, xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride):
    torch = _torch()
    d = _desc(xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride, F=maps3.shape[0])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_raypaths_integrate(C.byref(d), C.c_void_p(maps3.data_ptr()), C.c_void_p(y.data_ptr()),
                                                      None if ln is None else C.c_void_p(ln.data_ptr())))


FAN_RAYS = 1 << 22        # rays per launch of a fan of several origins: 64 MiB of expanded float32 end points at the most


def _fan(out, m3, xg, zg, a, b, dtype, dev, xstride, zstride):
    """``out[k, j]`` (``A x J``, contiguous) = the integral along origin ``a[k]`` -> end point ``b[j]``.  One origin is one launch with a point stride of 0.
    Several origins are expanded into explicit rays, origin by origin (neighbouring lanes then share the origin and walk to neighbouring end points), and
    launched together, ``FAN_RAYS`` at a time: a launch per origin would leave a device with a thousand SIMDs one wave each at 65 536 end points, and the
    walk is a chain of dependent steps that only other waves can hide."""
    A, J = a.shape[0], b.shape[0]
    if A == 0 or J == 0:
        return
    if A == 1:
        return _integrate_into(out[0], None, m3, xg, zg, a, b, J, 0, 1, dtype, dev, xstride, zstride)
    step = max(1, FAN_RAYS // J)
    for k0 in range(0, A, step):
        k1 = min(A, k0 + step)
        ae = a[k0:k1].repeat_interleave(J, dim=0)
        be = b.repeat(k1 - k0, 1)
        _integrate_into(out[k0:k1].view(-1), None, m3, xg, zg, ae, be, (k1 - k0) * J, 1, 1, dtype, dev, xstride, zstride)


def _maps(maps, ord, X, Z):
    """``(maps as F x d0 x d1, xstride, zstride, had_F)``; a single 2-D map keeps its own strides, a stack is made contiguous (maps X Z elements apart)"""
    torch = _torch()
    if not (isinstance(maps, torch.Tensor) and maps.is_cuda):
        raise DasError("ray_integrals: maps must be a device tensor")
    if maps.dtype not in (torch.float32, torch.float64):
        raise DasError(f"ray_integrals: float32 or float64 maps, got {str(maps.dtype).replace('torch.', '')}")
    _strides(ord, X, Z)
    want = (Z, X) if ord == "ZX" else (X, Z)
    if maps.ndim not in (2, 3) or tuple(maps.shape[-2:]) != want:
        raise DasError(f"ray_integrals: with ord = '{ord}' a map is {want[0]} x {want[1]} (or F such maps), got {tuple(maps.shape)}")
    had_F = maps.ndim == 3
    m3 = maps.contiguous() if had_F else maps.unsqueeze(0)
    s0, s1 = m3.stride(1), m3.stride(2)
    xstride, zstride = (s1, s0) if ord == "ZX" else (s0, s1)
    return m3, int(xstride), int(zstride), had_F


def ray_integrals(maps, xg, zg, pa, pb, ord="ZX", check_grid=True):
    """``(y, len)``: ``y[j] = integral of the bilinear interpolant of the map along the part of ray pa[j] -> pb[j] inside the grid``, and that part's length
    ``len[j]``.  ``maps``: a device tensor, ``Z x X`` for ``ord = "ZX"`` (``X x Z`` for ``"XZ"``), float32 or float64 -- the precision of the whole
    computation -- or ``F`` such maps, then ``y`` is ``F x J``.  ``pa``, ``pb``: ``2 x J`` (x; z), or one point (``2`` / ``2 x 1``) against many.
    One kernel walks each ray and gathers the map as it goes: no triplets, no atomics, no synchronisation (with host or unchecked grids)."""
    torch = _torch()
    if not isinstance(maps, torch.Tensor):
        raise DasError("ray_integrals: maps must be a device tensor")
    _strides(ord, 2, 2)
    if not maps.is_cuda or maps.dtype not in (torch.float32, torch.float64):
        _maps(maps, ord, 2, 2)                                                        # (raises: the message names what is wrong)
    dev, dtype = maps.device, maps.dtype
    xg, zg = _grid(xg, "x", dtype, dev, check_grid), _grid(zg, "z", dtype, dev, check_grid)
    m3, xstride, zstride, had_F = _maps(maps, ord, xg.numel(), zg.numel())
    a, b, J, sa, sb = _pair(pa, pb, dtype, dev)
    F = m3.shape[0]
    if J == 0 or F == 0:
        return torch.zeros((F, J) if had_F else (J,), dtype=dtype, device=dev), torch.zeros((J,), dtype=dtype, device=dev)
    y = torch.empty((F, J), dtype=dtype, device=dev)
    ln = torch.empty((J,), dtype=dtype, device=dev)
    _integrate_into(y, ln, m3, xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride)
    return (y if had_F else y[0]), ln


def _backproject_into(g, col, r2, xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride):
    """``g``: ``F`` contiguous maps or None (then ``col`` is the whole job); ``r2``: ``F x J`` contiguous; ``col``: one map or None"""
    torch = _torch()
    d = _desc(xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride, F=0 if g is None else g.shape[0])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_raypaths_backproject(C.byref(d), None if g is None else C.c_void_p(r2.data_ptr()), None if g is None else C.c_void_p(g.data_ptr()),
                                                        None if col is None else C.c_void_p(col.data_ptr())))


def _residuals(r, who):
    """the checks of a residual tensor that need no device: float32 or float64, ``J`` or ``F x J``"""
    torch = _torch()
    if not isinstance(r, torch.Tensor):
        raise DasError(f"{who}: r must be a device tensor")
    _dtype_of(r)
    if not r.is_floating_point():
        raise DasError(f"{who}: float32 or float64 values, got {str(r.dtype).replace('torch.', '')}")
    if r.ndim not in (1, 2):
        raise DasError(f"{who}: r holds J values (or F x J), got {tuple(r.shape)}")
    if not r.is_cuda:
        raise DasError(f"{who}: r must be a device tensor")


def ray_backproject(r, xg, zg, pa, pb, ord="ZX", colsum=False, check_grid=True):
    """``g``, or ``(g, col)`` with ``colsum=True``: ``g[iz, ix] = sum_j w_j(ix, iz) r[j]`` -- the transposed product of :func:`ray_integrals`, the residuals
    of the rays ``pa[j] -> pb[j]`` spread back over the nodes each ray weighs -- and ``col[iz, ix] = sum_j w_j(ix, iz)``, the column sums of the system matrix.
    ``r``: a device tensor of ``J`` values, float32 or float64 -- the precision of the whole computation -- or ``F x J``, then ``g`` is ``F`` maps.  A map is
    ``Z x X`` for ``ord = "ZX"``, ``X x Z`` for ``"XZ"``, contiguous.  ``pa``, ``pb``: ``2 x J`` (x; z), or one point (``2`` / ``2 x 1``) against many.
    One kernel, a lane per node asking every ray for its weight: no triplets, no atomics (two runs give the same bits), no synchronisation (with host or
    unchecked grids).  A ray that gives nothing in :func:`ray_integrals` gives nothing here, whatever its ``r[j]`` holds."""
    torch = _torch()
    _strides(ord, 2, 2)
    _residuals(r, "ray_backproject")
    dev, dtype = r.device, r.dtype
    xg, zg = _grid(xg, "x", dtype, dev, check_grid), _grid(zg, "z", dtype, dev, check_grid)
    X, Z = xg.numel(), zg.numel()
    a, b, J, sa, sb = _pair(pa, pb, dtype, dev)
    if r.shape[-1] != J:
        raise DasError(f"ray_backproject: r holds {r.shape[-1]} values per vector for {J} rays")
    had_F = r.ndim == 2
    r2 = (r if had_F else r.unsqueeze(0)).contiguous()
    F = r2.shape[0]
    shape = (Z, X) if ord == "ZX" else (X, Z)
    xstride, zstride = (1, X) if ord == "ZX" else (Z, 1)
    g = torch.empty((F,) + shape, dtype=dtype, device=dev)
    col = torch.empty(shape, dtype=dtype, device=dev) if colsum else None
    _backproject_into(g if F else None, col, r2, xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride)
    g = g if had_F else g[0]
    return (g, col) if colsum else g


def ray_sart(t, xg, zg, pa, pb, s0, iters=10, relax=1.0, ord="ZX", check_grid=True):
    """the slowness map after ``iters`` steps of SART from ``s0``: ``s <- s + relax C A' R (t - A s)`` with ``A`` the straight-ray matrix of the rays
    ``pa[j] -> pb[j]`` (:func:`ray_integrals`, :func:`ray_backproject`), ``R = 1 / len`` its row sums (the clipped lengths) and ``C = 1 / colsum`` its
    column sums, both computed once.  A ray of no length inside the grid and a node no ray weighs get the weight 0: the node keeps ``s0``.
    ``t``: ``J`` arrival times [s for a map in s/m]; ``s0``: a device tensor, ``Z x X`` (``ord = "ZX"``) or ``X x Z``, float32 or float64 -- the precision of
    the whole computation; it is not modified.  A fixed count of steps, no convergence test, nothing read back: the loop only queues work.
    ``relax`` in (0, 2), the range in which SART's weighted residual cannot grow."""
    torch = _torch()
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise DasError(f"ray_sart: iters must be a non-negative integer, got {iters!r}")
    if not (0 < float(relax) < 2):
        raise DasError(f"ray_sart: relax must lie in (0, 2), got {relax!r}")
    _strides(ord, 2, 2)
    if not isinstance(s0, torch.Tensor):
        raise DasError("ray_sart: s0 must be a device tensor")
    _dtype_of(s0)
    if not s0.is_cuda or s0.dtype not in (torch.float32, torch.float64):
        _maps(s0, ord, 2, 2)                                                          # (raises: the message names what is wrong)
    dev, dtype = s0.device, s0.dtype
    xg, zg = _grid(xg, "x", dtype, dev, check_grid), _grid(zg, "z", dtype, dev, check_grid)
    X, Z = xg.numel(), zg.numel()
    if s0.ndim != 2:
        raise DasError(f"ray_sart: s0 is one 2-D map, got {tuple(s0.shape)}")
    _maps(s0, ord, X, Z)
    a, b, J, sa, sb = _pair(pa, pb, dtype, dev)
    t = _as(t, dtype, dev).reshape(-1)
    if t.numel() != J:
        raise DasError(f"ray_sart: t holds {t.numel()} arrival times for {J} rays")
    s = s0.clone(memory_format=torch.contiguous_format)
    xstride, zstride = (1, X) if ord == "ZX" else (Z, 1)
    if J == 0 or iters == 0:
        return s
    geo = (xg, zg, a, b, J, sa, sb, dtype, dev, xstride, zstride)
    y, ln = torch.empty((1, J), dtype=dtype, device=dev), torch.empty((J,), dtype=dtype, device=dev)
    g, col = torch.empty_like(s).unsqueeze(0), torch.empty_like(s)
    _integrate_into(y, ln, s.unsqueeze(0), *geo)
    _backproject_into(None, col, None, *geo)
    zero = torch.zeros((), dtype=dtype, device=dev)
    rinv, cinv = torch.where(ln > 0, 1 / ln, zero), torch.where(col > 0, relax / col, zero)
    for it in range(int(iters)):
        if it:
            _integrate_into(y, None, s.unsqueeze(0), *geo)
        _backproject_into(g, None, torch.where(ln > 0, (t - y[0]) * rinv, zero).unsqueeze(0), *geo)
        s.addcmul_(g[0], cinv)
    return s


def rayPaths(xg, zg, pj, pa, ord="ZX", method="bilerp", bsize=None, check_grid=True):
    """``(w, d)``: the ray-path integral weights on the grid ``{xg, zg}`` for the rays ``pa -> pj``.  ``pj``, ``pa``: ``2 x J x M`` (x; z), broadcast against
    each other (``2``, ``2 x J`` and singleton ``J`` or ``M`` are taken).  ``w``: a coalesced ``torch.sparse_coo_tensor`` of size ``(I J) x M``, ``I = X Z``, in
    the precision of the points; weights on the same node are summed.  Row ``i + I j`` with ``i = iz + Z ix`` (``ord = "ZX"``) or ``ix + X iz`` (``"XZ"``),
    0-based (the module docstring says how that reshapes).  ``d``: ``J x M``, the FULL length ``|pa - pj|``, not the clipped one.  ``bsize``: rays ``j`` per
    chunk, so that the triplet buffers stay bounded (default: the reference's rule).  As the reference does, the call asserts that no weight is negative or
    NaN -- one synchronisation per chunk, which this function can afford (the fused :func:`ray_integrals` has none).  ``method = "xiaolin"`` is not built."""
    torch = _torch()
    if method == "xiaolin":
        raise NotImplementedError("rayPaths: method 'xiaolin' (Xiaolin Wu's line weights) is not built; the device path is 'bilerp'")
    if method != "bilerp":
        raise DasError(f"rayPaths: method must be 'bilerp' or 'xiaolin', got {method!r}")
    dev = _device_of(pj, pa, xg, zg)
    dtype = _dtype_of(pj, pa)
    gx, gz = _grid(xg, "x", dtype, dev, check_grid), _grid(zg, "z", dtype, dev, check_grid)
    X, Z = gx.numel(), gz.numel()
    xstride, zstride = _strides(ord, X, Z)
    P = []
    for p, name in ((pj, "pj"), (pa, "pa")):
        t = _as(p, dtype, dev)
        if t.ndim > 3 or t.ndim < 1 or t.shape[0] != 2:
            raise DasError(f"rayPaths: {name} is 2 x J x M, got {tuple(t.shape)}")
        P.append(t.reshape(tuple(t.shape) + (1,) * (3 - t.ndim)))
    try:
        shape = torch.broadcast_shapes(P[0].shape, P[1].shape)
    except RuntimeError:
        raise DasError(f"rayPaths: pj {tuple(P[0].shape)} and pa {tuple(P[1].shape)} do not broadcast") from None
    _, J, M = shape
    pjb, pab = P[0].expand(shape), P[1].expand(shape)
    I = X * Z
    if bsize is None:
        bsize = default_bsize(X, Z, M)
    if int(bsize) != bsize or bsize < 1:
        raise DasError(f"rayPaths: bsize must be a positive integer, got {bsize!r}")
    bsize = int(bsize)
    d = torch.linalg.vector_norm(pab - pjb, dim=0)                                   # J x M
    rows, cols, vals = [], [], []
    for j0 in range(0, J, bsize):
        j1 = min(J, j0 + bsize)
        n = (j1 - j0) * M
        if n == 0:
            continue
        a = pab[:, j0:j1, :].reshape(2, n).t().contiguous()                          # rays in (j, m) order
        b = pjb[:, j0:j1, :].reshape(2, n).t().contiguous()
        w, ix, iz = _weights(gx, gz, a, b, n, 1, 1, dtype, dev)
        if bool(((w < 0) | torch.isnan(w)).any().item()):
            raise AssertionError("rayPaths: found negative or NaN weights - this is likely due to numerical precision issues. Consider changing the grid "
                                 "axes and ensure that the grid contains all endpoints.")
        w, ix, iz = w.reshape(n, -1), ix.reshape(n, -1), iz.reshape(n, -1)
        val = (ix >= 0) & (ix < X) & (iz >= 0) & (iz < Z)
        ray, _ = val.nonzero(as_tuple=True)
        lin = zstride * iz[val].to(torch.int64) + xstride * ix[val].to(torch.int64)
        rows.append(lin + I * (j0 + torch.div(ray, M, rounding_mode="floor")))
        cols.append(ray % M)
        vals.append(w[val])
    if rows:
        idx = torch.stack((torch.cat(rows), torch.cat(cols)))
        v = torch.cat(vals)
    else:
        idx, v = torch.zeros((2, 0), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=dtype, device=dev)
    return torch.sparse_coo_tensor(idx, v, (I * J, M)).coalesce(), d


def globalAverageC(c, x, z, pa, pb, order="ZX", check_grid=True):
    """``c_avg``: the global average sound speed from the point ``pa`` to every point ``pb`` through the speed map ``c`` sampled on the grid ``{x, z}`` --
    the reference's ``globalAverageC(med, scan, pa, pb)`` with ``c = props(med, scan)``, ``x = scan.x``, ``z = scan.z``, ``order`` the map's two dimensions
    (``"ZX"``: ``Z x X``).  ``c``: a device tensor, float32 or float64.  ``pb``: ``2 x J`` (x; z); ``pa``: ``2`` / ``2 x 1`` -> ``J`` values, or, as an
    extension, ``2 x A`` with ``A > 1`` -> ``J x A``.

    Line by line as the reference: a ``pb`` outside the scan bounds ``[x[0], x[-1]] x [z[0], z[-1]]`` becomes NaN; ``c_avg = l / integral(1 / c) dl`` with
    ``l = |pa - pb|`` the FULL length of the ray while the integral runs over the part inside the grid only -- so a ``pa`` outside the grid biases the result
    (too fast: the outside part counts with slowness 0) exactly as it does in the reference; infinite results become NaN.  Runs on :func:`ray_integrals`'s
    kernel (several origins: expanded into rays and launched together): no triplets are formed."""
    torch = _torch()
    if not (isinstance(c, torch.Tensor) and c.is_cuda):
        raise DasError("globalAverageC: c must be a device tensor")
    if c.ndim != 2:
        raise DasError(f"globalAverageC: c is one 2-D map, got {tuple(c.shape)}")
    dev, dtype = c.device, c.dtype
    if dtype not in (torch.float32, torch.float64):
        raise DasError(f"globalAverageC: float32 or float64 map, got {str(dtype).replace('torch.', '')}")
    xg, zg = _grid(x, "x", dtype, dev, check_grid), _grid(z, "z", dtype, dev, check_grid)
    m3, xstride, zstride, _ = _maps(1 / c, order, xg.numel(), zg.numel())
    a, A = _points(pa, "pa", dtype, dev)
    b, J = _points(pb, "pb", dtype, dev)
    single = A == 1
    lo = torch.stack((xg[0], zg[0]))
    hi = torch.stack((xg[-1], zg[-1]))
    inside = ((b >= lo) & (b <= hi)).all(dim=1, keepdim=True)
    b = torch.where(inside, b, torch.full_like(b, float("nan")))
    out = torch.empty((A, J), dtype=dtype, device=dev)
    _fan(out, m3, xg, zg, a, b, dtype, dev, xstride, zstride)
    l = torch.linalg.vector_norm(a[:, None, :] - b[None, :, :], dim=2)                # A x J
    cavg = 1 / (out / l)
    cavg = torch.where(torch.isinf(cavg), torch.full_like(cavg, float("nan")), cavg)
    return cavg[0] if single else cavg.t()
