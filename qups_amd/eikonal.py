"""Travel times through a sound-speed map on the device, and the delay tables ``bfDASLUT`` takes sampled from them: the producer half of the
reference's ``bfEikonal`` (``src/UltrasoundSystem.m:4204-4331``; ``kern/msfm.m`` with two arguments: first order, four neighbours).

``msfm`` keeps ``kern/msfm.m``'s contract; ``eikonal`` solves many source sets in the same launches; ``eikonal_tables`` samples maps at pixel
positions (separable cubic convolution, NaN outside the grid); ``travel_time_tables`` chains the two in blocks of sources so that the maps of all
elements never have to coexist.  The work is ``qdas_eikonal`` / ``qdas_eikonal_tables`` (``libqdas.so``, ``csrc/eikonal.hip``) on torch's current
stream; there is no CPU fallback.  The pure helpers (``scan_grid``, ``grid_coordinates``, ``same_aperture``) need no device.

Volumes (``msfm3d``: first order, six neighbours) arrive under names of their own -- ``msfm3d``, ``eikonal3``, ``eikonal3_tables``,
``travel_time_tables3``, ``scan_grid3`` -- on ``qdas_eikonal3`` / ``qdas_eikonal3_tables`` (``csrc/eikonal3.hip``); the 2-D names keep their
behaviour, including their refusal of a third dimension.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["msfm", "eikonal", "eikonal_tables", "travel_time_tables", "last_passes", "pass_cap", "scan_grid", "grid_coordinates", "same_aperture",
           "msfm3d", "eikonal3", "eikonal3_tables", "travel_time_tables3", "pass_cap3", "scan_grid3"]

MAP_BUDGET_BYTES = 1 << 30          # maps that exist at one time (travel_time_tables): 1 GiB = 850 maps of the reference's 481 x 321 example
SNAP = 1e-11                        # cells: a coordinate this close to a node is the node


# ---------------------------------------------------------------------------------------------------------------- pure helpers (no device)
def scan_grid(scan):
    """The uniform 2-D grid behind a Cartesian scan: ``(origin (3,), dp, dims, axes, size)``.

    ``dims``: the two non-singleton array dimensions of ``scan.positions()`` (0-based, in order), ``axes``: the space axis (0 x, 1 y, 2 z) that
    varies along each, ``size``: ``(C1, C2)``.  Raises with the reference's text (``src/UltrasoundSystem.m:4271-4273``) when the steps differ,
    and for anything that is not a Cartesian grid with exactly one singleton dimension (volumes: :func:`scan_grid3`)."""
    return _uniform_grid(scan, 2, "bfEikonal: the sound speed grid must have exactly one singleton dimension (3-D grids, msfm3d, are not built)")


def scan_grid3(scan):
    """The uniform 3-D grid behind a Cartesian scan without a singleton dimension: ``(origin (3,), dp, dims, axes, size)`` as :func:`scan_grid`, with
    ``dims = (0, 1, 2)``, three ``axes`` and ``size = (C1, C2, C3)``; the same Cartesian and equal-step checks and the same reference text."""
    return _uniform_grid(scan, 3, "bfEikonal: a sound speed volume must have three non-singleton dimensions")


def _uniform_grid(scan, ndim, wrong_dims):
    pos = np.asarray(scan.positions(), float)
    if pos.ndim != 4 or pos.shape[0] != 3:
        raise DasError("bfEikonal: the sound speed grid must be a scan with 3 x I1 x I2 x I3 positions")
    shape = pos.shape[1:]
    dims = [d for d in range(3) if shape[d] > 1]
    if len(dims) != ndim:
        raise DasError(wrong_dims)
    not_cartesian = DasError("bfEikonal: the sound speed grid must be a Cartesian scan (one space axis per array dimension)")
    og = pos[:, 0, 0, 0].copy()
    axes, lines = [], []
    for d in dims:                                          # the line of positions along array dimension d through the first pixel
        line = np.moveaxis(pos, d + 1, 1)[:, :, 0, 0]     # 3 x shape[d]
        moving = np.flatnonzero(np.ptp(line, axis=1))
        if moving.size != 1:
            raise not_cartesian
        axes.append(int(moving[0]))
        lines.append(line[moving[0]])
    if len(set(axes)) != len(axes):
        raise not_cartesian
    steps = np.concatenate([np.diff(v) for v in lines])
    dp = float((lines[0][-1] - lines[0][0]) / (shape[dims[0]] - 1))             # the mean step of the first axis: what linspace meant
    # every position is origin + its axis offsets
    model = np.broadcast_to(og[:, None, None, None], pos.shape).copy()
    for d, a, v in zip(dims, axes, lines):
        model[a] += (v - og[a]).reshape([-1 if k == d else 1 for k in range(3)])
    if not np.allclose(model, pos, rtol=0, atol=1e-9 * abs(dp)):
        raise not_cartesian
    if not dp > 0 or not np.all(np.abs(steps - dp) <= 1e-9 * dp):               # (uniquetol of the steps is one value, :4264)
        raise DasError("The simulation scan must have equally sized steps in all non-singleton dimensions.")
    return og, dp, tuple(dims), tuple(axes), tuple(shape[d] for d in dims)


def grid_coordinates(P, origin, dp, axes):
    """1-based grid coordinates ``len(axes) x n`` of the positions ``P`` (``3 x n``): ``(P - origin) / dp + 1`` along the grid's axes (reference ``:4283-4284``).
    A coordinate within 1e-11 of a node is that node: the reference's interpolant takes the grid vectors themselves, so a position on a grid line
    is on it exactly, while the quotient is off by rounding.  This departs from the reference's plain quotient in one visible way: an ELEMENT whose
    quotient lands a rounding error below a grid line is floored to that line's node here and to the node before it there (where the outcome depends
    on the rounding of one division)."""
    P = np.asarray(P, float).reshape(3, -1)
    g = np.stack([(P[a] - origin[a]) / dp for a in axes]) + 1.0
    r = np.round(g)
    return np.where(np.abs(g - r) <= SNAP, r, g)


def same_aperture(us):
    """whether the transmit maps are the receive maps (reference ``:4300``: ``us.tx == us.rx``; here also: equal element positions)"""
    if us.tx is us.rx:
        return True
    a, b = np.asarray(us.tx.positions()), np.asarray(us.rx.positions())
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _check_sources(sp, size, base=1):
    """kern/msfm.m:96-99, its texts (1-based)"""
    sp1 = sp - base + 1
    if np.any(sp1 < 1) or np.any(np.isnan(sp1)):
        raise DasError("Source points must be >= 1 to be within the field.")
    for d in range(len(size)):
        if np.any(sp1[d] > size[d]):
            raise DasError(f"Source points must be <= {size[d]} in dimension {d + 1} to be in the field.")


# ---------------------------------------------------------------------------------------------------------------- device
def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("qups_amd: no HIP device visible -- the eikonal solver has no CPU fallback")
    return torch


def pass_cap(C1, C2):
    """the default cap on the solver's passes for a ``C1 x C2`` grid"""
    return int(_lib.lib().qdas_eikonal_pass_cap(int(C1), int(C2)))


def last_passes():
    """passes the calling thread's last solve took"""
    return int(_lib.lib().qdas_eikonal_last_passes())


def _speed_colmajor(c, dev, torch):
    ct = (c if hasattr(c, "is_cuda") else torch.from_numpy(np.asarray(c, dtype=np.float64))).to(dev, torch.float64)
    if ct.ndim != 2:
        raise DasError("eikonal: the speed map must be 2-D")
    return ct.t().contiguous()                             # memory: C1 fastest


def eikonal(c, dp, sources, base=1, max_passes=0, device=None):
    """Travel-time maps ``C1 x C2 x K`` (float64 device tensor, seconds) of ``K`` source sets through the speed map ``c`` (``C1 x C2``) on a grid
    of step ``dp``.  ``sources``: a ``2 x K`` array (one point per set) or a sequence of ``2 x P_k`` arrays, grid coordinates in index base ``base``,
    floored to a node.  ``max_passes``: 0 = the derived cap.  Raises :class:`qups_amd._lib.QdasError` (code ``QDAS_ENOCONV``) at the cap."""
    torch = _torch()
    dev = torch.device(device if device is not None else (c.device if hasattr(c, "is_cuda") and c.is_cuda else f"cuda:{torch.cuda.current_device()}"))
    if isinstance(sources, (list, tuple)) and len(sources) and np.ndim(sources[0]) == 2:
        sets = [np.asarray(s, np.float64).reshape(2, -1) for s in sources]
    else:
        a = np.asarray(sources, np.float64).reshape(2, -1)
        sets = [a[:, k:k + 1] for k in range(a.shape[1])]
    cc = _speed_colmajor(c, dev, torch)
    C2, C1 = (int(v) for v in cc.shape)
    K = len(sets)
    T = torch.empty((K, C2, C1), dtype=torch.float64, device=dev)
    if K == 0 or C1 * C2 == 0:
        return T.permute(2, 1, 0)
    for s in sets:
        _check_sources(s, (C1, C2), base)
    pts = np.ascontiguousarray(np.concatenate(sets, axis=1).T)           # npts x 2: (first, second) per point
    begin = np.zeros(K + 1, np.uint64)
    begin[1:] = np.cumsum([s.shape[1] for s in sets])
    d = _lib.EikonalDesc()
    d.C1, d.C2, d.K, d.npts = C1, C2, K, pts.shape[0]
    d.set_begin = begin.ctypes.data_as(C.POINTER(C.c_uint64))
    d.dp, d.base, d.max_passes = float(dp), int(base), int(max_passes)
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_eikonal(C.byref(d), C.c_void_p(cc.data_ptr()), C.c_void_p(pts.ctypes.data), C.c_void_p(T.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return T.permute(2, 1, 0)


def _maps_colmajor(T, torch):
    """(K, C2, C1)-contiguous storage of a C1 x C2 [x K] tensor"""
    if T.ndim == 2:
        T = T.unsqueeze(-1)
    return T.to(torch.float64).permute(2, 1, 0).contiguous()


def eikonal_tables(T, Pi, base=1, out=None):
    """Sample the maps ``T`` (``C1 x C2 x K``, device) at ``I`` pixels given by their grid coordinates ``Pi`` (``2 x I``): ``I x K`` float64, NaN outside the
    grid (``griddedInterpolant(grd, T, 'cubic', 'none')``).  ``out``: a ``K x I`` contiguous device tensor to fill (its transpose is returned)."""
    torch = _torch()
    dev = T.device
    Tm = _maps_colmajor(T, torch)
    K, C2, C1 = (int(v) for v in Tm.shape)
    pt = (Pi if hasattr(Pi, "is_cuda") else torch.from_numpy(np.asarray(Pi, np.float64))).to(dev, torch.float64).reshape(2, -1)
    I = int(pt.shape[1])
    pc = pt.t().contiguous()                                # I x 2: one coordinate pair per pixel
    tau = torch.empty((K, I), dtype=torch.float64, device=dev) if out is None else out
    if tuple(tau.shape) != (K, I) or not tau.is_contiguous() or tau.dtype != torch.float64:
        raise DasError("eikonal_tables: out must be a contiguous K x I float64 tensor")
    d = _lib.EikonalDesc()
    d.C1, d.C2, d.K, d.I, d.base = C1, C2, K, I, int(base)
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qdas_eikonal_tables(C.byref(d), C.c_void_p(Tm.data_ptr()), C.c_void_p(pc.data_ptr()), C.c_void_p(tau.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return tau.t()


def travel_time_tables(c, dp, src, Pi, Isz, base=1, max_passes=0, device=None, budget=None):
    """``I1 x I2 x I3 x K`` delay table (float64, device, in the memory layout ``qdas_das_lut`` reads) of ``K`` single-point sources ``src`` (``2 x K``):
    the sources are solved in blocks whose maps stay below ``budget`` bytes and each block is sampled before the next is solved."""
    tau, travel_time_tables.last_passes = _blocked_tables(2, c, dp, src, Pi, Isz, base, max_passes, device, budget)
    return tau


def _blocked_tables(nd, c, dp, src, Pi, Isz, base, max_passes, device, budget):
    """``(table, most passes of a block)`` for a map of ``nd`` = 2 | 3 dimensions"""
    torch = _torch()
    solve, sample, passes_of = (eikonal, eikonal_tables, last_passes) if nd == 2 else (eikonal3, eikonal3_tables, lambda: eikonal3.last_passes)
    src = np.asarray(src, np.float64).reshape(nd, -1)
    K = src.shape[1]
    I = int(np.prod(Isz))
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    buf = torch.empty((K, I), dtype=torch.float64, device=dev)
    ct = (c if hasattr(c, "is_cuda") else torch.from_numpy(np.asarray(c, dtype=np.float64))).to(dev, torch.float64)
    kb = max(1, min(65535, int((MAP_BUDGET_BYTES if budget is None else budget) // max(8 * ct.numel(), 1))))
    pt = (Pi if hasattr(Pi, "is_cuda") else torch.from_numpy(np.asarray(Pi, np.float64))).to(dev, torch.float64)
    passes = 0
    for k0 in range(0, K, kb):
        T = solve(ct, dp, src[:, k0:k0 + kb], base=base, max_passes=max_passes, device=dev)
        passes = max(passes, passes_of())
        sample(T, pt, base=base, out=buf[k0:k0 + kb])
        del T
    return buf.reshape((K,) + tuple(reversed(Isz))).permute(3, 2, 1, 0), passes


def msfm(F, source_points, use_second=False, use_cross=False):
    """``T = msfm(F, SourcePoints)`` (reference ``kern/msfm.m``): ``F`` the speed in cells per second (``C1 x C2``), ``source_points`` ``2 x K'``, 1-based,
    floored to a node; every point gets ``T = 0`` and ONE map ``C1 x C2`` (float64 device tensor) comes back.  First order, four neighbours -- what the
    reference's ``bfEikonal`` asks for; the second-order and cross stencils and 3-D maps are not built."""
    if use_second or use_cross:
        raise DasError("msfm: the second-order and cross stencils (UseSecond, UseCross) are not built")
    shape = tuple(int(v) for v in F.shape)
    if len(shape) > 2 and any(v > 1 for v in shape[2:]):
        raise DasError("msfm: 3-D speed maps (msfm3d) are not built")
    sp = np.asarray(source_points, np.float64)
    if sp.ndim == 1:
        sp = sp.reshape(-1, 1)
    if sp.shape[0] != 2:
        raise DasError("msfm: SourcePoints must be 2 x K for a 2-D speed map")
    _check_sources(sp, shape[:2])
    F2 = F.reshape(shape[:2])
    return eikonal(F2, 1.0, [sp], base=1)[:, :, 0]


# ---------------------------------------------------------------------------------------------------------------- volumes (csrc/eikonal3.hip)
def pass_cap3(C1, C2, C3):
    """the default cap on the 3-D solver's passes for a ``C1 x C2 x C3`` grid"""
    return int(_lib.lib().qdas_eikonal3_pass_cap(int(C1), int(C2), int(C3)))


def _desc3(C1, C2, C3, K, dev, torch):
    d = _lib.Eikonal3Desc()
    d.C1, d.C2, d.C3, d.K = C1, C2, C3, K
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.queue = torch.cuda.current_stream(dev).cuda_stream
    return d


def eikonal3(c, dp, sources, base=1, max_passes=0, device=None):
    """Travel-time maps ``C1 x C2 x C3 x K`` (float64 device tensor, seconds) of ``K`` source sets through the speed volume ``c`` (``C1 x C2 x C3``) on a
    grid of step ``dp``.  ``sources``: a ``3 x K`` array (one point per set) or a sequence of ``3 x P_k`` arrays, grid coordinates in index base ``base``,
    floored to a node.  ``max_passes``: 0 = the derived cap.  Raises :class:`qups_amd._lib.QdasError` (code ``QDAS_ENOCONV``) at the cap.  The call
    waits for the current stream (the host ends the iteration).  ``eikonal3.last_passes`` / ``eikonal3.last_visits``: the passes and the tile visits
    of the last solve."""
    torch = _torch()
    dev = torch.device(device if device is not None else (c.device if hasattr(c, "is_cuda") and c.is_cuda else f"cuda:{torch.cuda.current_device()}"))
    if isinstance(sources, (list, tuple)) and len(sources) and np.ndim(sources[0]) == 2:
        sets = [np.asarray(s, np.float64).reshape(3, -1) for s in sources]
    else:
        a = np.asarray(sources, np.float64).reshape(3, -1)
        sets = [a[:, k:k + 1] for k in range(a.shape[1])]
    ct = (c if hasattr(c, "is_cuda") else torch.from_numpy(np.asarray(c, dtype=np.float64))).to(dev, torch.float64)
    if ct.ndim != 3:
        raise DasError("eikonal3: the speed map must be 3-D")
    cc = ct.permute(2, 1, 0).contiguous()                  # memory: C1 fastest
    C3, C2, C1 = (int(v) for v in cc.shape)
    K = len(sets)
    T = torch.empty((K, C3, C2, C1), dtype=torch.float64, device=dev)
    eikonal3.last_passes = eikonal3.last_visits = 0
    if K == 0 or C1 * C2 * C3 == 0:
        return T.permute(3, 2, 1, 0)
    for s in sets:
        _check_sources(s, (C1, C2, C3), base)
    pts = np.ascontiguousarray(np.concatenate(sets, axis=1).T)           # npts x 3: (first, second, third) per point
    begin = np.zeros(K + 1, np.uint64)
    begin[1:] = np.cumsum([s.shape[1] for s in sets])
    with torch.cuda.device(dev):
        d = _desc3(C1, C2, C3, K, dev, torch)
        d.npts = pts.shape[0]
        d.set_begin = begin.ctypes.data_as(C.POINTER(C.c_uint64))
        d.dp, d.base, d.max_passes = float(dp), int(base), int(max_passes)
        L = _lib.lib()
        nbytes, passes = C.c_uint64(), C.c_uint32()
        _lib.check(L.qdas_eikonal3_work_bytes(C.byref(d), C.byref(nbytes)))
        work = torch.empty((int(nbytes.value),), dtype=torch.uint8, device=dev)
        rc = L.qdas_eikonal3(C.byref(d), C.c_void_p(cc.data_ptr()), C.c_void_p(pts.ctypes.data), C.c_void_p(T.data_ptr()),
                             C.c_void_p(work.data_ptr()), nbytes.value, C.byref(passes))
        eikonal3.last_passes = int(passes.value)
        _lib.check(rc)
        eikonal3.last_visits = int(work[:8].view(torch.int64).item())   # (the solve has waited for the stream: this read costs one small copy)
    return T.permute(3, 2, 1, 0)


eikonal3.last_passes = eikonal3.last_visits = 0


def eikonal3_tables(T, Pi, base=1, out=None):
    """Sample the maps ``T`` (``C1 x C2 x C3 x K``, device) at ``I`` pixels given by their grid coordinates ``Pi`` (``3 x I``): ``I x K`` float64, NaN outside
    the grid (``griddedInterpolant({g1, g2, g3}, T, 'cubic', 'none')``).  ``out``: a ``K x I`` contiguous device tensor to fill (its transpose is returned).
    One launch on the current stream, no synchronisation."""
    torch = _torch()
    dev = T.device
    if T.ndim == 3:
        T = T.unsqueeze(-1)
    Tm = T.to(torch.float64).permute(3, 2, 1, 0).contiguous()           # (K, C3, C2, C1)-contiguous: no copy for what eikonal3 returned
    K, C3, C2, C1 = (int(v) for v in Tm.shape)
    pt = (Pi if hasattr(Pi, "is_cuda") else torch.from_numpy(np.asarray(Pi, np.float64))).to(dev, torch.float64).reshape(3, -1)
    I = int(pt.shape[1])
    pc = pt.t().contiguous()                                # I x 3: one coordinate triplet per pixel
    tau = torch.empty((K, I), dtype=torch.float64, device=dev) if out is None else out
    if tuple(tau.shape) != (K, I) or not tau.is_contiguous() or tau.dtype != torch.float64:
        raise DasError("eikonal3_tables: out must be a contiguous K x I float64 tensor")
    with torch.cuda.device(dev):
        d = _desc3(C1, C2, C3, K, dev, torch)
        d.I, d.base = I, int(base)
        _lib.check(_lib.lib().qdas_eikonal3_tables(C.byref(d), C.c_void_p(Tm.data_ptr()), C.c_void_p(pc.data_ptr()), C.c_void_p(tau.data_ptr())))
    return tau.t()


def travel_time_tables3(c, dp, src, Pi, Isz, base=1, max_passes=0, device=None, budget=None):
    """``I1 x I2 x I3 x K`` delay table (float64, device, in the memory layout ``qdas_das_lut`` reads) of ``K`` single-point sources ``src`` (``3 x K``) in
    the volume ``c``: as :func:`travel_time_tables`, the sources are solved in blocks whose maps stay below ``budget`` bytes (one 129^3 map is 17 MB)
    and each block is sampled before the next is solved."""
    return _blocked_tables(3, c, dp, src, Pi, Isz, base, max_passes, device, budget)[0]


def msfm3d(F, source_points, use_second=False, use_cross=False):
    """``T = msfm3d(F, SourcePoints)`` (reference ``kern/msfm.m`` for ``size(F, 3) > 1``): ``F`` the speed in cells per second (``C1 x C2 x C3``),
    ``source_points`` ``3 x K'``, 1-based, floored to a node; every point gets ``T = 0`` and ONE map ``C1 x C2 x C3`` (float64 device tensor) comes back.
    First order, six neighbours -- what the reference's ``bfEikonal`` asks for; the second-order and cross stencils are not built."""
    if use_second or use_cross:
        raise DasError("msfm3d: the second-order and cross stencils (UseSecond, UseCross) are not built")
    shape = tuple(int(v) for v in F.shape)
    if len(shape) != 3:
        raise DasError("msfm3d: the speed map must be 3-D")
    sp = np.asarray(source_points, np.float64)
    if sp.ndim == 1:
        sp = sp.reshape(-1, 1)
    if sp.shape[0] != 3:
        raise DasError("msfm3d: SourcePoints must be 3 x K for a 3-D speed map")
    _check_sources(sp, shape)
    return eikonal3(F, 1.0, [sp], base=1)[:, :, :, 0]
