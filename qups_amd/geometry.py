"""Geometry producers consumed by the DAS path -- host logic, numpy only.

The reference keeps these in its definition classes; only the few formulas whose OUTPUT feeds the
kernel are restated here (``3 x N`` element positions / normals, ``3 x I1 x I2 x I3`` pixel grids,
and the per-sequence ``(Pv, Nv, options)`` mapping of ``UltrasoundSystem.DAS``).
"""
from __future__ import annotations

import numpy as np


def linear_array(numel: int, pitch: float, offset=(0.0, 0.0, 0.0)):
    """Element positions ``3 x N`` and normals of a linear array.

    reference ``src/TransducerArray.m:95-99`` (``x = linspace(-w/2, w/2, numel)``) and ``:101-109``
    (normals ``[sin(theta); 0; cos(theta)]`` with ``theta = rot(1) = 0``).
    """
    w = (numel - 1) * pitch
    x = np.linspace(-w / 2, w / 2, numel)
    p = np.stack([x, np.zeros(numel), np.zeros(numel)]) + np.asarray(offset, float).reshape(3, 1)
    n = np.stack([np.zeros(numel), np.zeros(numel), np.ones(numel)])
    return p, n


def convex_array(numel: int, radius: float, angular_pitch_deg: float, offset=(0.0, 0.0, 0.0)):
    """Positions / normals of a curvilinear array; apex ("center") at ``offset - [0,0,radius]``.

    reference ``src/TransducerConvex.m:85-92`` (``R [sin t; 0; cos t] - [0;0;R]``) and ``:94-102``.
    """
    aw = (numel - 1) * angular_pitch_deg
    th = np.deg2rad(np.linspace(-aw / 2, aw / 2, numel))
    n = np.stack([np.sin(th), np.zeros(numel), np.cos(th)])
    p = radius * n - np.array([[0.0], [0.0], [radius]]) + np.asarray(offset, float).reshape(3, 1)
    return p, n


def matrix_array(numd, pitch, offset=(0.0, 0.0, 0.0)):
    """Positions / normals of a matrix array of ``numd = (Nx, Ny)`` elements (a scalar: square) with ``pitch = (px, py)`` (a scalar: both) in the
    plane ``z = 0``: element ``ix + Nx iy`` lies at ``(x[ix], y[iy], 0)`` -- x runs fastest.

    reference ``src/TransducerMatrix.m:130-138`` (``x = linspace(-w/2, w/2, numd(1))``, ``y`` likewise with ``numd(end)`` and ``pitch(end)``,
    ``ndgrid(x, y, 0)`` flattened) and ``:140-147`` (normals ``[0; 0; 1]`` with ``rot = 0``).
    """
    nd = np.broadcast_to(np.asarray(numd, int).reshape(-1), (2,)) if np.size(numd) == 1 else np.asarray(numd, int).reshape(2)
    pt = np.broadcast_to(np.asarray(pitch, float).reshape(-1), (2,)) if np.size(pitch) == 1 else np.asarray(pitch, float).reshape(2)
    w, h = (nd[0] - 1) * pt[0], (nd[1] - 1) * pt[1]
    x, y = np.linspace(-w / 2, w / 2, nd[0]), np.linspace(-h / 2, h / 2, nd[1])
    X, Y = np.meshgrid(x, y, indexing="ij")
    numel = int(nd[0] * nd[1])
    p = np.stack([X.ravel(order="F"), Y.ravel(order="F"), np.zeros(numel)]) + np.asarray(offset, float).reshape(3, 1)
    n = np.stack([np.zeros(numel), np.zeros(numel), np.ones(numel)])
    return p, n


def scan_cartesian(x, z, y=(0.0,)):
    """Pixel positions ``3 x I1 x I2 x I3`` of a Cartesian scan in the reference's default order
    ``'ZXY'`` -- depth z is the FASTEST image axis (reference ``src/ScanCartesian.m:11,126-143``,
    ``src/Scan.m:194``)."""
    x, y, z = (np.asarray(v, float).reshape(-1) for v in (x, y, z))
    Z, X, Y = np.meshgrid(z, x, y, indexing="ij")
    return np.stack([X, Y, Z])


def scan_polar(r, a_deg, origin=(0.0, 0.0, 0.0), y=(0.0,)):
    """Pixel positions of a polar scan, order ``'RAY'``: ``z = r cos a``, ``x = r sin a`` about
    ``origin`` (reference ``src/ScanPolar.m:11,99-115``)."""
    r, a, y = (np.asarray(v, float).reshape(-1) for v in (r, a_deg, y))
    R, A, Y = np.meshgrid(r, np.deg2rad(a), y, indexing="ij")
    og = np.asarray(origin, float)
    return np.stack([R * np.sin(A) + og[0], Y + og[1], R * np.cos(A) + og[2]])


def scan_spherical(r, a_deg, e_deg, origin=(0.0, 0.0, 0.0)):
    """Pixel positions of a spherical scan, order ``'RAE'``: ``z = r cos e cos a``, ``x = r cos e sin a``, ``y = r sin e`` about ``origin`` -- the
    reference's ``[Z, X, Y] = sph2cart(deg2rad(A), deg2rad(E), R)`` (``src/ScanSpherical.m:77-93``)."""
    r, a, e = (np.asarray(v, float).reshape(-1) for v in (r, a_deg, e_deg))
    R, A, E = np.meshgrid(r, np.deg2rad(a), np.deg2rad(e), indexing="ij")
    og = np.asarray(origin, float)
    return np.stack([R * np.cos(E) * np.sin(A) + og[0], R * np.sin(E) + og[1], R * np.cos(E) * np.cos(A) + og[2]])


def _enclosing_step(r):
    """the reference's ``dr`` of an axis (``uniquetol(diff(r), 1e-3)``, ``src/ScanPolar.m:260``) as this package reads it: finite when all ``diff(r)`` agree
    within ``1e-3 max|diff(r)|``, and then the smallest difference; else NaN (an axis of one node: Inf)"""
    d = np.diff(np.asarray(r, float).reshape(-1))
    if d.size == 0:
        return np.inf
    return float(d.min()) if d.max() - d.min() <= 1e-3 * np.abs(d).max() else np.nan


def _stepped_axis(lo, hi, dr):
    """``dr * (floor(lo / dr) : ceil(hi / dr))`` (``src/ScanCartesian.m:175-177``).  An axis of zero extent on a multiple of ``dr`` (0, say) is the single
    value ``dr * floor(lo / dr)``; off a multiple it is, as in the reference, the two multiples around it, so that the axis contains it.  The end indices move
    out by one where rounding left ``dr * floor(lo / dr)`` above ``lo`` (``dr * ceil(hi / dr)`` below ``hi``): the axis contains ``[lo, hi]``."""
    k0, k1 = np.floor(lo / dr), np.ceil(hi / dr)
    k0 -= dr * k0 > lo
    k1 += dr * k1 < hi
    return dr * np.arange(k0, k1 + 1)


def _enclosing(pos, dr, fallback):
    lo, hi = pos.reshape(3, -1).min(1), pos.reshape(3, -1).max(1)
    if np.isfinite(dr) and dr > 0:
        return tuple(_stepped_axis(lo[k], hi[k], dr) for k in range(3))
    return tuple(fallback(k, lo[k], hi[k]) for k in range(3))


def cartesian_of_polar(r, a_deg, origin=(0.0, 0.0, 0.0), y=(0.0,)):
    """``(x, y, z)``: the axes of the Cartesian scan that encloses a polar scan, the reference's ``ScanCartesian(scanPolar)`` (``src/ScanPolar.m:203-226``).
    The bounds are those of all positions, per coordinate.  When the range axis has a step ``dr`` -- all ``diff(r)`` agree within ``1e-3 max|diff(r)|``, this
    package's reading of ``uniquetol(diff(r), 1e-3)``; ``dr`` is then the smallest difference -- every axis is ``dr * (floor(min / dr) : ceil(max / dr))``
    and an axis of zero extent on a multiple of ``dr`` the single value ``dr * floor(min / dr)`` (off one: the two multiples around it).  Otherwise the
    axes keep the reference's default counts: ``linspace(min, max, 161)`` for ``x`` and ``z`` and, for ``y``, the upper bound alone (``linspace(., ., 1)``).
    The axes contain every position of the source scan."""
    pos = scan_polar(r, a_deg, origin, y)
    return _enclosing(pos, _enclosing_step(r), lambda k, lo, hi: np.array([hi]) if k == 1 else np.linspace(lo, hi, 161))


def cartesian_of_spherical(r, a_deg, e_deg, origin=(0.0, 0.0, 0.0)):
    """``(x, y, z)`` that enclose a spherical scan, the reference's ``ScanCartesian(scanSpherical)`` (``src/ScanSpherical.m:190-214``): as
    :func:`cartesian_of_polar` when the range axis has a step; otherwise the two-point axes ``[min, max]`` the reference leaves behind (it sets ``'x', grd{1}``,
    the bounds themselves)."""
    pos = scan_spherical(r, a_deg, e_deg, origin)
    return _enclosing(pos, _enclosing_step(r), lambda k, lo, hi: np.array([lo, hi]) if hi > lo else np.array([lo]))


def sequence_args(seq_type: str, *, tx_pos=None, tx_normals=None, focus=None, tx_offset=(0.0, 0.0, 0.0)):
    """``(Pv, Nv, option_strings)`` exactly as ``UltrasoundSystem.DAS`` derives them from the
    sequence type (reference ``src/UltrasoundSystem.m:3340-3352``):

    * ``'FSA'``: ``Pv`` = transmit element positions, ``Nv`` = element normals, ``'diverging-waves'``
    * ``'PW'`` : ``Pv = [0;0;0]``, ``Nv = focus`` (unit normals), ``'plane-waves'``
    * ``'FC'|'VS'|'DV'``: ``Pv = focus``, ``Nv = normalize(focus - tx.offset)``; ``'DV'`` adds
      ``'diverging-waves'``
    """
    if seq_type == "FSA":
        return np.asarray(tx_pos, float), np.asarray(tx_normals, float), ["diverging-waves"]
    if seq_type == "PW":
        return np.zeros((3, 1)), np.asarray(focus, float), ["plane-waves"]
    if seq_type in ("FC", "VS", "DV"):
        f = np.asarray(focus, float)
        nf = f - np.asarray(tx_offset, float).reshape(3, 1)
        # NB the reference divides by norm(nf) of the whole 3 x M matrix (:3350); per-column
        # normalisation is the documented intent and identical for the sign test it feeds.
        nf = nf / np.linalg.norm(nf, axis=0, keepdims=True)
        return f, nf, (["diverging-waves"] if seq_type == "DV" else [])
    raise ValueError(f"unknown sequence type {seq_type!r}")


def point_target_data(scat_pos, scat_amp, Pr, Pv, Nv, *, VS=True, DV=False, c0=1540.0, fs, fc, T, t0=0.0,
                      bw=1.2, baseband=False, dtype=np.complex64):
    """Analytic echoes of point targets: ``x[t,n,m] = sum_k A_k g(t/fs + t0 - tau_k(n,m))`` with
    ``g(t) = exp(-(t fc bw)^2) exp(2j pi fc t)`` and ``tau_k = (dv + dr)/c0`` using the same time-of-flight
    model as the beamformer (reference ``src/bf.cu:104-114``).  A stand-in for ``greens``:
    synthetic-data generator for tests and benchmarks, NOT a simulator port."""
    P = np.asarray(scat_pos, float).reshape(3, -1)
    A = np.broadcast_to(np.asarray(scat_amp, float).reshape(-1), (P.shape[1],))
    Pr, Pv, Nv = (np.asarray(v, float).reshape(3, -1) for v in (Pr, Pv, Nv))
    N, M = Pr.shape[1], max(Pv.shape[1], Nv.shape[1])
    Pv = np.broadcast_to(Pv, (3, M)) if Pv.shape[1] == 1 else Pv
    Nv = np.broadcast_to(Nv, (3, M)) if Nv.shape[1] == 1 else Nv
    t0 = np.broadcast_to(np.asarray(t0, float).reshape(-1), (M,))
    t = np.arange(T)[:, None, None] / fs + t0[None, None, :]
    x = np.zeros((T, N, M), np.complex128)
    for k in range(P.shape[1]):
        rv = P[:, k:k + 1] - Pv
        if VS:
            r = np.linalg.norm(rv, axis=0)
            dv = r if DV else np.copysign(r, (rv * Nv).sum(0))
        else:
            dv = (rv * Nv).sum(0)
        dr = np.linalg.norm(P[:, k:k + 1] - Pr, axis=0)
        tau = (dv[None, :] + dr[:, None]) / c0             # N x M
        d = t - tau[None]
        g = np.exp(-(d * fc * bw) ** 2) * np.exp(2j * np.pi * fc * d)
        if baseband:                                       # downmixed at fc: x * exp(-2j pi fc t_abs)
            g = g * np.exp(-2j * np.pi * fc * t)
        x += A[k] * g
    return x.astype(dtype)
