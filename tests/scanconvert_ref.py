"""A float64 numpy restatement of the scan conversion contract of include/qdas.h (qdas_scanconvert), for the tests: ``searchsorted`` cells, closed
boundaries, the lerps along r, then a, then e, ``pre`` on the corner samples, ``fill`` outside.  Also the case grids every scanconvert test shares.

The sector of the cases has the geometry of the C5 configuration: origin (0, 0, -49.6 mm), r from 49.6 to 99.6 mm, +-37 degrees (volumes: +-25 degrees of
elevation too); the Cartesian grid reaches 10 % beyond the sector on every side, so a third to a half of its pixels are outside.  Building a case ASSERTS that
every query lies at least 1e-9 of the axis span away from every boundary of the sector (``MARGIN``): that is what allows the device tests to demand an
identical inside mask.  A grid that violates it is a broken fixture, not a tolerance."""
import functools

import numpy as np

MARGIN = 1e-9
ORIGIN = (0.0, 0.0, -49.6e-3)
R0, R1, AMAX, EMAX = 49.6e-3, 99.6e-3, 37.0, 25.0
POLAR = {"2x2": (2, 2, 7, 5, False), "5x4": (5, 4, 23, 19, True), "17x9": (17, 9, 70, 65, True), "64x33": (64, 33, 130, 129, False)}      # R, A, Z, X, non-uniform
SPHERICAL = {"2x2x2": (2, 2, 2, 5, 5, 5, False), "5x4x3": (5, 4, 3, 13, 11, 9, True), "17x9x8": (17, 9, 8, 33, 31, 29, False)}           # R, A, E, Z, X, Y


def deg2rad(a_deg):
    return np.asarray(a_deg, np.float64) * np.pi / 180


# ---------------------------------------------------------------------------------------------------------------- the contract
def locate(g, p):
    """``(inside, cell, weight)`` of the coordinates ``p`` on the axis ``g``: inside iff ``g[0] <= p <= g[-1]`` (a NaN is outside); the cell is the largest
    ``k <= n - 2`` with ``g[k] <= p``"""
    g, p = np.asarray(g, np.float64), np.asarray(p, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (p >= g[0]) & (p <= g[-1])
    k = np.clip(np.searchsorted(g, np.where(inside, p, g[0]), side="right") - 1, 0, g.size - 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (p - g[k]) / (g[k + 1] - g[k])
    return inside, k, w


def polar_coords(origin, x, z):
    """``(rho, alpha)``, each ``Z x X``"""
    dz, dx = np.asarray(z, np.float64)[:, None] - origin[2], np.asarray(x, np.float64)[None, :] - origin[0]
    dz, dx = np.broadcast_arrays(dz, dx)
    return np.hypot(dz, dx), np.arctan2(dx, dz)


def spherical_coords(origin, x, y, z):
    """``(rho, alpha, eps)``, each ``Z x X x Y``"""
    dz = np.asarray(z, np.float64)[:, None, None] - origin[2]
    dx = np.asarray(x, np.float64)[None, :, None] - origin[0]
    dy = np.asarray(y, np.float64)[None, None, :] - origin[1]
    dz, dx, dy = np.broadcast_arrays(dz, dx, dy)
    return np.sqrt(dx * dx + dy * dy + dz * dz), np.arctan2(dx, dz), np.arctan2(dy, np.hypot(dz, dx))


def apply_pre(b, pre="none", db_floor=-np.inf):
    if pre == "none":
        return b
    m = np.abs(b)
    if pre == "abs":
        return m
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 20 * np.log10(m)
        return np.where(v < db_floor, db_floor, v)


def _lerp(a, b, t):
    with np.errstate(invalid="ignore", over="ignore"):
        return a + t * (b - a)


def convert_polar(b, r, a_rad, origin, x, z, pre="none", db_floor=-np.inf, fill=np.nan):
    """``(out, inside)``: ``b`` is ``R x A x P`` (float64 or complex128), ``out`` ``Z x X x P``, ``inside`` ``Z x X``"""
    v = apply_pre(np.asarray(b), pre, db_floor)
    rho, alpha = polar_coords(origin, x, z)
    ir, k, u = locate(r, rho)
    ia, l, w = locate(a_rad, alpha)
    inside = ir & ia
    u, w = u[..., None], w[..., None]
    lo = _lerp(v[k, l], v[k + 1, l], u)
    hi = _lerp(v[k, l + 1], v[k + 1, l + 1], u)
    out = _lerp(lo, hi, w)
    out[~inside] = fill
    return out, inside


def convert_spherical(b, r, a_rad, e_rad, origin, x, y, z, pre="none", db_floor=-np.inf, fill=np.nan):
    """``(out, inside)``: ``b`` is ``R x A x E x P``, ``out`` ``Z x X x Y x P``"""
    v = apply_pre(np.asarray(b), pre, db_floor)
    rho, alpha, eps = spherical_coords(origin, x, y, z)
    ir, k, u = locate(r, rho)
    ia, l, w = locate(a_rad, alpha)
    ie, m, t = locate(e_rad, eps)
    inside = ir & ia & ie
    u, w, t = u[..., None], w[..., None], t[..., None]
    sheets = []
    for mm in (m, m + 1):
        lo = _lerp(v[k, l, mm], v[k + 1, l, mm], u)
        hi = _lerp(v[k, l + 1, mm], v[k + 1, l + 1, mm], u)
        sheets.append(_lerp(lo, hi, w))
    out = _lerp(sheets[0], sheets[1], t)
    out[~inside] = fill
    return out, inside


def corner_max(b, pre, db_floor):
    """max |v| over the finite corner values after ``pre``: the scale of the tolerance"""
    v = np.abs(apply_pre(np.asarray(b), pre, db_floor))
    return float(v[np.isfinite(v)].max())


def g_factor(*axes):
    """the largest max|axis value| / min cell width over the source axes: float64 geometry rounding enters through the slope across a cell"""
    return max(float(np.abs(g).max() / np.diff(g).min()) for g in axes)


def bound(K, np_real, c, b, pre="none", db_floor=-np.inf):
    """the tolerance of the device and host-core tests on inside pixels: ``K (eps_dtype + eps64 G) max|v|`` with ``v`` the corner values after ``pre``"""
    axes = [c["r"], c["a"]] + ([c["e"]] if "e" in c else [])
    return K * (np.finfo(np_real).eps + np.finfo(np.float64).eps * g_factor(*axes)) * corner_max(b, pre, db_floor)


# ---------------------------------------------------------------------------------------------------------------- the case grids
def _axis(lo, hi, n, warp):
    t = np.linspace(0.0, 1.0, n)
    if warp is not None and n > 2:
        t = t ** warp
    g = lo + (hi - lo) * t
    g[-1] = hi
    return g


def _beyond(p, n):
    lo, hi = p.min(), p.max()
    return np.linspace(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n)


def _assert_margin(pairs, exempt=None):
    """every (axis, coordinates) pair: no coordinate within MARGIN of the span of the axis' two ends"""
    worst = np.inf
    for g, p in pairs:
        if exempt is not None:
            p = p[~exempt]
        d = min(np.abs(p - g[0]).min(), np.abs(p - g[-1]).min()) / (g[-1] - g[0])
        worst = min(worst, d)
    assert worst >= MARGIN, f"a query lies {worst:.3e} of an axis span from a boundary of the sector: broken fixture"
    return worst


@functools.lru_cache(maxsize=None)
def polar_case(name):
    """dict(r, a_deg, a, origin, x, z, margin): axes of one polar case; never modified"""
    R, A, Z, X, nu = POLAR[name]
    r = _axis(R0, R1, R, 1.3 if nu else None)
    a_deg = _axis(-AMAX, AMAX, A, 0.8 if nu else None)
    a = deg2rad(a_deg)
    px, pz = np.outer(r, np.sin(a)) + ORIGIN[0], np.outer(r, np.cos(a)) + ORIGIN[2]
    x, z = _beyond(px, X), _beyond(pz, Z)
    rho, alpha = polar_coords(ORIGIN, x, z)
    margin = _assert_margin(((r, rho), (a, alpha)))
    for v in (r, a_deg, a, x, z):
        v.setflags(write=False)
    return dict(r=r, a_deg=a_deg, a=a, origin=ORIGIN, x=x, z=z, margin=margin, uniform=not nu)


@functools.lru_cache(maxsize=None)
def spherical_case(name):
    R, A, E, Z, X, Y, nu = SPHERICAL[name]
    r = _axis(R0, R1, R, 1.3 if nu else None)
    a_deg, e_deg = _axis(-AMAX, AMAX, A, 0.8 if nu else None), _axis(-EMAX, EMAX, E, 1.2 if nu else None)
    a, e = deg2rad(a_deg), deg2rad(e_deg)
    RR, AA, EE = np.meshgrid(r, a, e, indexing="ij")
    px, py, pz = RR * np.cos(EE) * np.sin(AA) + ORIGIN[0], RR * np.sin(EE) + ORIGIN[1], RR * np.cos(EE) * np.cos(AA) + ORIGIN[2]
    x, y, z = _beyond(px, X), _beyond(py, Y), _beyond(pz, Z)
    rho, alpha, eps = spherical_coords(ORIGIN, x, y, z)
    margin = _assert_margin(((r, rho), (a, alpha), (e, eps)))
    for v in (r, a_deg, e_deg, a, e, x, y, z):
        v.setflags(write=False)
    return dict(r=r, a_deg=a_deg, e_deg=e_deg, a=a, e=e, origin=ORIGIN, x=x, y=y, z=z, margin=margin, uniform=not nu)


@functools.lru_cache(maxsize=None)
def node_hit_case():
    """origin, r and z are multiples of 2^-10, the a axis holds 0 and the x axis holds ox: in the column x = ox, atan2(0, dz) = 0 and hypot(dz, 0) = |dz| are
    exact, so the output there is the source node values bit for bit (integer data: the lerps are exact).  z has one pixel before r[0] and one past r[R-1];
    the pixels AT r[0] and r[R-1] are inside.  ``col`` is the column, ``l0`` the node of angle 0, ``rows`` the z indices of the R nodes."""
    q = 1.0 / 1024
    origin = (3 * q, 0.0, -51 * q)
    r = (51 + 6 * np.arange(9.0)) * q
    a_deg = np.array([-30.0, -10.0, 0.0, 15.0, 35.0])
    z = 6 * np.arange(-1.0, 10.0) * q
    x = origin[0] + np.array([-0.02, -0.005, 0.0, 0.01, 0.03])
    a = deg2rad(a_deg)
    rho, alpha = polar_coords(origin, x, z)
    exempt = np.zeros(rho.shape, bool)
    exempt[:, 2] = True
    margin = _assert_margin(((r, rho), (a, alpha)), exempt)
    assert np.array_equal(rho[1:10, 2], r) and (alpha[:, 2] == 0).all()
    for v in (r, a_deg, a, x, z):
        v.setflags(write=False)
    return dict(r=r, a_deg=a_deg, a=a, origin=origin, x=x, z=z, col=2, l0=2, rows=np.arange(1, 10), margin=margin, uniform=True)


def linear_field(c, r, a_rad, e_rad=None):
    """``c0 + c1 r + c2 a (+ c3 e)`` on the source nodes"""
    f = c[0] + c[1] * np.asarray(r)[:, None] + c[2] * np.asarray(a_rad)[None, :]
    if e_rad is not None:
        f = f[:, :, None] + c[3] * np.asarray(e_rad)[None, None, :]
    return f


def data(shape, dtype, seed, zeros=0):
    """random normal data of a numpy dtype (complex: both parts), as the float64 / complex128 values the device sees; ``zeros`` exact zeros planted"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    v = rng.standard_normal(shape)
    if dt.kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    v = v.astype(dt)
    if zeros:
        flat = v.reshape(-1)
        flat[rng.choice(flat.size, size=min(zeros, flat.size), replace=False)] = 0
    return v
