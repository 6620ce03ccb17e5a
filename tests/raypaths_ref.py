"""A float64 numpy restatement of the bilinear ray weights, written from the contract in include/qdas.h (the reference's kern/wbilerp.m route: normalise the
ray so that it runs up in x with a slope in [0, 1], list the end points and every crossing with a grid line, sort, integrate each segment in closed form,
undo the normalisation) -- a helper module, not a conftest.  Deliberately NOT the device's parametric walk: the two share the contract only.

Also the closed forms the contract implies, which depend on no restatement: the Liang-Barsky clipped length and the integral of a linear field."""
from __future__ import annotations

import numpy as np


def dense(xg, zg, a, b):
    """the ``X x Z`` sum of the weights of the ray ``a -> b`` (``W[ix, iz]``)"""
    x, z = np.asarray(xg, np.float64), np.asarray(zg, np.float64)
    X, Z = x.size, z.size
    W = np.zeros((X, Z))
    xa, za, xb, zb = (float(v) for v in (a[0], a[1], b[0], b[1]))
    if not np.all(np.isfinite([xa, za, xb, zb])) or (xa == xb and za == zb):
        return W
    with np.errstate(divide="ignore", invalid="ignore"):
        neg = (np.float64(zb - za) / np.float64(xb - xa) < 0) or (np.float64(xb - xa) / np.float64(zb - za) < 0)
    steep = abs(zb - za) > abs(xb - xa)
    rev = (za > zb) if steep else (xa > xb)
    # the normalised frame (u: the axis the ray runs up along; v: the other one, negated when the slope is negative)
    if steep:
        pu, pv, qu, qv, gu, gv = za, xa, zb, xb, z, x
    else:
        pu, pv, qu, qv, gu, gv = xa, za, xb, zb, x, z
    if rev:
        pu, pv, qu, qv = qu, qv, pu, pv
    if neg:
        pv, qv, gv = -pv, -qv, -gv[::-1]
    U, V = gu.size, gv.size
    m = (qv - pv) / (qu - pu)
    pts = [(pu, pv), (qu, qv)] + [(g, pv + m * (g - pu)) for g in gu]
    if qv != pv:
        mi = (qu - pu) / (qv - pv)
        pts += [(pu + mi * (g - pv), g) for g in gv]
    pts = np.array(pts)
    pts = pts[np.argsort(pts[:, 0], kind="stable")]
    if m != 0:
        pts[:, 1] = np.sort(pts[:, 1])
    lo = np.array([max(gu[0], pu), max(gv[0], pv)])
    hi = np.array([min(gu[-1], qu), min(gv[-1], qv)])
    Wn = np.zeros((U, V))
    for p1, p2 in zip(pts[:-1], pts[1:]):
        l = np.hypot(*(p2 - p1))
        if l == 0 or not (np.all(lo <= p1) and np.all(p1 <= hi) and np.all(lo <= p2) and np.all(p2 <= hi)):
            continue
        mid = 0.5 * (p1 + p2)
        iu = int(np.clip(np.searchsorted(gu, mid[0], "right") - 1, 0, U - 2))
        iv = int(np.clip(np.searchsorted(gv, mid[1], "right") - 1, 0, V - 2))
        h = np.array([gu[iu + 1] - gu[iu], gv[iv + 1] - gv[iv]])
        for du in (0, 1):
            for dv in (0, 1):
                q = np.array([gu[iu + du], gv[iv + dv]])
                s = np.where((p1 <= q) & (p2 <= q), 1.0, -1.0)
                ca = 1 + s * (p1 - q) / h
                cb = s * (p1 - p2) / h
                c = ca[0] * ca[1] - (ca[0] * cb[1] + ca[1] * cb[0]) / 2 + cb[0] * cb[1] / 3
                Wn[iu + du, iv + dv] += l * c
    if neg:
        Wn = Wn[:, ::-1]
    return Wn.T.copy() if steep else Wn


def dense_many(xg, zg, pa, pb):
    """``J x X x Z`` for the rays ``pa[:, j] -> pb[:, j]`` (``2 x J`` each; one point broadcasts)"""
    pa, pb = np.asarray(pa, np.float64).reshape(2, -1), np.asarray(pb, np.float64).reshape(2, -1)
    J = max(pa.shape[1], pb.shape[1])
    pa, pb = np.broadcast_to(pa, (2, J)), np.broadcast_to(pb, (2, J))
    return np.stack([dense(xg, zg, pa[:, j], pb[:, j]) for j in range(J)]) if J else np.zeros((0, len(xg), len(zg)))


def clip(xg, zg, a, b):
    """Liang-Barsky: ``(t0, t1)`` of the part of ``a + t (b - a)``, t in [0, 1], inside the grid's box; ``None`` when there is none"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return None
    t0, t1 = 0.0, 1.0
    for p, d, lo, hi in ((a[0], b[0] - a[0], xg[0], xg[-1]), (a[1], b[1] - a[1], zg[0], zg[-1])):
        if d == 0:
            if p < lo or p > hi:
                return None
            continue
        ta, tb = (lo - p) / d, (hi - p) / d
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return (t0, t1) if t1 > t0 else None


def clipped_length(xg, zg, a, b):
    c = clip(xg, zg, a, b)
    return 0.0 if c is None else (c[1] - c[0]) * float(np.hypot(b[0] - a[0], b[1] - a[1]))


def linear_integral(xg, zg, a, b, f0, fx, fz):
    """the line integral of ``f0 + fx x + fz z`` over the clipped ray: its length times the field at its mid point"""
    c = clip(xg, zg, a, b)
    if c is None:
        return 0.0
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    mid = a + 0.5 * (c[0] + c[1]) * (b - a)
    return clipped_length(xg, zg, a, b) * (f0 + fx * mid[0] + fz * mid[1])


# ---------------------------------------------------------------------------------------------------------------- the cases both test files share
def sign_swap_cases():
    """the 32 sign / swap cases of the reference's KernTest.wbilerp_test: grid -5:5 x -4:4, (-4, 1) -> (3, -2), each of the four coordinates with either
    sign, and the same with the two axes swapped"""
    out = []
    for swap in (False, True):
        x, z, e = np.arange(-5.0, 6.0), np.arange(-4.0, 5.0), (-4.0, 1.0, 3.0, -2.0)
        if swap:
            x, z, e = z, x, (e[1], e[0], e[3], e[2])
        for i in range(16):
            s = [-1.0 + 2.0 * ((i >> k) & 1) for k in range(4)]
            out.append((x, z, np.array([s[0] * e[0], s[1] * e[1]]), np.array([s[2] * e[2], s[3] * e[3]])))
    return out


def grids():
    rng = np.random.default_rng(11)
    nx = np.cumsum(rng.uniform(0.5, 1.5, 33))
    nz = np.cumsum(rng.uniform(0.5, 1.5, 41))
    return {
        "2x2": (np.array([-1.0, 2.0]), np.array([0.5, 1.75])),
        "11x9": (np.arange(-5.0, 6.0), np.arange(-4.0, 5.0)),
        "33x41": (1e-3 * (nx - nx.mean()), 1e-3 * nz),
        "2x65": (np.array([0.0, 3e-3]), 1e-3 * np.linspace(0, 20, 65)),
        "65x2": (1e-3 * np.linspace(-10, 10, 65), np.array([1e-3, 2.5e-3])),
    }


def rays(xg, zg, seed=5, nrand=40):
    """``(pa, pb)``, ``2 x J`` each: random rays with end points up to a quarter of the span outside the grid; vertical, horizontal, on a grid line, on the
    first and last row / column; node to node; end points on the border and in the corners; rays that miss the grid; zero length; NaN and Inf coordinates"""
    rng = np.random.default_rng(seed)
    X, Z = xg.size, zg.size
    sx, sz = xg[-1] - xg[0], zg[-1] - zg[0]
    A, B = [], []

    def add(a, b):
        A.append(np.array(a, np.float64))
        B.append(np.array(b, np.float64))

    def rnd(out=0.25):
        return np.array([rng.uniform(xg[0] - out * sx, xg[-1] + out * sx), rng.uniform(zg[0] - out * sz, zg[-1] + out * sz)])

    for _ in range(nrand):
        add(rnd(), rnd())
    for _ in range(nrand // 4):
        add(rnd(0.0), rnd(0.0))                                           # wholly inside
    for _ in range(4):
        p, q = rnd(), rnd()
        add(p, (p[0], q[1]))                                              # vertical
        add(p, (q[0], p[1]))                                              # horizontal
    for i in sorted({0, X // 2, X - 1}):                                  # along x-grid lines, first and last column included
        add((xg[i], zg[0] - 0.1 * sz), (xg[i], zg[-1] + 0.1 * sz))
        add((xg[i], zg[-1]), (xg[i], zg[0]))
        add((xg[i], zg[Z // 2]), (xg[i], 0.5 * (zg[0] + zg[1])))
    for k in sorted({0, Z // 2, Z - 1}):                                  # along z-grid lines, first and last row included
        add((xg[0] - 0.1 * sx, zg[k]), (xg[-1] + 0.1 * sx, zg[k]))
        add((xg[-1], zg[k]), (xg[0], zg[k]))
        add((xg[X // 2], zg[k]), (0.5 * (xg[0] + xg[1]), zg[k]))
    for _ in range(8):                                                    # node to node
        add((xg[rng.integers(X)], zg[rng.integers(Z)]), (xg[rng.integers(X)], zg[rng.integers(Z)]))
    add((xg[0], zg[0]), (xg[-1], zg[-1]))                                 # corner to corner, both diagonals
    add((xg[-1], zg[0]), (xg[0], zg[-1]))
    add((xg[0], zg[0]), (xg[0], zg[-1]))                                  # along the border
    add((xg[0], zg[-1]), (xg[-1], zg[-1]))
    add((xg[0], 0.5 * (zg[0] + zg[-1])), (xg[-1], zg[-1]))                # border to corner
    add((xg[-1], zg[-1]), rnd(0.0))                                       # corner to inside
    add((xg[0] - 0.2 * sx, zg[0] - 0.1 * sz), (xg[0] + 0.1 * sx, zg[0] - 0.01 * sz))      # misses the grid
    add((xg[0] - 0.2 * sx, zg[0]), (xg[0] - 0.1 * sx, zg[-1]))
    add((xg[-1] + 0.1 * sx, zg[0] - sz), (xg[-1] + 0.1 * sx, zg[-1] + sz))
    add((xg[0] - 0.1 * sx, zg[0] + 0.1 * sz), (xg[0] + 0.05 * sx, zg[0] - 0.1 * sz))       # cuts a corner
    add((xg[0] - 0.1 * sx, zg[0] - 0.1 * sz), (xg[0], zg[0]))                              # touches a corner from outside
    p = rnd(0.0)
    add(p, p)                                                             # zero length
    add((xg[1], zg[1]), (xg[1], zg[1]))
    for bad in (np.nan, np.inf, -np.inf):
        add((bad, zg[0]), rnd(0.0))
        add(rnd(0.0), (xg[0], bad))
    add((np.nan, np.nan), (np.nan, np.nan))
    add((-np.inf, zg[0]), (np.inf, zg[0]))
    return np.array(A).T.copy(), np.array(B).T.copy()
