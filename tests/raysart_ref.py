"""SART on the float64 restatement's dense matrix (tests/raypaths_ref.py), in numpy -- a helper module, not a conftest: what ``qups_amd.ray_sart`` is held
against, with and without a device.  Also the ray set and the medium both test files share."""
from __future__ import annotations

import functools

import numpy as np

from tests import raypaths_ref as R


def edge_rays(xg, zg, nt=16, ns=8):
    """``(pa, pb)``, ``2 x (nt nt + ns ns)``: every one of ``nt`` points on the top edge to every one of ``nt`` on the bottom edge, then ``ns`` points on the
    left edge to ``ns`` on the right -- the through-transmission set of a ring or of two facing arrays"""
    xt, zs = np.linspace(xg[0], xg[-1], nt), np.linspace(zg[0], zg[-1], ns)
    a = [(x0, zg[0]) for x0 in xt for _ in xt] + [(xg[0], z0) for z0 in zs for _ in zs]
    b = [(x1, zg[-1]) for _ in xt for x1 in xt] + [(xg[-1], z1) for _ in zs for z1 in zs]
    return np.array(a).T.copy(), np.array(b).T.copy()


def inclusion(xg, zg, c0=1540.0, dc=60.0):
    """the slowness ``X x Z`` of a Gaussian inclusion of ``+dc`` m/s in ``c0`` at the grid's centre, a sixth of the span wide"""
    XX, ZZ = np.meshgrid(xg, zg, indexing="ij")
    xc, zc = 0.5 * (xg[0] + xg[-1]), 0.5 * (zg[0] + zg[-1])
    q = ((XX - xc) / (np.ptp(xg) / 6)) ** 2 + ((ZZ - zc) / (np.ptp(zg) / 6)) ** 2
    return 1.0 / (c0 + dc * np.exp(-0.5 * q))


def sart(A, t, s0, iters, relax=1.0):
    """``(maps, res)``: the iterate after every step (``iters + 1`` vectors, the start first) of ``s <- s + relax C A' R (t - A s)`` with ``R = 1 / row sums``,
    ``C = 1 / column sums`` (0 where a sum is 0), and the R-weighted residual ``sqrt(sum (t - A s)^2 / len)`` of each"""
    ln, col = A.sum(1), A.sum(0)
    with np.errstate(divide="ignore"):
        rinv, cinv = np.where(ln > 0, 1 / ln, 0.0), np.where(col > 0, 1 / col, 0.0)
    s = np.asarray(s0, np.float64).copy()
    maps, res = [s.copy()], []
    for _ in range(iters):
        e = t - A @ s
        res.append(float(np.sqrt(np.sum(e * e * rinv))))
        s = s + relax * cinv * (A.T @ (e * rinv))
        maps.append(s.copy())
    e = t - A @ s
    res.append(float(np.sqrt(np.sum(e * e * rinv))))
    return maps, res


@functools.lru_cache(maxsize=None)
def case(name):
    """grid ``name`` of ``raypaths_ref.grids()``, the edge rays, the dense matrix ``A`` (``J x (X Z)``, node ``ix Z + iz``), the inclusion's arrival times and
    the homogeneous start -- computed once, never modified"""
    xg, zg = R.grids()[name]
    pa, pb = edge_rays(xg, zg)
    A = R.dense_many(xg, zg, pa, pb).reshape(pa.shape[1], -1)
    s_true = inclusion(xg, zg).reshape(-1)
    t = A @ s_true
    s0 = np.full(s_true.shape, 1 / 1540.0)
    for v in (xg, zg, pa, pb, A, s_true, t, s0):
        v.setflags(write=False)
    return dict(xg=xg, zg=zg, pa=pa, pb=pb, A=A, s_true=s_true, t=t, s0=s0, X=xg.size, Z=zg.size)
