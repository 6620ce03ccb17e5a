"""The restatement of qdas_fdtd3 in numpy, written once for float64 and float32 (``dtype``): the scheme of include/qdas.h with whole-array slices, the 3-D
twin of tests/fdtd_ref.py (whose ``dplus`` / ``dminus`` / ``pml`` / ``xcorr_lag`` / ``tolerance`` it uses as they are: they are axis-generic).

Grid ``Z x X x Y`` nodes of spacing ``h`` plus ``P`` PML cells on all six faces (``c``, ``rho`` extended by edge replication); ``p``, ``rz``, ``rx``, ``ry`` at
``(i, j, k)``, ``uz`` at ``(i + 1/2, j, k)``, ``ux`` at ``(i, j + 1/2, k)``, ``uy`` at ``(i, j, k + 1/2)``; the staggered density of an axis is the mean of the two
neighbours along it with the last one kept.

    1. u_a <- A+_a (A+_a u_a - (dt / rho_sg,a) D+_a p)       2. u_a[src] += n_a s[n, m, v] 2 c[src] dt / h
    3. r_a <- A_a (A_a r_a - dt rho D-_a u_a)                 4. p = c^2 ((rz + rx) + ry)             5. rec[n, j, v] = p[sensor j]

Arrays here are ``V x Z' x X' x Y'`` (z is axis 1); the tables are made in float64 and rounded once to ``dtype``, as the device's are."""
import os
import re

import numpy as np

from tests.fdtd_ref import COEFS, dminus, dplus, pml, tolerance, xcorr_lag  # noqa: F401  (re-exported: the one rule, the one lag)

AXES = ("z", "x", "y")
STATES = ("p", "uz", "ux", "uy", "rz", "rx", "ry")


def limit(R):
    return 1.0 / (np.sqrt(3.0) * sum(abs(a) for a in COEFS[R]))


def tables(c, rho, h, dt, P):
    c, rho = np.asarray(c, np.float64), np.asarray(rho, np.float64)
    ce, re_ = np.pad(c, P, mode="edge"), np.pad(rho, P, mode="edge")
    sg = []
    for ax in range(3):
        a = re_.copy()
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(None, -1), slice(1, None)
        a[tuple(lo)] = (re_[tuple(lo)] + re_[tuple(hi)]) / 2
        sg.append(a)
    A = [pml(ce.shape[ax], P, c.max(), h, dt) for ax in range(3)]
    return ce, re_, sg, A


def simulate(c, rho, h, dt, P, R, src, nrm, s, sen, Nt, dtype=np.float64, snapshots=False):
    """``c``, ``rho``: ``Z x X x Y``; ``src``, ``sen``: ``(iz, ix, iy)`` integer arrays of INTERIOR nodes; ``nrm``: ``3 x M`` rows ``(nz, nx, ny)``; ``s``:
    ``T' x M x V``.  Returns ``(rec Nt x N x V, state dict of V x Z' x X' x Y' arrays[, snapshots Nt x Z x X x Y x V of the interior p])`` in ``dtype``."""
    dtype = np.dtype(dtype).type
    ce, re_, sg, A = tables(c, rho, h, dt, P)
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    c2, rr = f(ce * ce), f(re_)
    dtr = [f(dt / g) for g in sg]
    shape = lambda ax: tuple(-1 if d == ax + 1 else 1 for d in range(4))
    An = [f(A[ax][0]).reshape(shape(ax)) for ax in range(3)]
    As = [f(A[ax][1]).reshape(shape(ax)) for ax in range(3)]
    inv_h, dt_h = dtype(1.0 / h), dtype(dt / h)
    s = f(s)
    Ts, M, V = s.shape
    si = tuple(np.asarray(a, np.int64) + P for a in src)
    ni = tuple(np.asarray(a, np.int64) + P for a in sen)
    nrm = np.asarray(nrm, np.float64).reshape(3, -1)
    w = [f(nrm[ax] * 2.0 * ce[si] * dt / h) if M else f(np.zeros(0)) for ax in range(3)]
    N3 = ce.shape
    p = np.zeros((V,) + N3, dtype)
    u = [np.zeros((V,) + N3, dtype) for _ in range(3)]
    r = [np.zeros((V,) + N3, dtype) for _ in range(3)]
    rec = np.zeros((Nt, len(ni[0]), V), dtype)
    inner = (slice(None),) + tuple(slice(P, n - P) for n in N3)
    snap = np.zeros((Nt,) + tuple(n - 2 * P for n in N3) + (V,), dtype) if snapshots else None
    vi = lambda idx: (slice(None),) + idx
    for n in range(Nt):
        for ax in range(3):
            u[ax] = As[ax] * (As[ax] * u[ax] - (dtr[ax] * inv_h)[None] * dplus(p, ax + 1, R, dtype))
            if n < Ts and M:
                u[ax][vi(si)] += (w[ax][:, None] * s[n]).T
        for ax in range(3):
            r[ax] = An[ax] * (An[ax] * r[ax] - (dt_h * rr)[None] * dminus(u[ax], ax + 1, R, dtype))
        p = c2[None] * ((r[0] + r[1]) + r[2])
        rec[n] = p[vi(ni)].T
        if snapshots:
            snap[n] = np.moveaxis(p[inner], 0, -1)
    state = dict(p=p, uz=u[0], ux=u[1], uy=u[2], rz=r[0], rx=r[1], ry=r[2])
    return (rec, state, snap) if snapshots else (rec, state)


# ---------------------------------------------------------------------------------------------------------------- the parity cases (host core and GPU)
def _brick():
    """the kernel's brick over the EXTENDED grid (z along lanes), from the header"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qdas.h")) as f:
        header = f.read()
    return tuple(int(re.search(rf"#define QDAS_FDTD3_{n} (\d+)\b", header).group(1)) for n in ("TZ", "TX", "TY"))


TZ, TX, TY = _brick()
# (Z, X, Y, P), by the extended extents Nz x Nx x Ny:
#   (a) no extent a multiple of its brick edge, more than one brick in x and in y (P = 3: 43 x (TX + 11) x (TY + 9))
#   (b) P = 0 and exactly 64 x 2 TX x 2 TY
#   (c), (d), (e) three interior nodes with P = 4 (extent 11, thinner than the halo of R = 4) in z, x, y in turn, the other two one past a brick edge (65, 2 TX + 1, 2 TY + 1)
#   (f) every extent one node past a brick edge (P = 2)
GRIDS = [(37, TX + 5, TY + 3, 3), (64, 2 * TX, 2 * TY, 0), (3, 2 * TX - 7, 2 * TY - 7, 4), (57, 3, 2 * TY - 7, 4), (57, 2 * TX - 7, 3, 4), (61, TX - 3, TY - 3, 2)]
H, NT, TS = 1e-4, 100, 40


def smooth_map(Z, X, Y, lo, hi, seed):
    """a smooth random map with min ``lo`` and max ``hi``: a few low cosines (the 3-D twin of fdtd_ref.smooth_map)"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*(np.arange(n) / max(n - 1, 1) for n in (Z, X, Y)), indexing="ij")
    u = sum(rng.standard_normal() * np.cos(np.pi * (a * g[0] + b * g[1] + d * g[2]) + rng.uniform(0, 6)) for a in range(3) for b in range(3) for d in range(2))
    u = (u - u.min()) / max(u.max() - u.min(), 1e-30)
    return lo + (hi - lo) * u


def _pick(Z, X, Y, P):
    """sources and sensors: the first and the last interior node, a brick corner, a brick's last row, last column and last plane (where the grid reaches one);
    the last interior node is both a source and a sensor"""
    def first(n, mod, want, default):
        return next((k for k in range(n) if (k + P) % mod == want), default)
    corner = (first(Z, TZ, 0, 0), first(X, TX, 0, X // 2), first(Y, TY, 0, Y // 2))
    last = (first(Z, TZ, TZ - 1, Z - 1), first(X, TX, TX - 1, X // 2), first(Y, TY, TY - 1, Y // 2))
    uniq = lambda pts: list(dict.fromkeys(pts))
    src = uniq([(0, 0, 0), (Z - 1, X - 1, Y - 1), corner, last])
    sen = uniq([(Z - 1, X - 1, Y - 1), (corner[0], min(corner[1] + 1, X - 1), corner[2]), (Z // 2, X // 2, Y // 2), (0, X - 1, 0), (last[0], X // 2, last[2]),
                (Z // 2, last[1], Y - 1)])
    return src, sen


def parity_case(Z, X, Y, P, V, seed=0):
    """the inputs of one parity case (float64): a heterogeneous medium with c_max / c_min = 1.2, a source table with different delays and apodization per
    pulse, oblique normals, dt at 0.3 of c_max dt / h (inside the limit of every order)"""
    rng = np.random.default_rng(seed + 7 * Z + 3 * X + Y)
    c = smooth_map(Z, X, Y, 1400.0, 1680.0, seed + Z)
    rho = smooth_map(Z, X, Y, 900.0, 1100.0, seed + X + 1)
    dt = 0.3 * H / c.max()
    src, sen = _pick(Z, X, Y, P)
    M = len(src)
    nrm = np.array([[1.0, 0.0, 0.6, -0.48][:M], [0.0, 0.6, 0.64, 0.6][:M], [0.0, -0.8, 0.48, 0.64][:M]])
    dl = rng.uniform(0, 8, (M, V))
    ap = rng.uniform(0.5, 1.5, (M, V))
    n = np.arange(TS, dtype=np.float64)[:, None, None]
    s = ap[None] * np.sin(2 * np.pi * (n - dl[None] - 12) / 16.0) * np.exp(-(((n - dl[None] - 12) / 6.0) ** 2))
    z, x, y = np.arange(Z) * H, (np.arange(X) - (X - 1) / 2) * H, (np.arange(Y) - (Y - 1) / 2) * H
    cols = lambda pts: tuple(np.array([q[a] for q in pts]) for a in range(3))
    return dict(c=c, rho=rho, h=H, dt=dt, P=P, src=cols(src), sen=cols(sen), nrm=nrm, s=s, Nt=NT, z=z, x=x, y=y)


def swap_xy(cs):
    """the case with x and y exchanged: medium, nodes, normals and axes"""
    sw = lambda t: (t[0], t[2], t[1])
    return dict(cs, c=np.ascontiguousarray(cs["c"].transpose(0, 2, 1)), rho=np.ascontiguousarray(cs["rho"].transpose(0, 2, 1)), src=sw(cs["src"]), sen=sw(cs["sen"]),
                nrm=cs["nrm"][[0, 2, 1]], x=cs["y"], y=cs["x"])


def run_case(cs, R, dtype=np.float64, **kw):
    return simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], cs["P"], R, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], dtype, **kw)


_REFS = {}


def parity_refs(Z, X, Y, P, R, V):
    """``(case, ref64, ref32, d32)``, computed once: ``ref* = (rec, state)`` of the restatement, ``d32[name] = max|ref32 - ref64| / max|ref64|`` per output"""
    key = (Z, X, Y, P, R, V)
    if key not in _REFS:
        cs = parity_case(Z, X, Y, P, V)
        r64, r32 = run_case(cs, R, np.float64), run_case(cs, R, np.float32)
        d32 = {"rec": np.abs(r32[0] - r64[0]).max() / np.abs(r64[0]).max()}
        for k in r64[1]:
            d32[k] = np.abs(r32[1][k] - r64[1][k]).max() / np.abs(r64[1][k]).max()
        for a in (r64[0], r32[0], *r64[1].values(), *r32[1].values()):
            a.setflags(write=False)
        _REFS[key] = (cs, r64, r32, d32)
    return _REFS[key]
