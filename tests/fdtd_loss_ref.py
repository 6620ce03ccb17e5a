"""The restatement of qdas_fdtd_lossy in numpy, float64 and float32: tests/fdtd_ref.py's step with step 4 replaced (include/qdas.h states it).

    rn = rz + rx                                                         (after step 3)
    relaxation (L >= 1):  e_l <- e_l + E_l (rn - e_l),   p = c2 (rn + kap sum_l g_l (rn - e_l))      (the updated e_l, l ascending)
    Stokes (L = 0):       p = c2 (rn + kap (rn - ro)),    ro = rz + rx before step 3                 (kap holds mud = 2 c a / dt)
    and p = c2 rn exactly where kap is 0.

``kap`` is a ``Z x X`` map on the interior grid, extended into the PML by edge replication like ``c`` and ``rho``.  Arrays are ``V x Z' x X'``, the memory
variables ``V x L x Z' x X'``.  The scalars ``g``, ``E`` are made in float64 and rounded once to ``dtype``, as the device's are."""
import numpy as np

from tests.fdtd_ref import GRIDS, dminus, dplus, parity_case, tables, tolerance  # noqa: F401  (GRIDS, tolerance: for the tests that import this module)


def simulate(c, rho, h, dt, P, R, src, nrm, s, sen, Nt, kap, g=(), E=(), dtype=np.float64):
    """tests/fdtd_ref.simulate with absorption.  ``g``, ``E``: the ``L`` mechanisms (``L = 0``: Stokes).  Returns ``(rec Nt x N x V, states)`` with the five
    states ``V x Z' x X'`` and ``e``: ``V x L x Z' x X'``."""
    dtype = np.dtype(dtype).type
    ce, re, sgz, sgx, az, azs, ax, axs = tables(c, rho, h, dt, P)
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    c2, rr, dtrz, dtrx = f(ce * ce), f(re), f(dt / sgz), f(dt / sgx)
    kp = f(np.pad(np.asarray(kap, np.float64), P, mode="edge"))[None]
    az, azs, ax, axs = f(az)[None, :, None], f(azs)[None, :, None], f(ax)[None, None, :], f(axs)[None, None, :]
    inv_h, dt_h = dtype(1.0 / h), dtype(dt / h)
    g, E = f(g).reshape(-1), f(E).reshape(-1)
    L = g.size
    assert E.size == L
    s = f(s)
    Ts, M, V = s.shape
    siz, six = (np.asarray(a, np.int64) + P for a in src)
    niz, nix = (np.asarray(a, np.int64) + P for a in sen)
    nrm = np.asarray(nrm, np.float64).reshape(2, -1)
    wz = f(nrm[0] * 2.0 * ce[siz, six] * dt / h) if M else f(np.zeros(0))
    wx = f(nrm[1] * 2.0 * ce[siz, six] * dt / h) if M else f(np.zeros(0))
    Nz, Nx = ce.shape
    p, uz, ux, rz, rx = (np.zeros((V, Nz, Nx), dtype) for _ in range(5))
    e = np.zeros((V, L, Nz, Nx), dtype)
    rec = np.zeros((Nt, len(niz), V), dtype)
    for n in range(Nt):
        uz = azs * (azs * uz - (dtrz * inv_h)[None] * dplus(p, 1, R, dtype))
        ux = axs * (axs * ux - (dtrx * inv_h)[None] * dplus(p, 2, R, dtype))
        if n < Ts and M:
            uz[:, siz, six] += (wz[:, None] * s[n]).T
            ux[:, siz, six] += (wx[:, None] * s[n]).T
        ro = rz + rx
        rz = az * (az * rz - (dt_h * rr)[None] * dminus(uz, 1, R, dtype))
        rx = ax * (ax * rx - (dt_h * rr)[None] * dminus(ux, 2, R, dtype))
        rn = rz + rx
        if L == 0:
            acc = rn - ro
        else:
            acc = np.zeros_like(rn)
            for l in range(L):
                e[:, l] = e[:, l] + E[l] * (rn - e[:, l])
                acc = acc + g[l] * (rn - e[:, l])
        with np.errstate(invalid="ignore"):
            p = c2[None] * np.where(kp != 0, rn + kp * acc, rn)
        rec[n] = p[:, niz, nix].T
    return rec, dict(p=p, uz=uz, ux=ux, rz=rz, rx=rx, e=e)


# ---------------------------------------------------------------------------------------------------------------- the parity cases (host core and GPU)
def loss_case(Z, X, L, dt, seed=0):
    """the loss block of a parity case: a smooth ``kap`` map that is 0 in one corner region and reaches a strong loss elsewhere, and ``L`` mechanisms with
    ``E`` spread over two decades.  Relaxation: ``kap sum g <= 0.2`` (the unrelaxed speed stays below 1.1 c: 0.3 x 1.1 is inside the limit of every order);
    Stokes: ``mud <= 0.25``."""
    from tests.fdtd_ref import smooth_map
    u = smooth_map(Z, X, -0.25, 1.0, seed + 3 * Z + X)
    kap = np.maximum(u, 0.0) * (0.25 if L == 0 else 0.2)
    g = np.array([0.5, 0.3, 0.15, 0.05][:L]) / max(sum([0.5, 0.3, 0.15, 0.05][:L]), 1e-30)
    E = np.array([0.3, 0.08, 0.02, 0.004][:L])
    return dict(kap=kap, g=g, E=E)


_REFS = {}


def parity_refs(Z, X, P, R, V, L):
    """``(case, loss, ref64, ref32, d32)``, computed once and read-only: ``d32[name] = max|ref32 - ref64| / max|ref64|`` for the record, the five states and
    ``e`` (0 for an output the reference leaves empty or all zero: the tolerance is then its floor)"""
    key = (Z, X, P, R, V, L)
    if key not in _REFS:
        cs = parity_case(Z, X, P, V)
        ls = loss_case(Z, X, L, cs["dt"])
        run = lambda dt_: simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, R, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], ls["kap"], ls["g"], ls["E"], dt_)
        r64, r32 = run(np.float64), run(np.float32)
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max()) if b.size and np.abs(b).max() > 0 else 0.0
        d32 = {"rec": rel(r32[0], r64[0])}
        d32.update({k: rel(r32[1][k], r64[1][k]) for k in r64[1]})
        for a in (r64[0], r32[0], *r64[1].values(), *r32[1].values()):
            a.setflags(write=False)
        _REFS[key] = (cs, ls, r64, r32, d32)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------- the physics case
C0, RHO0, FC, YS = 1540.0, 1000.0, 5e6, ((1.1, 3), (1.5, 3), (2.0, 0))
ALPHA_DB = 0.75                     # dB/(MHz^y cm)
BAND = (3e6, 7e6)


def physics_setup():
    """homogeneous 1540 m/s, h = lambda / 6 at 5 MHz, a point source and two sensors 10 mm apart in depth on a narrow grid, PML 20; c dt / h = 0.2"""
    h = C0 / FC / 6.0
    d_nodes = int(round(10e-3 / h))
    Z, X = d_nodes + 30, 21
    dt = 0.2 * h / C0
    t = np.arange(0, 1.6e-6, dt)
    tc = 0.8e-6
    w = np.sin(2 * np.pi * FC * (t - tc)) * np.exp(-((t - tc) / 0.16e-6) ** 2)          # -6 dB two-sided bandwidth about 3 .. 7 MHz
    src = (np.array([2]), np.array([X // 2]))
    sen = (np.array([15, 15 + d_nodes]), np.array([X // 2, X // 2]))
    Nt = int((Z * h / C0 + 2.2e-6) / dt)
    return dict(h=h, dt=dt, Z=Z, X=X, P=20, R=4, src=src, sen=sen, nrm=np.array([[1.0], [0.0]]), s=w[:, None, None], Nt=Nt, d=d_nodes * h)


def measured_alpha(rec_lossy, rec_lossless, dt, d, freqs):
    """``-ln(|P2 / P1|_lossy / |P2 / P1|_lossless) / d`` at ``freqs`` (Np / m), from the spectra of the two sensors' records (``Nt x 2``)"""
    n = 8 * rec_lossy.shape[0]
    f = np.fft.rfftfreq(n, dt)
    spec = lambda r: np.abs(np.fft.rfft(np.asarray(r, np.float64), n, axis=0))
    a, b = spec(rec_lossy), spec(rec_lossless)
    ratio = (a[:, 1] / a[:, 0]) / (b[:, 1] / b[:, 0])
    return np.interp(freqs, f, -np.log(ratio) / d)
