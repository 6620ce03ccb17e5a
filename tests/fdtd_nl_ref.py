"""The restatement of qdas_fdtd_nonlinear in numpy, float64 and float32: tests/fdtd_loss_ref.py's step with steps 3 and 4 replaced (include/qdas.h states it).

    ro = rz + rx                                                          (before step 3)
    3'. r_a <- A_a (A_a r_a - (dt / h) (rho + K ro) h D-_a u_a)           K = 2 (the convective term) or 0
    rn = rz + rx                                                          (after it)
    4'. p = c2 (lin + bq rn^2),   lin = rn + [the absorption term of tests/fdtd_loss_ref.py, if a loss map is given]
    and p = c2 lin exactly where bq is 0.

``bq = BoA / (2 rho)`` is a ``Z x X`` map on the interior grid, extended into the PML by edge replication like ``c`` and ``rho``.  With ``K = 0`` and a zero
``bq`` every value is tests/fdtd_ref.py's (``kap=None``) or tests/fdtd_loss_ref.py's, bit for bit.  ``lines=True`` sets ``dt / rho_sgx`` to 0, as the physics
tests do with the device's tables: ``ux`` and ``rx`` stay 0 and every column is a 1-D line of its own (the x half of the step is then skipped here)."""
import math

import numpy as np

from tests.fdtd_loss_ref import loss_case
from tests.fdtd_ref import GRIDS, dminus, dplus, parity_case, smooth_map, tables, tolerance  # noqa: F401  (GRIDS, tolerance: for the tests that import this module)


def simulate(c, rho, h, dt, P, R, src, nrm, s, sen, Nt, bq, K=2.0, kap=None, g=(), E=(), dtype=np.float64, lines=False):
    """tests/fdtd_loss_ref.simulate with nonlinearity.  ``kap=None``: no absorption; else ``g``, ``E``: the ``L`` mechanisms (``L = 0``: Stokes).  Returns
    ``(rec Nt x N x V, states)`` with the five states ``V x Z' x X'``, ``e``: ``V x L x Z' x X'`` and ``mach``: the largest ``|u| / c`` any node saw."""
    dtype = np.dtype(dtype).type
    ce, re, sgz, sgx, az, azs, ax, axs = tables(c, rho, h, dt, P)
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    c2, rr, dtrz, dtrx = f(ce * ce), f(re), f(dt / sgz), f(dt / sgx)
    ext = lambda m: f(np.pad(np.broadcast_to(np.asarray(m, np.float64), np.shape(c)), P, mode="edge"))[None]
    bqe = ext(bq)
    kp = None if kap is None else ext(kap)
    az, azs, ax, axs = f(az)[None, :, None], f(azs)[None, :, None], f(ax)[None, None, :], f(axs)[None, None, :]
    inv_h, dt_h, K = dtype(1.0 / h), dtype(dt / h), dtype(K)
    g, E = f(g).reshape(-1), f(E).reshape(-1)
    L = g.size
    assert E.size == L and (kp is not None or L == 0)
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
    inv_c = 1.0 / ce
    mach = 0.0
    for n in range(Nt):
        uz = azs * (azs * uz - (dtrz * inv_h)[None] * dplus(p, 1, R, dtype))
        if not lines:
            ux = axs * (axs * ux - (dtrx * inv_h)[None] * dplus(p, 2, R, dtype))
        if n < Ts and M:
            uz[:, siz, six] += (wz[:, None] * s[n]).T
            if not lines:
                ux[:, siz, six] += (wx[:, None] * s[n]).T
        with np.errstate(invalid="ignore"):
            mach = max(mach, float(np.nanmax(np.maximum(np.abs(uz), np.abs(ux)) * inv_c[None])))
        ro = rz + rx
        w = dt_h * (rr[None] + K * ro)
        rz = az * (az * rz - w * dminus(uz, 1, R, dtype))
        if not lines:
            rx = ax * (ax * rx - w * dminus(ux, 2, R, dtype))
        rn = rz + rx
        lin = rn
        if kp is not None:
            if L == 0:
                acc = rn - ro
            else:
                acc = np.zeros_like(rn)
                for l in range(L):
                    e[:, l] = e[:, l] + E[l] * (rn - e[:, l])
                    acc = acc + g[l] * (rn - e[:, l])
            with np.errstate(invalid="ignore"):
                lin = np.where(kp != 0, rn + kp * acc, rn)
        with np.errstate(invalid="ignore"):
            p = c2[None] * np.where(bqe != 0, lin + bqe * (rn * rn), lin)
        rec[n] = p[:, niz, nix].T
    return rec, dict(p=p, uz=uz, ux=ux, rz=rz, rx=rx, e=e, mach=mach)


# ---------------------------------------------------------------------------------------------------------------- the parity cases (host core and GPU)
MACH = 4e-3                         # what the source tables of the parity cases are scaled to: max|u| / c of the LINEAR run (the tests hold 1e-3 .. 1e-2)
BOA_MAX = 10.0
LOSSES = (None, 0, 3)               # no absorption, Stokes, three relaxation mechanisms

_CASES = {}


def nl_case(Z, X, P, V):
    """tests/fdtd_ref.parity_case driven hard: the source table scaled so that the largest ``|u| / c`` of the linear lossless run (order 8, float64) is
    ``MACH``, and a smooth ``BoA`` map that is 0 over part of the grid and reaches ``BOA_MAX``.  Computed once, read-only."""
    key = (Z, X, P, V)
    if key not in _CASES:
        cs = dict(parity_case(Z, X, P, V))
        _, st = simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, 4, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], 0.0, K=0.0)
        cs["s"] = cs["s"] * (MACH / st["mach"])
        cs["BoA"] = np.maximum(smooth_map(Z, X, -0.25 * BOA_MAX, BOA_MAX, 11 + 5 * Z + X), 0.0)
        cs["bq"] = cs["BoA"] / (2.0 * cs["rho"])
        for a in (cs["BoA"], cs["bq"]):
            a.setflags(write=False)
        _CASES[key] = cs
    return _CASES[key]


_REFS = {}


def parity_refs(Z, X, P, R, V, L, K=2.0):
    """``(case, loss, ref64, ref32, d32)``, computed once and read-only, as tests/fdtd_loss_ref.parity_refs; ``L``: an entry of ``LOSSES`` (``loss`` is None
    without absorption).  ``ref64[1]["mach"]`` is the largest ``|u| / c`` of the float64 run."""
    key = (Z, X, P, R, V, L, K)
    if key not in _REFS:
        cs = nl_case(Z, X, P, V)
        ls = None if L is None else loss_case(Z, X, L, cs["dt"])
        kw = {} if ls is None else dict(kap=ls["kap"], g=ls["g"], E=ls["E"])
        run = lambda dt_: simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, R, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], cs["bq"], K=K, dtype=dt_, **kw)
        r64, r32 = run(np.float64), run(np.float32)
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max()) if b.size and np.abs(b).max() > 0 else 0.0
        d32 = {"rec": rel(r32[0], r64[0])}
        d32.update({k: rel(r32[1][k], r64[1][k]) for k in r64[1] if k != "mach"})
        for a in (r64[0], r32[0], *r64[1].values(), *r32[1].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[key] = (cs, ls, r64, r32, d32)
    return _REFS[key]


_LINEAR = {}


def linear_record(Z, X, P, R, V, L):
    """the float64 record of the same case (the same scaled sources) WITHOUT the nonlinear terms: ``K = 0`` and ``bq = 0``"""
    key = (Z, X, P, R, V, L)
    if key not in _LINEAR:
        cs = nl_case(Z, X, P, V)
        ls = None if L is None else loss_case(Z, X, L, cs["dt"])
        kw = {} if ls is None else dict(kap=ls["kap"], g=ls["g"], E=ls["E"])
        rec, _ = simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, R, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], 0.0, K=0.0, **kw)
        rec.setflags(write=False)
        _LINEAR[key] = rec
    return _LINEAR[key]


# ---------------------------------------------------------------------------------------------------------------- the physics case: Fubini
C0, RHO0, FC, BOA, P0 = 1500.0, 1000.0, 2.5e6, 6.0, 0.5e6
PPW, CFL, CYCLES, RAMP, WINDOW = 16, 0.2, 16, 3, 8          # points per wavelength, c dt / h, cycles of the burst, of each cosine ramp, of the harmonic window
SENSORS = (2, 10, 20, 30)                                   # wavelengths from the source
SRC_NODE = 4
# the three columns that carry a line each (interior x indices) and what they hold
COLUMNS = (0, 2)


def physics_setup():
    """homogeneous 1500 m/s, 1000 kg/m^3, h = lambda / 16 at 2.5 MHz, c dt / h = 0.2, order 8, PML 20; lines of about 60 wavelengths along z, one per column of
    ``COLUMNS`` (with ``dt / rho_sgx = 0`` the columns do not talk): a source at node ``SRC_NODE`` that radiates a 16-cycle burst (3-cycle cosine ramps) of
    ``v0 = P0 / (rho c)`` = 0.333 m/s, i.e. 0.5 MPa, and sensors 2, 10, 20 and 30 wavelengths further on.  Column 0 holds ``B/A = 6``, column 2 ``B/A = 0``."""
    h = C0 / FC / PPW
    dt = CFL * h / C0
    Z, X = 60 * PPW, 3
    spp = int(round(PPW / CFL))                                   # steps per period: 80
    n = np.arange(CYCLES * spp, dtype=np.float64)
    env = np.minimum(1.0, np.minimum(n, n[-1] - n) / (RAMP * spp))
    env = 0.5 - 0.5 * np.cos(np.pi * env)
    v0 = P0 / (RHO0 * C0)
    w = v0 * env * np.sin(2 * np.pi * n / spp)
    M = len(COLUMNS)
    src = (np.full(M, SRC_NODE), np.array(COLUMNS))
    sen = (np.array([SRC_NODE + k * PPW for _ in COLUMNS for k in SENSORS]), np.array([col for col in COLUMNS for _ in SENSORS]))
    BoA = np.zeros((Z, X))
    BoA[:, COLUMNS[0]] = BOA
    Nt = (SENSORS[-1] + CYCLES // 2 + WINDOW // 2 + 1) * spp
    return dict(h=h, dt=dt, Z=Z, X=X, P=20, R=4, src=src, sen=sen, nrm=np.stack([np.ones(M), np.zeros(M)]), s=np.repeat(w[:, None, None], M, 1), Nt=Nt, spp=spp,
                v0=v0, BoA=BoA, c=np.full((Z, X), C0), rho=np.full((Z, X), RHO0))


def _bessel(n, x):
    """``J_n(x)`` from its power series (small arguments only)"""
    return sum((-1.0) ** m / (math.factorial(m) * math.factorial(m + n)) * (x / 2.0) ** (2 * m + n) for m in range(12))


def fubini_ratio(beta, v0, wavelengths):
    """the second harmonic over the fundamental of a plane wave at ``wavelengths`` from its source, ``B2 / B1`` with ``Bn = 2 Jn(n sigma) / (n sigma)``,
    ``sigma = beta (v0 / c) 2 pi wavelengths``"""
    sigma = beta * (v0 / C0) * 2.0 * math.pi * wavelengths
    return (2.0 * _bessel(2, 2.0 * sigma) / (2.0 * sigma)) / (2.0 * _bessel(1, sigma) / sigma)


def harmonic_ratio(trace, spp, wavelengths):
    """``|P2| / |P1|`` of one sensor's record: the DFT at ``fc`` and ``2 fc`` over the central ``WINDOW`` cycles of the burst (a whole number of periods, so a
    rectangular window keeps the two lines apart); the burst's centre arrives ``CYCLES / 2 + wavelengths`` periods after the first step"""
    trace = np.asarray(trace, np.float64)
    n0 = int(round((CYCLES / 2.0 + wavelengths - WINDOW / 2.0) * spp))
    seg = trace[n0:n0 + WINDOW * spp]
    assert seg.size == WINDOW * spp
    ph = 2.0 * np.pi * np.arange(seg.size) / spp
    return float(abs(np.sum(seg * np.exp(-2j * ph))) / abs(np.sum(seg * np.exp(-1j * ph))))


def fubini_deviations(rec, spp, v0, betas):
    """the relative deviations of the measured second-harmonic ratio from Fubini's, ``len(COLUMNS) x len(SENSORS)``; ``betas``: one per column"""
    out = np.zeros((len(COLUMNS), len(SENSORS)))
    for a, beta in enumerate(betas):
        for b, wl in enumerate(SENSORS):
            out[a, b] = harmonic_ratio(rec[:, a * len(SENSORS) + b], spp, wl) / fubini_ratio(beta, v0, wl) - 1.0
    return out


# ---------------------------------------------------------------------------------------------------------------- the end-to-end case: tissue harmonic imaging
E2E = dict(H=0.05e-3, C0=1500.0, RHO0=1000.0, FC=2.5e6, FS=20e6, Z=280, X=120, SCAT=(slice(239, 241), slice(59, 61)), BOA=6.0, ALPHA=0.5, AMP=6.0)


def e2e_setup():
    """a plane wave of 2.5 MHz from 16 elements at 0.3 mm pitch into ``B/A = 6``, 0.5 dB/(MHz^1.01 cm) on a 0.05 mm grid of 280 x 120 nodes (12 points per
    wavelength, 6 at the second harmonic), a density scatterer (rho x 2 over 0.1 mm) at 12 mm; the waveform is a Gaussian pulse of 6 m/s at each element's
    node (an element every 6th node: about 1 m/s of plane wave, 1.5 MPa).  Returns ``(us, c, rho, cgrd, kw, zi, xi)``: ``us.fdtdSim(c, rho, cgrd, **kw)`` is
    the positive pulse, ``waveform=-kw["waveform"]`` its inverse; ``zi``, ``xi`` are the image's axes."""
    from qups_amd import Scan, Sequence, Transducer, UltrasoundSystem
    e = E2E
    z, x = np.arange(e["Z"]) * e["H"], (np.arange(e["X"]) - (e["X"] - 1) / 2) * e["H"]
    zi, xi = np.arange(10e-3, 14.01e-3, 0.15e-3), np.arange(-1.5e-3, 1.51e-3, 0.15e-3)          # pixels of a quarter wavelength at the fundamental
    us = UltrasoundSystem(Transducer.linear(16, 0.3e-3, e["FC"]), Sequence("PW", focus=np.array([[0.0], [0.0], [1.0]]), c0=e["C0"]), Scan.cartesian(xi, zi), fs=e["FS"])
    wt = np.arange(-48, 49) / 60e6
    w = e["AMP"] * np.sin(2 * np.pi * e["FC"] * wt) * np.exp(-(wt / 0.35e-6) ** 2)
    c = np.full((e["Z"], e["X"]), e["C0"])
    rho = np.full((e["Z"], e["X"]), e["RHO0"])
    rho[e["SCAT"]] *= 2
    kw = dict(waveform=w, wv_t0=wt[0], wv_fs=60e6, c0=e["C0"], rho0=e["RHO0"], isosub=True, BoA=e["BOA"], alpha=e["ALPHA"])
    return us, c, rho, Scan.cartesian(x, z), kw, zi, xi


def harmonic_level(b_fund, b_harm):
    """``(peak pixel of the fundamental image, of the harmonic image, 20 log10 of the ratio of the peaks)`` from the two envelope images"""
    kf, kh = (np.unravel_index(np.argmax(b), b.shape) for b in (b_fund, b_harm))
    return kf, kh, float(20.0 * np.log10(b_harm[kh] / b_fund[kf]))
