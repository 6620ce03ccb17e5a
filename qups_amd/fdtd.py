"""A 2-D acoustic FDTD channel-data simulator on the device: ``csrc/fdtd.hip`` behind :func:`fdtd` (arrays) and ``UltrasoundSystem.fdtdSim`` (objects).

The scheme is linear, lossless and first order on a staggered grid, of order ``2R`` in space (``include/qdas.h`` states it in full; ``tests/fdtd_ref.py`` is
its numpy restatement).  It follows the wrapper contract of the reference's ``kspaceFirstOrder`` (``src/UltrasoundSystem.m:2458-3170``) where that contract
is about our objects -- grid, time step, sources, sensors, ``t0``, ``isosub``, ``field`` -- but the numerical method is FDTD, NOT k-space pseudospectral:
absolute amplitude and dispersion are this discretisation's and are not matched to k-Wave.

Absorption is optional (``alpha``, ``alpha_power``): relaxation mechanisms fitted to a power law inside a band (:func:`relaxation_fit`), or the Stokes
term at ``alpha_power = 2`` -- a relaxation FDTD of the Fullwave kind, NOT k-Wave's fractional Laplacian (``qdas_fdtd_lossy``;
``tests/fdtd_loss_ref.py`` is its restatement).  Without ``alpha`` the solver is lossless and takes the path it always took.

Nonlinear propagation is optional too (``BoA``): k-Wave's nonlinear first-order equations -- the convective term in the density update and the quadratic
``B/2A`` term in the equation of state (``qdas_fdtd_nonlinear``; ``tests/fdtd_nl_ref.py`` is its restatement).  Without ``BoA`` the solver is linear and takes
the paths it always took.

Everything the kernel reads is prepared here on the host in float64 (the extended medium, staggered densities, PML factors, the sampled source table, the
per-tile point lists) and uploaded once; the states, the record and every table are torch tensors, so the C entry allocates nothing.  There is no CPU
fallback: without the library or a device the call raises."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .das_spec import DasError

__all__ = ["fdtd", "launch", "prepare", "time_step", "stability_limit", "tx_table", "pml_size", "pml_factors", "nearest_nodes", "iso_density", "grid_spacing",
           "tile_lists", "COEFS", "TILE", "STATES", "relaxation_fit", "relaxation_response", "alpha_np", "loss_model", "loss_time_step", "FIT_SPREADS", "nl_model", "source_mach"]

COEFS = {1: (1.0,), 2: (9.0 / 8.0, -1.0 / 24.0), 4: (1225.0 / 1024.0, -245.0 / 3072.0, 49.0 / 5120.0, -5.0 / 7168.0)}
TILE = (_lib.FDTD_TZ, _lib.FDTD_TX)


def stability_limit(R: int) -> float:
    """``c_max dt / h <= 1 / (sqrt(2) sum|a_k|)``: 0.707, 0.606 and 0.5497 for R = 1, 2, 4"""
    return 1.0 / (math.sqrt(2.0) * sum(abs(a) for a in COEFS[int(R)]))


def _order(order):
    if order not in (2, 4, 8):
        raise DasError(f"fdtd: order is 2, 4 or 8 (R = 1, 2, 4), got {order!r}")
    return int(order) // 2


def grid_spacing(z, x, y=None):
    """``h`` of a uniform square grid; unequal or non-uniform spacing (beyond 1e-6 relative) and a non-singleton y (``fdtd3.grid_spacing3`` takes volumes) are
    refused"""
    z, x = np.asarray(z, np.float64).reshape(-1), np.asarray(x, np.float64).reshape(-1)
    if y is not None and np.size(y) > 1:
        raise DasError("fdtd: the grid has a non-singleton y; this is the 2-D solver (3-D grids: qups_amd.fdtd3)")
    if z.size < 2 or x.size < 2:
        raise DasError("fdtd: the grid needs at least two nodes in z and in x")
    dz, dx = np.diff(z), np.diff(x)
    h = float(dz.mean())
    if not h > 0 or np.abs(dz - h).max() > 1e-6 * h or np.abs(dx - h).max() > 1e-6 * h:
        raise DasError(f"fdtd: the grid spacing must be uniform and equal in z and x (dz = {h:g}, dx = {float(dx.mean()):g})")
    return h


def time_step(fs, c_max, h, CFL_max=0.25, order=8):
    """``(ratio, fs_, dt)`` (reference ``:2714-2729``): the largest step allowed is ``dt_cfl = CFL_max h / c_max``; ``ratio = max(1, ceil((1 / fs) / dt_cfl))
    = max(1, ceil(c_max / (fs CFL_max h)))``, ``fs_ = ratio fs``, ``dt = 1 / fs_``; a ``dt`` above the scheme's stability limit is refused"""
    R = _order(order)
    if not (fs > 0 and c_max > 0 and h > 0 and CFL_max > 0):
        raise DasError("fdtd: fs, c_max, h and CFL_max must be positive")
    ratio = max(1, int(math.ceil(float(c_max) / (float(fs) * float(CFL_max) * float(h)) - 1e-12)))
    fs_ = ratio * float(fs)
    dt = 1.0 / fs_
    if c_max * dt / h > stability_limit(R):
        raise DasError(f"fdtd: c_max dt / h = {c_max * dt / h:.4f} is above the stability limit {stability_limit(R):.4f} of order {2 * R}")
    return ratio, fs_, dt


def _sample_cubic(w, idx):
    """``w`` at the fractional 0-based indices ``idx`` with the Catmull-Rom cubic ``greens`` uses for its waveform; taps outside the record are 0 (float64)"""
    w = np.asarray(w, np.float64).reshape(-1)
    idx = np.asarray(idx, np.float64)
    ti = np.floor(idx)
    u = idx - ti
    wt = 0.5 * np.stack([u * (-1.0 + u * (2.0 - u)), 2.0 + u * u * (3.0 * u - 5.0), u * (1.0 + u * (4.0 - 3.0 * u)), u * u * (u - 1.0)])
    out = np.zeros(idx.shape)
    for k in range(4):
        t = ti.astype(np.int64) - 1 + k
        ok = (t >= 0) & (t < w.size)
        out += np.where(ok, wt[k] * w[np.clip(t, 0, w.size - 1)], 0.0)
    return out


def tx_table(waveform, wv_t0, wv_fs, delays, apod, fs_):
    """``(s, txn0, txne)``: the source table ``T' x M x V`` in float64 (reference ``:2735-2741``).  ``del = -delays``;
    ``txn0 = floor((wv_t0 + min del) fs_)``, ``txne = ceil((wv_tend + max del) fs_)``; ``s[n, m, v] = apod[m, v] w((txn0 + n) / fs_ - del[m, v])``"""
    w = np.asarray(waveform, np.float64).reshape(-1)
    dl = -np.asarray(delays, np.float64)
    ap = np.asarray(apod, np.float64)
    tend = wv_t0 + (w.size - 1) / wv_fs
    txn0 = int(math.floor((wv_t0 + dl.min()) * fs_ + 1e-9))
    txne = int(math.ceil((tend + dl.max()) * fs_ - 1e-9))
    t = np.arange(txn0, txne + 1, dtype=np.float64)[:, None, None] / fs_
    s = ap[None] * _sample_cubic(w, (t - dl[None] - wv_t0) * wv_fs)
    return s, txn0, txne


def _largest_prime_factor(n):
    n, f, best = int(n), 2, 1
    while f * f <= n:
        while n % f == 0:
            best, n = f, n // f
        f += 1
    return max(best, n) if n > 1 else best


def pml_size(PML, Z, X, Y=None):
    """a scalar is taken as is; a pair ``[lo, hi]`` picks the size in that range whose ``Z + 2P`` and ``X + 2P`` (and ``Y + 2P`` of a volume) have the
    smallest largest prime factor (the first such size), as the reference does for its FFTs -- harmless here, kept for parity"""
    if np.ndim(PML) == 0:
        P = int(PML)
        if P < 0 or P != PML:
            raise DasError(f"fdtd: PML must be a non-negative integer, got {PML!r}")
        return P
    if np.size(PML) != 2:
        raise DasError(f"fdtd: PML is a size or a range [lo, hi], got {PML!r}")
    lo, hi = (int(v) for v in np.asarray(PML).reshape(-1))
    if lo < 0 or hi < lo:
        raise DasError(f"fdtd: PML is a size or a range [lo, hi], got {PML!r}")
    ext = [n for n in (Z, X, Y) if n is not None]
    return min(range(lo, hi + 1), key=lambda P: (max(_largest_prime_factor(n + 2 * P) for n in ext), P))


def pml_factors(N, P, c_max, h, dt):
    """``(A, A_staggered)`` of ``N`` nodes (the layer included): ``exp(-alpha dt / 2)``, ``alpha = 2 (c_max / h) (xi / P)^4``, ``xi`` the depth into the layer in
    cells, evaluated at ``i`` and at ``i + 1/2``; 1 inside and for ``P = 0`` (float64)"""
    i = np.arange(N, dtype=np.float64)
    if P == 0:
        return np.ones(N), np.ones(N)

    def A(pos):
        xi = np.maximum(np.maximum(P - pos, pos - (N - 1 - P)), 0.0)
        return np.exp(-(2.0 * (c_max / h) * (xi / P) ** 4) * dt / 2.0)

    return A(i), A(i + 0.5)


def nearest_nodes(z, x, pos):
    """``(iz, ix)`` of the nearest node per position; ``pos`` is ``3 x M`` with rows ``(x, y, z)``, as ``Transducer.positions()`` gives them, or ``2 x M``
    with rows ``(z, x)``.  The reference's assertion applies when two positions share a node (``:2753-2768``)."""
    z, x = np.asarray(z, np.float64).reshape(-1), np.asarray(x, np.float64).reshape(-1)
    pos = np.asarray(pos, np.float64)
    pz, px = (pos[2], pos[0]) if pos.shape[0] == 3 else (pos[0], pos[1])
    iz = np.abs(pz[:, None] - z[None]).argmin(1)
    ix = np.abs(px[:, None] - x[None]).argmin(1)
    if len({(a, b) for a, b in zip(iz.tolist(), ix.tolist())}) != iz.size:
        raise DasError("Elements are not unique; the Scan spacing or sizing may be too small.")
    return iz.astype(np.int64), ix.astype(np.int64)


def iso_density(c, c0, rho0):
    """the iso-impedance medium of ``isosub``: ``rho_iso = c0 rho0 / c`` (reference ``:2706-2712``)"""
    return float(c0) * float(rho0) / np.asarray(c, np.float64)


def tile_lists(Nz, Nx, nodes):
    """``(start, list)`` int32: the per-tile lists of the points at ``nodes`` (``j Nz + i``), from the library's host helper"""
    L = _lib.lib()
    nodes = np.ascontiguousarray(nodes, np.int32)
    nt = int(L.qdas_fdtd_tiles(Nz, Nx))
    start, lst = np.zeros(nt + 1, np.int32), np.zeros(max(nodes.size, 1), np.int32)
    _lib.check(L.qdas_fdtd_tile_lists(Nz, Nx, nodes.size, nodes.ctypes.data if nodes.size else None, start.ctypes.data, lst.ctypes.data))
    return start, lst[:nodes.size]


FIT_SPREADS = (1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # the `s` of relaxation_fit: how far the centres reach past the band
FIT_POINTS = 64


def alpha_np(alpha, y):
    """``a`` in Np (rad/s)^-y m^-1 from ``alpha`` in dB/(MHz^y cm), k-Wave's unit (the reference hands ``1e4 Medium.alpha0`` to k-Wave in it,
    ``src/Medium.m:443``): ``a = alpha 100 / (20 log10 e) (1e-6 / 2 pi)^y``"""
    return np.asarray(alpha, np.float64) * 100.0 / (20.0 * math.log10(math.e)) * (1e-6 / (2.0 * math.pi)) ** float(y)


def relaxation_response(tau, dt, w):
    """``(E, D)``: ``E_l = 1 - exp(-dt / tau_l)`` and the DISCRETE response ``D_l(w) = 1 - E_l / (1 - (1 - E_l) e^{i w dt})`` of the update
    ``e <- e + E (r - e)`` (``r - e = D r``), ``L x len(w)`` complex.  Its limit for ``dt -> 0`` is the Debye response ``-i w tau / (1 - i w tau)``."""
    tau = np.asarray(tau, np.float64).reshape(-1)
    w = np.asarray(w, np.float64).reshape(-1)
    E = -np.expm1(-float(dt) / tau)
    D = 1.0 - E[:, None] / (1.0 - (1.0 - E[:, None]) * np.exp(1j * w[None] * float(dt)))
    return E, D


def _nnls_active_sets(A, b):
    """``min |A g - b|_2`` over ``g >= 0`` for a handful of columns: the least-squares solution of every subset of columns that comes out positive is a
    candidate, and the optimum is the best of them (it is the unconstrained solution on its own support)"""
    n = A.shape[1]
    best, best_r = np.zeros(n), float(np.linalg.norm(b))
    for mask in range(1, 1 << n):
        cols = [k for k in range(n) if mask >> k & 1]
        g, *_ = np.linalg.lstsq(A[:, cols], b, rcond=None)
        if not (g > 0).all():
            continue
        r = float(np.linalg.norm(A[:, cols] @ g - b))
        if r < best_r:
            best_r, best = r, np.zeros(n)
            best[cols] = g
    return best


def relaxation_fit(y, band, dt, L=3):
    """``(tau, E, g, fit_err)``: ``L`` relaxation mechanisms whose summed loss follows ``w^y`` over ``band = (f_lo, f_hi)`` at the time step ``dt``.

    For small loss the scheme absorbs ``alpha(w) = (w / 2c) kap sum_l g_l (-Im D_l(w))`` with the update's own discrete response ``D_l``
    (:func:`relaxation_response`), so with ``kap = 2 c a`` the weights must make ``sum_l g_l (-Im D_l(w)) = w^(y - 1)``.  The centres ``1 / (2 pi tau_l)`` are
    log-spaced over ``[f_lo / s, s f_hi]``; for each ``s`` of ``FIT_SPREADS`` the non-negative ``g`` minimises the least squares of
    ``sum_l g_l (-Im D_l(w)) / w^(y - 1) - 1`` over 64 log-spaced frequencies of the band (the ``2^L`` active sets, each a ``lstsq``), and the ``s`` with the
    smallest LARGEST deviation is kept.  ``fit_err`` is that largest relative deviation from the power law inside the band: the model's own error, before
    any discretisation in space.  float64, numpy only."""
    y, dt, L = float(y), float(dt), int(L)
    f_lo, f_hi = (float(v) for v in band)
    if not 1 <= L <= _lib.FDTD_MAX_L:
        raise ValueError(f"relaxation_fit: L is 1 .. {_lib.FDTD_MAX_L}, got {L}")
    if not (0 < f_lo < f_hi and math.isfinite(f_hi)):
        raise ValueError(f"relaxation_fit: the band is (f_lo, f_hi) with 0 < f_lo < f_hi, got {band!r}")
    if not (1.0 <= y < 2.0):
        raise ValueError(f"relaxation_fit: 1 <= y < 2 (y = 2 is the Stokes term), got {y}")
    if not dt > 0:
        raise ValueError("relaxation_fit: dt must be positive")
    w = 2.0 * math.pi * np.geomspace(f_lo, f_hi, FIT_POINTS)
    w_ref = 2.0 * math.pi * math.sqrt(f_lo * f_hi)
    best = None
    for s in FIT_SPREADS:
        fc = np.geomspace(f_lo / s, s * f_hi, L) if L > 1 else np.array([math.sqrt(f_lo * f_hi)])
        tau = 1.0 / (2.0 * math.pi * fc)
        E, D = relaxation_response(tau, dt, w)
        A = (-D.imag / (w[None] / w_ref) ** (y - 1.0)).T           # columns scaled to O(1): g = g' w_ref^(y - 1)
        g = _nnls_active_sets(A, np.ones(w.size))
        err = float(np.abs(A @ g - 1.0).max())
        if best is None or err < best[3]:
            best = (tau, E, g * w_ref ** (y - 1.0), err)
        if L == 1:
            break                                                    # one centre: the spread does not move it
    return best


def loss_model(c, alpha, alpha_power, alpha_band, dt, mechanisms=3):
    """the loss block of one run from the interior maps, float64: a dict with ``mode`` (``"stokes"`` | ``"relax"``), ``L``, ``tau, E, g, fit_err`` and
    ``kap`` (``Z x X``: ``2 c a`` under relaxation, ``mud = 2 c a / dt`` under Stokes), and ``speed``: the largest speed the time step must respect,
    ``max c sqrt(1 + kap sum g)`` (the unrelaxed speed) or, for Stokes, ``max c sqrt(1 + 2 mud)`` (its factor at the Nyquist frequency).  ``alpha``: a scalar
    or a ``Z x X`` map in dB/(MHz^y cm); ``y < 1``, ``y > 2`` and a negative or non-finite ``alpha`` raise ``ValueError``."""
    c = np.asarray(c, np.float64)
    y = 1.01 if alpha_power is None else float(alpha_power)
    if not (1.0 <= y <= 2.0):
        raise ValueError(f"fdtd: alpha_power is 1 .. 2 (relaxation below 2, Stokes at 2), got {alpha_power!r}")
    al = np.asarray(alpha.detach().cpu().numpy() if hasattr(alpha, "detach") else alpha, np.float64)
    if al.ndim and al.size != c.size:
        raise DasError(f"fdtd: alpha is a scalar or a map of the grid's size {c.shape}, got {al.shape}")
    if not np.isfinite(al).all() or (al < 0).any():
        raise ValueError("fdtd: alpha must be finite and not negative")
    a = alpha_np(np.broadcast_to(al.reshape(c.shape) if al.ndim else al, c.shape), y)
    dt = float(dt)
    if y == 2.0:
        kap = 2.0 * c * a / dt
        return dict(mode="stokes", L=0, y=y, tau=np.zeros(0), E=np.zeros(0), g=np.zeros(0), fit_err=0.0, kap=kap, speed=float((c * np.sqrt(1.0 + 2.0 * kap)).max()))
    if alpha_band is None:
        raise DasError("fdtd: alpha_band = (f_lo, f_hi) is needed to fit the relaxation mechanisms")
    tau, E, g, fit_err = relaxation_fit(y, alpha_band, dt, mechanisms)
    kap = 2.0 * c * a
    return dict(mode="relax", L=int(mechanisms), y=y, tau=tau, E=E, g=g, fit_err=fit_err, kap=kap, speed=float((c * np.sqrt(1.0 + kap * g.sum())).max()))


def _given_loss(loss, c):
    """a caller's loss block checked and completed to :func:`loss_model`'s dict"""
    mode = loss.get("mode")
    if mode not in ("stokes", "relax"):
        raise DasError(f"fdtd: the loss block's mode is 'stokes' or 'relax', got {mode!r}")
    g, E = (np.asarray(loss.get(k, ()), np.float64).reshape(-1) for k in ("g", "E"))
    kap = np.asarray(loss["kap"], np.float64)
    if kap.shape != c.shape:
        raise DasError(f"fdtd: the loss map has the grid's size {c.shape}, got {kap.shape}")
    if g.size != E.size or (mode == "stokes") != (g.size == 0) or g.size > _lib.FDTD_MAX_L:
        raise DasError(f"fdtd: relaxation takes 1 .. {_lib.FDTD_MAX_L} pairs (g, E), Stokes none; got {g.size} and {E.size}")
    if not np.isfinite(kap).all() or (kap < 0).any() or not np.isfinite(g).all() or (g < 0).any() or not ((E > 0) & (E <= 1)).all():
        raise ValueError("fdtd: the loss map and g must be finite and not negative, E inside (0, 1]")
    speed = float((c * np.sqrt(1.0 + (2.0 * kap if mode == "stokes" else kap * g.sum()))).max())
    return dict(mode=mode, L=int(g.size), y=loss.get("y"), tau=loss.get("tau"), E=E, g=g, fit_err=loss.get("fit_err"), kap=kap, speed=speed)


def loss_time_step(fs, c, alpha, alpha_power, alpha_band, h, CFL_max=0.25, order=8, mechanisms=3):
    """``(ratio, fs_, dt, loss)`` with absorption: fit at the lossless ``dt``, take ``dt`` from ``CFL_max`` with the speed bound of that fit
    (:func:`loss_model`'s ``speed``), then fit again at the final ``dt``: ``loss`` is that last model"""
    c = np.asarray(c, np.float64)
    _, _, dt0 = time_step(fs, c.max(), h, CFL_max, order)
    first = loss_model(c, alpha, alpha_power, alpha_band, dt0, mechanisms)
    ratio, fs_, dt = time_step(fs, first["speed"], h, CFL_max, order)
    return ratio, fs_, dt, loss_model(c, alpha, alpha_power, alpha_band, dt, mechanisms)


def nl_model(rho, BoA, convective=True):
    """the nonlinear block of one run from the interior maps, float64: ``None`` for ``BoA = None`` or an all-NaN ``BoA`` (the reference drops ``BonA`` only when
    every value is NaN, ``src/Medium.m:442-447``: the linear solver), else a dict with ``bq = BoA / (2 rho)`` (``Z x X``), ``convective`` and ``beta_max``:
    the largest coefficient of nonlinearity ``1 + B/2A`` (``B/2A`` alone without the convective term).  ``BoA = 0`` is still nonlinear (``beta = 1``), as in
    k-Wave.  ``BoA``: a scalar or a ``Z x X`` map; a map that is partly NaN, or a negative or infinite value, raises ``ValueError``."""
    if BoA is None:
        return None
    rho = np.asarray(rho, np.float64)
    b = np.asarray(BoA.detach().cpu().numpy() if hasattr(BoA, "detach") else BoA, np.float64)
    if b.ndim and b.size != rho.size:
        raise DasError(f"fdtd: BoA is a scalar or a map of the grid's size {rho.shape}, got {b.shape}")
    if np.isnan(b).all():
        return None
    if not np.isfinite(b).all() or (b < 0).any():
        raise ValueError("fdtd: BoA must be finite and not negative (or NaN everywhere: the linear solver)")
    b = np.broadcast_to(b.reshape(rho.shape) if b.ndim else b, rho.shape)
    return dict(bq=b / (2.0 * rho), convective=bool(convective), beta_max=float((1.0 if convective else 0.0) + b.max() / 2.0))


def source_mach(s, c, dt, h):
    """the source Mach number of a transmit table in m/s: ``max|s| (2 c_max dt / h) / c_min`` -- the largest velocity one source node adds in a step (its
    weight is ``2 c dt / h``) over the slowest speed; a line of sources radiates ``v0 = s`` each way, so this bounds ``u / c`` at the aperture"""
    c = np.asarray(c, np.float64)
    s = np.asarray(s, np.float64)
    return float(np.abs(s).max() * 2.0 * c.max() * float(dt) / float(h) / c.min()) if s.size else 0.0


def prepare(c, rho, h, dt, P):
    """the kernel's host tables in float64 from the interior medium ``c``, ``rho`` (``Z x X``): a dict with ``Nz, Nx, c2, rho, dtrz, dtrx`` (``Nx x Nz``, z
    fastest: extended by edge replication, the staggered density the mean of the two neighbours with the last row kept) and ``az, azs, ax, axs``"""
    c, rho = np.asarray(c, np.float64), np.asarray(rho, np.float64)
    if c.ndim != 2 or rho.shape != c.shape:
        raise DasError(f"fdtd: c and rho are Z x X maps of one shape, got {c.shape} and {rho.shape}")
    if not (np.isfinite(c).all() and np.isfinite(rho).all() and (c > 0).all() and (rho > 0).all()):
        raise DasError("fdtd: c and rho must be finite and positive")
    ce, re = np.pad(c, P, mode="edge"), np.pad(rho, P, mode="edge")
    sgz, sgx = re.copy(), re.copy()
    sgz[:-1] = 0.5 * (re[:-1] + re[1:])
    sgx[:, :-1] = 0.5 * (re[:, :-1] + re[:, 1:])
    Nz, Nx = ce.shape
    c_max = float(c.max())
    az, azs = pml_factors(Nz, P, c_max, h, dt)
    ax, axs = pml_factors(Nx, P, c_max, h, dt)
    T = lambda a: np.ascontiguousarray(a.T)
    return dict(Nz=Nz, Nx=Nx, c=T(ce), c2=T(ce * ce), rho=T(re), dtrz=T(dt / sgz), dtrx=T(dt / sgx), az=az, azs=azs, ax=ax, axs=axs)


def fdtd(c, rho, z, x, src_pos, src_normal, s, sen_pos, Nt, dt, PML=20, order=8, prec="single", bsize=None, device=None, return_state=False, ld=None, prepare_only=False,
         sen_nodes=None, alpha=None, alpha_power=None, alpha_band=None, mechanisms=3, loss=None, BoA=None, convective=True):
    """``rec = fdtd(c, rho, z, x, src_pos, src_normal, s, sen_pos, Nt, dt)``: ``Nt`` steps of the scheme on the grid ``z`` x ``x`` (``c``, ``rho``: ``Z x X``)
    with ``PML`` cells added on every side.  ``src_pos`` / ``sen_pos``: positions (``3 x M`` rows x, y, z, or ``2 x M`` rows z, x) mapped to their nearest
    nodes; ``src_normal``: ``2 x M`` rows ``(nz, nx)``; ``s``: the source table ``T' x M x V`` (host array or tensor).  Returns the record ``Nt x N x V`` (a
    device tensor of ``prec``), and with ``return_state`` also a dict of the five state arrays ``V x Nx x Nz`` after the last step.  ``sen_nodes``: the
    sensors' interior nodes ``(iz, ix)`` given directly, in place of ``sen_pos`` (``field``: every node).  ``bsize``: pulses per call, to bound the memory of
    the states: without ``return_state`` ONE set of ``bsize x Nx x ld`` state arrays serves every block.  ``ld``: the row stride of the state arrays (default ``Nz``).  ``prepare_only``: ``(meta, tables, s)`` on the device for :func:`launch`, nothing run.
    Queued on torch's current stream.

    ABSORPTION.  ``alpha``: a scalar or a ``Z x X`` map in dB/(MHz^y cm) (k-Wave's ``alpha_coeff``), ``alpha_power = y`` (default 1.01) one number for the
    grid.  ``1 <= y < 2``: ``mechanisms = L <= 4`` relaxation mechanisms fitted to ``w^y`` over ``alpha_band = (f_lo, f_hi)`` by :func:`relaxation_fit` at
    this ``dt`` (a relaxation FDTD of the Fullwave kind, NOT k-Wave's fractional Laplacian; the fit's own error is ``meta["loss"]["fit_err"]`` of
    ``prepare_only``); ``y = 2``: the Stokes term, no extra state.  The map is extended into the PML like ``c`` and ``rho``.  Each pulse then holds ``5 + L``
    state arrays (``bsize`` bounds all of them), and ``return_state`` adds ``"e"``: ``V x L x Nx x Nz``.  ``dt`` must respect the unrelaxed speed
    (:func:`loss_model`).  ``loss``: the block given directly in place of ``alpha`` -- a dict with ``mode`` (``"stokes"`` | ``"relax"``), ``g``, ``E`` and the
    interior map ``kap`` (``2 c a``, or ``mud`` under Stokes), as :func:`loss_model` returns it.  ``alpha=None`` and ``loss=None``: the lossless solver,
    exactly as before.

    NONLINEARITY.  ``BoA``: a scalar or a ``Z x X`` map of B/A, extended into the PML like ``c``: the density update gains the convective term
    (``rho + 2 (rz + rx)`` in place of ``rho``; ``convective=False`` switches it off) and the equation of state ``B/2A rn^2 / rho`` (``qdas_fdtd_nonlinear``).  A
    progressive plane wave then follows Westervelt's equation with ``beta = 1 + B/2A``; ``BoA = 0`` is still nonlinear (``beta = 1``), as in k-Wave.  THE
    SOURCE TABLE IS IN m/s: a line of sources ``s = v0`` radiates a plane wave of particle velocity ``v0`` (pressure ``rho c v0``) each way, and under
    nonlinearity its absolute size matters.  ``dt`` is the linear one (the amplitude does not enter the stability check).  There is no shock capturing:
    without absorption a wave that reaches the shock distance (``sigma = 1``) rings at the grid scale.  ``BoA`` combines with ``alpha`` / ``loss``.
    ``BoA=None`` or all NaN: the linear solver, exactly as before; a partly NaN map, a negative or an infinite value: ``ValueError``."""
    import torch
    if prec not in ("single", "double"):
        raise DasError("fdtd: prec must be 'single' or 'double'")
    R = _order(order)
    h = grid_spacing(z, x)
    zc, xc = np.asarray(z, np.float64).reshape(-1), np.asarray(x, np.float64).reshape(-1)
    c = np.asarray(c.detach().cpu().numpy() if hasattr(c, "detach") else c, np.float64)
    rho = np.asarray(rho.detach().cpu().numpy() if hasattr(rho, "detach") else rho, np.float64)
    if c.shape != (zc.size, xc.size):
        raise DasError(f"fdtd: c is Z x X = {zc.size} x {xc.size}, got {c.shape}")
    P = pml_size(PML, zc.size, xc.size)
    dt = float(dt)
    if not (dt > 0 and math.isfinite(dt)):
        raise DasError("fdtd: dt must be positive")
    if c.max() * dt / h > stability_limit(R):
        raise DasError(f"fdtd: c_max dt / h = {c.max() * dt / h:.4f} is above the stability limit {stability_limit(R):.4f} of order {2 * R}")
    if alpha is not None and loss is not None:
        raise DasError("fdtd: give alpha or a ready-made loss block, not both")
    if loss is not None:
        loss = _given_loss(loss, c)
    if alpha is not None:
        loss = loss_model(c, alpha, alpha_power, alpha_band, dt, mechanisms)
    if loss is not None:
        if loss["speed"] * dt / h > stability_limit(R):
            raise DasError(f"fdtd: with absorption the fastest speed is {loss['speed']:.1f} m/s and c dt / h = {loss['speed'] * dt / h:.4f} is above the "
                           f"stability limit {stability_limit(R):.4f} of order {2 * R}")
    nl = nl_model(rho, BoA, convective) if rho.shape == c.shape else None
    tab = prepare(c, rho, h, dt, P)
    Nz, Nx = tab["Nz"], tab["Nx"]
    s_host = None if isinstance(s, torch.Tensor) else np.asarray(s, np.float64)
    if (s.ndim if s_host is None else s_host.ndim) != 3:
        raise DasError("fdtd: the source table is T' x M x V")
    Ts, M, V = (int(v) for v in (s.shape if s_host is None else s_host.shape))
    siz, six = nearest_nodes(zc, xc, src_pos) if M else (np.zeros(0, np.int64),) * 2
    if sen_nodes is not None:
        niz, nix = (np.asarray(a, np.int64).reshape(-1) for a in sen_nodes)
        if niz.size != nix.size or (niz.size and (niz.min() < 0 or niz.max() >= zc.size or nix.min() < 0 or nix.max() >= xc.size)):
            raise DasError("fdtd: sen_nodes are (iz, ix) inside the grid")
    else:
        niz, nix = nearest_nodes(zc, xc, sen_pos) if np.size(sen_pos) else (np.zeros(0, np.int64),) * 2
    nrm = np.asarray(src_normal, np.float64).reshape(2, -1)
    if siz.size != M or nrm.shape[1] != M:
        raise DasError(f"fdtd: {siz.size} source positions and {nrm.shape[1]} normals for a table of M = {M} sources")
    N, Nt = int(niz.size), int(Nt)
    if Nt < 0:
        raise DasError("fdtd: Nt must not be negative")
    src_node = ((six + P) * Nz + (siz + P)).astype(np.int32)
    sen_node = ((nix + P) * Nz + (niz + P)).astype(np.int32)
    csrc = tab["c"].reshape(-1)[src_node] if M else np.zeros(0)
    wz, wx = nrm[0] * 2.0 * csrc * dt / h, nrm[1] * 2.0 * csrc * dt / h

    if device is None:
        device = s.device if s_host is None and s.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DasError("fdtd: needs a device (there is no CPU fallback in this package)")
    rdt = torch.float32 if prec == "single" else torch.float64
    up = lambda a, dt_=None: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt_ or rdt)
    src_start, src_list = tile_lists(Nz, Nx, src_node)
    sen_start, sen_list = tile_lists(Nz, Nx, sen_node)
    tb = {k: up(tab[k]) for k in ("c2", "rho", "dtrz", "dtrx", "az", "azs", "ax", "axs")}
    tb.update(src_wz=up(wz), src_wx=up(wx))
    tb.update({k: up(v, torch.int32) for k, v in (("src_node", src_node), ("src_start", src_start), ("src_list", src_list), ("sen_node", sen_node),
                                                  ("sen_start", sen_start), ("sen_list", sen_list))})
    s_dev = (s if s_host is None else up(s_host)).to(device=dev, dtype=rdt)
    ld = Nz if ld is None else int(ld)
    if ld < Nz:
        raise DasError(f"fdtd: ld = {ld} is less than Nz = {Nz}")
    meta = dict(Nz=Nz, Nx=Nx, Nt=Nt, ld=ld, M=M, Ts=Ts, N=N, dt_h=dt / h, inv_h=1.0 / h, double=prec == "double", order=2 * R)
    Lm = 0
    if loss is not None:                                         # the map joins the tables under "kap"; launch() takes it out again
        tb["kap"] = up(np.ascontiguousarray(np.pad(loss["kap"], P, mode="edge").T))
        meta["loss"] = {k: loss[k] for k in ("mode", "L", "y", "tau", "E", "g", "fit_err", "speed")}
        Lm = loss["L"]
    if nl is not None:                                           # likewise under "bq"
        tb["bq"] = up(np.ascontiguousarray(np.pad(nl["bq"], P, mode="edge").T))
        meta["nl"] = dict(convective=nl["convective"], beta_max=nl["beta_max"])
    if prepare_only:
        return meta, tb, s_dev
    rec = torch.empty((Nt, N, V), dtype=rdt, device=dev)
    bs = V if not bsize else max(1, min(int(bsize), V))
    states = {k: [] for k in STATES}
    pool = None                                                  # the one set of state arrays every block works in, unless the states are wanted
    with torch.cuda.device(dev):
        for v0 in range(0, V, bs) if V else ():
            Vb = min(bs, V - v0)
            if return_state or pool is None:
                pool = {k: torch.empty((Vb, Nx, ld), dtype=rdt, device=dev) for k in STATES}
                if Lm:
                    pool["e"] = torch.empty((Vb, Lm, Nx, ld), dtype=rdt, device=dev)
            st = {k: pool[k][:Vb] for k in pool}
            for k in st:
                st[k].zero_()
            launch(meta, tb, st, s_dev[:, :, v0:v0 + Vb].contiguous(), rec, v0)
            if return_state:
                for k in st:
                    states.setdefault(k, []).append(st[k][..., :Nz])
    if not return_state:
        return rec
    cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    empty = torch.zeros((0, Nx, Nz), dtype=rdt, device=dev)
    if Lm and not states.get("e"):
        states["e"] = [torch.zeros((0, Lm, Nx, Nz), dtype=rdt, device=dev)]
    return rec, {k: (cat(v) if v else empty) for k, v in states.items()}


STATES = ("p", "uz", "ux", "rz", "rx")


def launch(meta, tb, st, sb, rec, v0=0, stream=None):
    """one call of ``qdas_fdtd``: ``meta`` the sizes and scalars, ``tb`` the device tables by the names of ``qdas_fdtd_args``, ``st`` the five state tensors
    ``Vb x Nx x ld`` (zero for a start from rest), ``sb`` the source table ``T' x M x Vb`` (contiguous), ``rec`` the whole record ``Nt x N x V`` of which the
    pulses ``v0 .. v0 + Vb - 1`` are written.  ``stream``: a ``torch.cuda.Stream`` (default: the current one).  Only enqueues.

    With ``meta["loss"]`` (``mode``, ``L``, ``g``, ``E``) the call is ``qdas_fdtd_lossy``: ``tb["kap"]`` is the loss map and ``st["e"]`` the memory
    variables ``Vb x L x Nx x ld`` (relaxation only).  With ``meta["nl"]`` (``convective``) the call is ``qdas_fdtd_nonlinear``, with or without a loss block:
    ``tb["bq"]`` is the map ``BoA / (2 rho)``."""
    import torch
    dev = st["p"].device
    Vb = int(st["p"].shape[0])
    d = _lib.FdtdDesc()
    d.Nz, d.Nx, d.V, d.Nt, d.ld, d.vstride = meta["Nz"], meta["Nx"], Vb, meta["Nt"], meta["ld"], meta["Nx"] * meta["ld"]
    d.M, d.Ts, d.N = meta["M"], meta["Ts"], meta["N"]
    d.rec_st, d.rec_sn, d.rec_sv = (int(v) for v in rec.stride())
    d.dt_h, d.inv_h = meta["dt_h"], meta["inv_h"]
    d.dtype, d.order = (0 if meta["double"] else 1), meta["order"]                  # QDAS_F64 | QDAS_F32
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.flags = int(meta.get("flags", 0))                                           # _lib.FDTD_ZERO: the entry clears the states itself
    stream = stream or torch.cuda.current_stream(dev)
    d.queue = C.c_void_p(stream.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    a = _lib.FdtdArgs()
    for k in STATES:
        setattr(a, k, ptr(st[k]))
    for k, t in tb.items():
        if k not in ("kap", "bq"):
            setattr(a, k, ptr(t))
    a.s = ptr(sb)
    a.rec = C.c_void_p(rec.data_ptr() + v0 * rec.stride(2) * rec.element_size()) if rec.numel() else None
    loss, nl = meta.get("loss"), meta.get("nl")
    q = None
    if loss is None and nl is None:
        _lib.check(_lib.lib().qdas_fdtd(C.byref(d), C.byref(a)))
    elif loss is not None:
        q = _lib.FdtdLoss()
        q.mode, q.L = (_lib.FDTD_LOSS_STOKES if loss["mode"] == "stokes" else _lib.FDTD_LOSS_RELAX), int(loss["L"])
        for k in range(q.L):
            q.g[k], q.E[k] = float(loss["g"][k]), float(loss["E"][k])
        q.kap = ptr(tb.get("kap"))
        q.e = ptr(st.get("e"))
        if q.L and st.get("e") is not None and (tuple(st["e"].shape[:2]) != (Vb, q.L) or tuple(st["e"].stride()) != (q.L * d.vstride, d.vstride, d.ld, 1)):
            raise DasError(f"fdtd: the memory variables are Vb x L x Nx x ld = {Vb} x {q.L} x {meta['Nx']} x {meta['ld']} in the states' layout")
        if nl is None:
            _lib.check(_lib.lib().qdas_fdtd_lossy(C.byref(d), C.byref(a), C.byref(q)))
    if nl is not None:
        w = _lib.FdtdNl()
        w.bq, w.flags = ptr(tb.get("bq")), (0 if nl.get("convective", True) else _lib.FDTD_NL_NO_CONVECTIVE)
        _lib.check(_lib.lib().qdas_fdtd_nonlinear(C.byref(d), C.byref(a), C.byref(q) if q is not None else None, C.byref(w)))
    if sb.numel():
        sb.record_stream(stream)
