"""The restatement of qdas_fdtd in numpy, written once for float64 and float32 (``dtype``): the scheme of include/qdas.h with whole-array slices.

Grid ``Z x X`` nodes of spacing ``h`` plus ``P`` PML cells on every side (``c``, ``rho`` extended by edge replication); ``p``, ``rz``, ``rx`` at ``(i, j)``,
``uz`` at ``(i + 1/2, j)``, ``ux`` at ``(i, j + 1/2)``; ``rho_sgz[i, j] = (rho[i, j] + rho[i + 1, j]) / 2`` with the last row kept, x likewise.

    D+f[i] = (1/h) sum_k a_k (f[i + k] - f[i - k + 1])      D-g[i] = (1/h) sum_k a_k (g[i + k - 1] - g[i - k])       (0 outside the array)

    1. uz <- A+z (A+z uz - (dt / rho_sgz) D+z p), ux likewise        2. uz[src] += nz s[n, m, v] 2 c[src] dt / h, ux[src] += nx s ...
    3. rz <- Az (Az rz - dt rho D-z uz), rx likewise                  4. p = c^2 (rz + rx)              5. rec[n, j, v] = p[sensor j]

``A = exp(-alpha dt / 2)``, ``alpha = 2 (c_max / h) (xi / P)^4``, ``xi`` the depth into the layer in cells (at ``+ 1/2`` for the staggered factors).
Arrays here are ``V x Z' x X'`` (z is axis 1); the tables are made in float64 and rounded once to ``dtype``, as the device's are."""
import numpy as np

COEFS = {1: (1.0,), 2: (9.0 / 8.0, -1.0 / 24.0), 4: (1225.0 / 1024.0, -245.0 / 3072.0, 49.0 / 5120.0, -5.0 / 7168.0)}


def limit(R):
    return 1.0 / (np.sqrt(2.0) * sum(abs(a) for a in COEFS[R]))


def pml(N, P, c_max, h, dt):
    A, As = np.ones(N), np.ones(N)
    for i in range(N):
        for arr, pos in ((A, float(i)), (As, i + 0.5)):
            xi = max(P - pos, pos - (N - 1 - P), 0.0) if P else 0.0
            if xi > 0:
                arr[i] = np.exp(-2.0 * (c_max / h) * (xi / P) ** 4 * dt / 2.0)
    return A, As


def _shift(f, k, axis):
    """g[i] = f[i + k] along ``axis``, 0 outside"""
    g = np.zeros_like(f)
    n = f.shape[axis]
    if abs(k) >= n:
        return g
    src = [slice(None)] * f.ndim
    dst = [slice(None)] * f.ndim
    src[axis] = slice(max(k, 0), n + min(k, 0))
    dst[axis] = slice(max(-k, 0), n - max(k, 0))
    g[tuple(dst)] = f[tuple(src)]
    return g


def dplus(f, axis, R, dtype):
    d = np.zeros_like(f)
    for k in range(1, R + 1):
        d += dtype(COEFS[R][k - 1]) * (_shift(f, k, axis) - _shift(f, 1 - k, axis))
    return d


def dminus(g, axis, R, dtype):
    d = np.zeros_like(g)
    for k in range(1, R + 1):
        d += dtype(COEFS[R][k - 1]) * (_shift(g, k - 1, axis) - _shift(g, -k, axis))
    return d


def tables(c, rho, h, dt, P):
    c, rho = np.asarray(c, np.float64), np.asarray(rho, np.float64)
    ce, re = np.pad(c, P, mode="edge"), np.pad(rho, P, mode="edge")
    sgz, sgx = re.copy(), re.copy()
    sgz[:-1] = (re[:-1] + re[1:]) / 2
    sgx[:, :-1] = (re[:, :-1] + re[:, 1:]) / 2
    az, azs = pml(ce.shape[0], P, c.max(), h, dt)
    ax, axs = pml(ce.shape[1], P, c.max(), h, dt)
    return ce, re, sgz, sgx, az, azs, ax, axs


def simulate(c, rho, h, dt, P, R, src, nrm, s, sen, Nt, dtype=np.float64, snapshots=False):
    """``c``, ``rho``: ``Z x X``; ``src``, ``sen``: ``(iz, ix)`` integer arrays of INTERIOR nodes; ``nrm``: ``2 x M`` rows ``(nz, nx)``; ``s``: ``T' x M x V``.
    Returns ``(rec Nt x N x V, state dict of V x Z' x X' arrays[, snapshots Nt x Z x X x V of the interior p])`` in ``dtype``."""
    dtype = np.dtype(dtype).type
    ce, re, sgz, sgx, az, azs, ax, axs = tables(c, rho, h, dt, P)
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    c2, rr, dtrz, dtrx = f(ce * ce), f(re), f(dt / sgz), f(dt / sgx)
    az, azs, ax, axs = f(az)[None, :, None], f(azs)[None, :, None], f(ax)[None, None, :], f(axs)[None, None, :]
    inv_h, dt_h = dtype(1.0 / h), dtype(dt / h)
    s = f(s)
    Ts, M, V = s.shape
    siz, six = (np.asarray(a, np.int64) + P for a in src)
    niz, nix = (np.asarray(a, np.int64) + P for a in sen)
    nrm = np.asarray(nrm, np.float64).reshape(2, -1)
    wz = f(nrm[0] * 2.0 * ce[siz, six] * dt / h) if M else f(np.zeros(0))
    wx = f(nrm[1] * 2.0 * ce[siz, six] * dt / h) if M else f(np.zeros(0))
    Nz, Nx = ce.shape
    p, uz, ux, rz, rx = (np.zeros((V, Nz, Nx), dtype) for _ in range(5))
    rec = np.zeros((Nt, len(niz), V), dtype)
    snap = np.zeros((Nt, Nz - 2 * P, Nx - 2 * P, V), dtype) if snapshots else None
    for n in range(Nt):
        uz = azs * (azs * uz - (dtrz * inv_h)[None] * dplus(p, 1, R, dtype))
        ux = axs * (axs * ux - (dtrx * inv_h)[None] * dplus(p, 2, R, dtype))
        if n < Ts and M:
            uz[:, siz, six] += (wz[:, None] * s[n]).T
            ux[:, siz, six] += (wx[:, None] * s[n]).T
        rz = az * (az * rz - (dt_h * rr)[None] * dminus(uz, 1, R, dtype))
        rx = ax * (ax * rx - (dt_h * rr)[None] * dminus(ux, 2, R, dtype))
        p = c2[None] * (rz + rx)
        rec[n] = p[:, niz, nix].T
        if snapshots:
            snap[n] = np.moveaxis(p[:, P:Nz - P, P:Nx - P], 0, -1)
    state = dict(p=p, uz=uz, ux=ux, rz=rz, rx=rx)
    return (rec, state, snap) if snapshots else (rec, state)


def xcorr_lag(a, b):
    """the lag (in samples, parabolic-interpolated) at which ``b`` best matches ``a`` delayed"""
    x = np.correlate(np.asarray(b, np.float64), np.asarray(a, np.float64), "full")
    k = int(np.argmax(x))
    y0, y1, y2 = x[k - 1], x[k], x[k + 1]
    return k - (len(a) - 1) + 0.5 * (y0 - y2) / (y0 - 2 * y1 + y2)


# ---------------------------------------------------------------------------------------------------------------- the parity cases (host core and GPU)
TZ, TX = 64, 16                    # the kernel's tile over the EXTENDED grid (z along lanes); tests/test_fdtd_host.py checks them against the header
# (Z, X, P): Nz x Nx = 49 x 41 (no tile multiple), 64 x 64 (exactly 1 x 4 tiles), 11 x 138 and 138 x 11 (thinner than the halo of R = 4 inside, 9 and 3 tiles
# across), 65 x 49 (one node past a tile both ways: Z = 49 and not 65, so that Nz = 49 + 16 = 64 + 1; Nx = 33 + 16 = 48 + 1)
GRIDS = [(37, 29, 6), (64, 64, 0), (3, 130, 4), (130, 3, 4), (49, 33, 8)]
H, NT, TS = 1e-4, 100, 40


def smooth_map(Z, X, lo, hi, seed):
    """a smooth random map with min ``lo`` and max ``hi``: a few low cosines"""
    rng = np.random.default_rng(seed)
    zz, xx = np.meshgrid(np.arange(Z) / max(Z - 1, 1), np.arange(X) / max(X - 1, 1), indexing="ij")
    u = sum(rng.standard_normal() * np.cos(np.pi * (a * zz + b * xx) + rng.uniform(0, 6)) for a in range(3) for b in range(3))
    u = (u - u.min()) / max(u.max() - u.min(), 1e-30)
    return lo + (hi - lo) * u


def _pick(Z, X, P):
    """sources and sensors: the first and the last interior node, a tile corner, a tile's last row (and last lane where the grid reaches one); the last
    interior node is both a source and a sensor"""
    def first(n, P, mod, want, default):
        return next((k for k in range(n) if (k + P) % mod == want), default)
    corner = (first(Z, P, TZ, 0, 0), first(X, P, TX, 0, X // 2))
    last = (first(Z, P, TZ, TZ - 1, Z - 1), first(X, P, TX, TX - 1, X // 2))
    uniq = lambda pts: list(dict.fromkeys(pts))
    src = uniq([(0, 0), (Z - 1, X - 1), corner, last])
    sen = uniq([(Z - 1, X - 1), (corner[0], min(corner[1] + 1, X - 1)), (Z // 2, X // 2), (0, X - 1)])
    return src, sen


def parity_case(Z, X, P, V, seed=0):
    """the inputs of one parity case (float64): a heterogeneous medium with c_max / c_min = 1.2, a source table with different delays and apodization per
    pulse, dt at 0.3 of c_max dt / h (inside the limit of every order)"""
    rng = np.random.default_rng(seed + 7 * Z + X)
    c = smooth_map(Z, X, 1400.0, 1680.0, seed + Z)
    rho = smooth_map(Z, X, 900.0, 1100.0, seed + X + 1)
    dt = 0.3 * H / c.max()
    src, sen = _pick(Z, X, P)
    M = len(src)
    nrm = np.array([[1.0, 0.0, 0.6, -0.8][:M], [0.0, 1.0, 0.8, 0.6][:M]])
    dl = rng.uniform(0, 8, (M, V))
    ap = rng.uniform(0.5, 1.5, (M, V))
    n = np.arange(TS, dtype=np.float64)[:, None, None]
    s = ap[None] * np.sin(2 * np.pi * (n - dl[None] - 12) / 16.0) * np.exp(-(((n - dl[None] - 12) / 6.0) ** 2))
    z, x = np.arange(Z) * H, (np.arange(X) - (X - 1) / 2) * H
    return dict(c=c, rho=rho, h=H, dt=dt, P=P, src=(np.array([a for a, _ in src]), np.array([b for _, b in src])),
                sen=(np.array([a for a, _ in sen]), np.array([b for _, b in sen])), nrm=nrm, s=s, Nt=NT, z=z, x=x)


_REFS = {}


def parity_refs(Z, X, P, R, V):
    """``(case, ref64, ref32, d32)``, computed once: ``ref* = (rec, state)`` of the restatement, ``d32[name] = max|ref32 - ref64| / max|ref64|`` per output"""
    key = (Z, X, P, R, V)
    if key not in _REFS:
        cs = parity_case(Z, X, P, V)
        run = lambda dt_: simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, R, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], dt_)
        r64, r32 = run(np.float64), run(np.float32)
        d32 = {"rec": np.abs(r32[0] - r64[0]).max() / np.abs(r64[0]).max()}
        for k in r64[1]:
            d32[k] = np.abs(r32[1][k] - r64[1][k]).max() / np.abs(r64[1][k]).max()
        for a in (r64[0], r32[0], *r64[1].values(), *r32[1].values()):
            a.setflags(write=False)
        _REFS[key] = (cs, r64, r32, d32)
    return _REFS[key]


def tolerance(d32, double):
    """the rule of tests/test_gpu_fdtd.py: float32 within ``8 d32`` (floor 1e-6), float64 within ``8 d32 2^-29`` (floor 1e-13), relative to the output's own maximum"""
    return max(8 * d32 * 2.0 ** -29, 1e-13) if double else max(8 * d32, 1e-6)
