"""float64 oracle of the 3-D eikonal feature, written from the update rule alone (nothing of the reference's msfm3d.c or of Kroon's C is copied).

``fmm3``: heap fast marching (frozen / narrow band / far) of the first-order, six-neighbour system with msfm3d's own rule.  With ``t_x, t_y, t_z`` the
smaller FROZEN neighbour along each axis (absent: +inf) and ``s = 1 / max(c / dp, eps)``: all finite ones go into one quadratic
``n T^2 - 2 T sum(t) + sum(t^2) - s^2 = 0``, the discriminant is clamped at 0 and the larger root taken; if that root is below any finite ``t`` the value is
``min(t) + s`` instead (NOT the two-term root).  Sources are floored to a node and get ``T = 0``; several points make one map.

``classical_update`` / ``fixed_point``: the classical upwind update (sorted axis minima ``t1 <= t2 <= t3``; ``t1 + s``, the two-term root while the value
exceeds ``t2``, the three-term root while it exceeds ``t3``) iterated by brute force, Jacobi, from +inf until nothing changes.  The device iterates this
rule; that its fixed point IS what the heap solver produces is the claim tests/test_eikonal3_host.py checks on tiny grids.

``sample3``: separable cubic convolution (Keys, a = -1/2) along dimension 1, then 2, then 3, NaN outside the grid, ghost nodes beyond the border by the rule of
tests/eikonal_ref.py applied dimension by dimension in that order.  A zero weight reads nothing.  Every sum is taken in the order the kernel
takes it, so only the kernel's fused multiply-adds separate the two (a few 1e-16 relative), and a pixel on a node gets the node's value bit for bit.
"""
import heapq

import numpy as np

EPS = np.finfo(np.float64).eps
INF = float("inf")


def _rule(ts, s):
    """msfm3d's value of a node from the frozen axis minima ``ts`` (at least one finite)"""
    f = [t for t in ts if t < INF]
    n = len(f)
    S = sum(f)
    Q = sum(t * t for t in f)
    disc = max(4.0 * S * S - 4.0 * n * (Q - s * s), 0.0)
    T = (2.0 * S + disc ** 0.5) / (2.0 * n)
    if any(T < t for t in f):
        T = min(f) + s
    return T


def _nodes(src, shape, base):
    out = []
    for p in np.asarray(src, np.float64).reshape(3, -1).T:
        q = tuple(int(np.floor(v - base)) for v in p)
        assert all(0 <= q[d] < shape[d] for d in range(3)), (p, shape)
        out.append(q)
    return out


def fmm3(c, dp, src, base=1):
    """``c``: C1 x C2 x C3 speeds, ``src``: 3 x P coordinates in index base ``base``; returns the C1 x C2 x C3 map in seconds"""
    c = np.asarray(c, np.float64)
    C = c.shape
    sl = (1.0 / np.maximum(c / dp, EPS)).tolist()           # (python lists: the scalar loop is several times faster than numpy indexing)
    Tl = np.full(C, np.inf).tolist()
    fz = np.zeros(C, bool).tolist()
    heap = []
    for q in _nodes(src, C, base):
        Tl[q[0]][q[1]][q[2]] = 0.0
        heapq.heappush(heap, (0.0,) + q)
    steps = ((1, 0, 0), (0, 1, 0), (0, 0, 1))

    def frozen(x, y, z):
        return Tl[x][y][z] if 0 <= x < C[0] and 0 <= y < C[1] and 0 <= z < C[2] and fz[x][y][z] else INF

    while heap:
        _, i, j, l = heapq.heappop(heap)
        if fz[i][j][l]:
            continue
        fz[i][j][l] = True
        for d in steps:
            for sg in (-1, 1):
                x, y, z = i + sg * d[0], j + sg * d[1], l + sg * d[2]
                if x < 0 or y < 0 or z < 0 or x >= C[0] or y >= C[1] or z >= C[2] or fz[x][y][z]:
                    continue
                ts = [min(frozen(x - e[0], y - e[1], z - e[2]), frozen(x + e[0], y + e[1], z + e[2])) for e in steps]
                v = _rule(ts, sl[x][y][z])
                if v < Tl[x][y][z]:
                    Tl[x][y][z] = v
                    heapq.heappush(heap, (v, x, y, z))
    return np.array(Tl)


def classical_update(a, b, c, s):
    """the classical first-order upwind value from the axis minima ``a, b, c`` (arrays; absent: +inf)"""
    t1, t2, t3 = np.sort(np.stack([a, b, c]), axis=0)
    with np.errstate(invalid="ignore"):
        v = t1 + s
        two = v > t2
        r2 = 0.5 * (t1 + t2 + np.sqrt(np.maximum(2.0 * s * s - (t1 - t2) ** 2, 0.0)))
        v = np.where(two, r2, v)
        three = two & (v > t3)
        r3 = (t1 + t2 + t3 + np.sqrt(np.maximum(3.0 * s * s - (t1 - t2) ** 2 - (t1 - t3) ** 2 - (t2 - t3) ** 2, 0.0))) / 3.0
        return np.where(three, r3, v)


def fixed_point(c, dp, src, base=1, max_sweeps=10000):
    """``T <- min(T, classical_update(T))`` at every node at once from +inf until a sweep changes nothing; returns ``(T, sweeps)``"""
    c = np.asarray(c, np.float64)
    s = 1.0 / np.maximum(c / dp, EPS)
    T = np.full(c.shape, np.inf)
    for q in _nodes(src, c.shape, base):
        T[q] = 0.0
    for sweep in range(1, max_sweeps + 1):
        P = np.pad(T, 1, constant_values=np.inf)
        a = np.minimum(P[:-2, 1:-1, 1:-1], P[2:, 1:-1, 1:-1])
        b = np.minimum(P[1:-1, :-2, 1:-1], P[1:-1, 2:, 1:-1])
        d = np.minimum(P[1:-1, 1:-1, :-2], P[1:-1, 1:-1, 2:])
        N = np.minimum(T, classical_update(a, b, d, s))
        if np.array_equal(N, T):
            return T, sweep
        T = N
    raise AssertionError("no fixed point")


# ---------------------------------------------------------------------------------------------------------------- sampler
def _extend(A, axis):
    """``A`` with one ghost node on either side along ``axis``: Keys' rule 3 f(0) - 3 f(1) + f(2), two nodes linear, one constant"""
    A = np.moveaxis(A, axis, 0)
    C = A.shape[0]
    if C >= 3:
        lo, hi = 3.0 * A[0] - 3.0 * A[1] + A[2], 3.0 * A[C - 1] - 3.0 * A[C - 2] + A[C - 3]
    elif C == 2:
        lo, hi = 2.0 * A[0] - A[1], 2.0 * A[1] - A[0]
    else:
        lo, hi = A[0], A[0]
    return np.moveaxis(np.concatenate([lo[None], A, hi[None]], 0), 0, axis)


def _keys(u, C):
    ok = (u >= 0) & (u <= C - 1)
    uu = np.where(ok, u, 0.0)
    fl = np.floor(uu)
    if C >= 2:
        fl = np.minimum(fl, C - 2)
    f = uu - fl
    f2 = f * f
    f3 = f2 * f
    w = np.stack([-0.5 * f3 + f2 - 0.5 * f, 1.5 * f3 - 2.5 * f2 + 1.0, -1.5 * f3 + 2.0 * f2 + 0.5 * f, 0.5 * f3 - 0.5 * f2])
    return ok, fl.astype(np.int64), w


def sample3(T, Pi, base=1):
    """``T``: C1 x C2 x C3, ``Pi``: 3 x I grid coordinates; returns I values"""
    T = np.asarray(T, np.float64)
    C = T.shape
    E = _extend(_extend(_extend(T, 0), 1), 2)               # E[i + 1, j + 1, l + 1] = node (i, j, l)
    Pi = np.asarray(Pi, np.float64).reshape(3, -1)
    ok, i0, w = zip(*(_keys(Pi[d] - base, C[d]) for d in range(3)))
    n = Pi.shape[1]
    add = lambda acc, wt, v: acc + np.where(wt != 0, wt * np.where(wt != 0, v, 0.0), 0.0)
    out = np.zeros(n)
    for cz in range(4):
        gz = np.zeros(n)
        for b in range(4):
            g = np.zeros(n)
            for a in range(4):          # node (i0 - 1 + a, ...); (an index is clipped only where its weight is 0: a single-node line)
                v = E[np.minimum(i0[0] + a, C[0] + 1), np.minimum(i0[1] + b, C[1] + 1), np.minimum(i0[2] + cz, C[2] + 1)]
                g = add(g, w[0][a], v)
            gz = add(gz, w[1][b], g)
        out = add(out, w[2][cz], gz)
    return np.where(ok[0] & ok[1] & ok[2], out, np.nan)


# ---------------------------------------------------------------------------------------------------------------- speed volumes of the tests
def layers_ball(C1, C2, C3):
    """two half spaces 1500 | 15000 m/s along dimension 0 (a 10 : 1 interface: head waves) plus a 3000 m/s ball in the slow half"""
    c = np.full((C1, C2, C3), 1500.0)
    c[(C1 + 1) // 2:] = 15000.0
    i, j, l = np.ogrid[:C1, :C2, :C3]
    c[(i - 0.25 * C1) ** 2 + (j - 0.5 * C2) ** 2 + (l - 0.4 * C3) ** 2 <= (0.2 * min(C1, C2, C3)) ** 2] = 3000.0
    return c


def smooth_random(C1, C2, C3, seed=0):
    """a smooth volume with max c / min c <= 2 (a few low-order cosines, scaled into 1000 .. 2000 m/s)"""
    rng = np.random.default_rng(seed)
    i, j, l = np.meshgrid(*(np.arange(C) / max(C - 1, 1) for C in (C1, C2, C3)), indexing="ij")
    f = np.zeros((C1, C2, C3))
    for _ in range(6):
        k = rng.uniform(0, 3, 3)
        ph, am = rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1)
        f += am * np.cos(2 * np.pi * (k[0] * i + k[1] * j + k[2] * l) + ph)
    f = (f - f.min()) / max(f.max() - f.min(), 1e-300)
    return 1000.0 + 1000.0 * f
