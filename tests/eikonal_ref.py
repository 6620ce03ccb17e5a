"""float64 oracle of the eikonal feature, written from the update rule alone (nothing of the reference's msfm2d.m or of Kroon's C is copied).

``fmm``: heap fast marching (frozen / narrow band / far) of the first-order, four-neighbour system.  With ``a``, ``b`` the smaller FROZEN neighbour
along each axis and ``s = 1 / max(c / dp, eps)``:  ``T = min(a, b) + s`` if ``|a - b| >= s`` or one is absent, else
``T = (a + b + sqrt(2 s^2 - (a - b)^2)) / 2``.  Sources are floored to a node and get ``T = 0``; several points make one map.

``sample``: separable cubic convolution (Keys, a = -1/2) at fractional grid coordinates, NaN outside the grid, ghost nodes beyond the border by
Keys' rule ``f(-1) = 3 f(0) - 3 f(1) + f(2)`` (two nodes: linear; one: constant).  A zero weight reads nothing.
"""
import heapq

import numpy as np

EPS = np.finfo(np.float64).eps


def _update(a, b, s):
    lo, hi = (a, b) if a <= b else (b, a)
    if hi - lo < s:                                        # (inf - finite = inf, never < s)
        return 0.5 * (a + b + np.sqrt(2.0 * s * s - (a - b) * (a - b)))
    return lo + s


def fmm(c, dp, src, base=1):
    """``c``: C1 x C2 speeds, ``src``: 2 x P coordinates in index base ``base``; returns the C1 x C2 map in seconds"""
    c = np.asarray(c, np.float64)
    C1, C2 = c.shape
    s = 1.0 / np.maximum(c / dp, EPS)
    T = np.full((C1, C2), np.inf)
    frozen = np.zeros((C1, C2), bool)
    heap = []
    for p in np.asarray(src, np.float64).reshape(2, -1).T:
        i, j = int(np.floor(p[0] - base)), int(np.floor(p[1] - base))
        assert 0 <= i < C1 and 0 <= j < C2
        T[i, j] = 0.0
        heapq.heappush(heap, (0.0, i, j))
    Tl, sl = T.tolist(), s.tolist()                         # (python lists: the scalar loop is several times faster than numpy indexing)
    fz = frozen.tolist()
    inf = float("inf")
    while heap:
        t, i, j = heapq.heappop(heap)
        if fz[i][j]:
            continue
        fz[i][j] = True
        for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            x, y = i + di, j + dj
            if x < 0 or y < 0 or x >= C1 or y >= C2 or fz[x][y]:
                continue
            a = min(Tl[x - 1][y] if x > 0 and fz[x - 1][y] else inf, Tl[x + 1][y] if x + 1 < C1 and fz[x + 1][y] else inf)
            b = min(Tl[x][y - 1] if y > 0 and fz[x][y - 1] else inf, Tl[x][y + 1] if y + 1 < C2 and fz[x][y + 1] else inf)
            v = float(_update(a, b, sl[x][y]))
            if v < Tl[x][y]:
                Tl[x][y] = v
                heapq.heappush(heap, (v, x, y))
    return np.array(Tl)


def _ghost(f0, f1, f2, C):
    return 3.0 * f0 - 3.0 * f1 + f2 if C >= 3 else (2.0 * f0 - f1 if C == 2 else f0)


def _extend(T):
    """the map with one ghost node on every side (first along dimension 0, then along dimension 1 of the extended lines)"""
    def ext(A):
        C = A.shape[0]
        g = lambda k: A[k] if 0 <= k < C else np.zeros_like(A[0])
        lo = _ghost(g(0), g(1), g(2), C)
        hi = _ghost(g(C - 1), g(C - 2) if C >= 2 else g(-1), g(C - 3) if C >= 3 else g(-1), C)
        return np.concatenate([lo[None], A, hi[None]], 0)
    return ext(ext(T).T).T


def _keys(u, C):
    ok = (u >= 0) & (u <= C - 1)
    uu = np.where(ok, u, 0.0)
    fl = np.floor(uu)
    if C >= 2:
        fl = np.minimum(fl, C - 2)
    f = uu - fl
    f2, f3 = f * f, f * f * f
    w = np.stack([-0.5 * f3 + f2 - 0.5 * f, 1.5 * f3 - 2.5 * f2 + 1.0, -1.5 * f3 + 2.0 * f2 + 0.5 * f, 0.5 * f3 - 0.5 * f2])
    return ok, fl.astype(np.int64), w


def sample(T, Pi, base=1):
    """``T``: C1 x C2, ``Pi``: 2 x I grid coordinates; returns I values"""
    T = np.asarray(T, np.float64)
    C1, C2 = T.shape
    E = _extend(T)                                          # E[i + 1, j + 1] = node (i, j)
    Pi = np.asarray(Pi, np.float64).reshape(2, -1)
    ok1, i0, wu = _keys(Pi[0] - base, C1)
    ok2, j0, wv = _keys(Pi[1] - base, C2)
    out = np.zeros(Pi.shape[1])
    for b in range(4):
        g = np.zeros(Pi.shape[1])
        for a in range(4):
            v = E[np.minimum(i0 + a, C1 + 1), np.minimum(j0 + b, C2 + 1)]   # node (i0 - 1 + a, j0 - 1 + b); (clipped only where the weight is 0: a single-node line)
            g = g + np.where(wu[a] != 0, wu[a] * np.where(wu[a] != 0, v, 0.0), 0.0)
        out = out + np.where(wv[b] != 0, wv[b] * np.where(wv[b] != 0, g, 0.0), 0.0)
    return np.where(ok1 & ok2, out, np.nan)


# ---------------------------------------------------------------------------------------------------------------- speed maps of the tests
def layers_disc(C1=161, C2=121):
    """four layers 1400-1600 m/s along dimension 0 plus a 1650 m/s disc"""
    c = np.empty((C1, C2))
    q = C1 // 4
    for k, v in enumerate((1500.0, 1400.0, 1600.0, 1450.0)):
        c[k * q:(k + 1) * q if k < 3 else C1] = v
    i, j = np.ogrid[:C1, :C2]
    c[(i - 0.6 * C1) ** 2 + (j - 0.4 * C2) ** 2 <= (0.12 * min(C1, C2)) ** 2] = 1650.0
    return c


def smooth_random(C1, C2, seed=0):
    """a smooth map with max c / min c <= 2 (a few low-order cosines, scaled into 1000 .. 2000 m/s)"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(C1) / max(C1 - 1, 1), np.arange(C2) / max(C2 - 1, 1), indexing="ij")
    f = np.zeros((C1, C2))
    for _ in range(6):
        k1, k2, ph, am = rng.uniform(0, 3), rng.uniform(0, 3), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1)
        f += am * np.cos(2 * np.pi * (k1 * i + k2 * j) + ph)
    f = (f - f.min()) / max(f.max() - f.min(), 1e-300)
    return 1000.0 + 1000.0 * f
