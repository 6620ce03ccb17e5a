// raypaths_walk.h -- the walk of one straight ray through a rectilinear grid, shared by the two kernels of raypaths.hip.  Plain C++ with no HIP in it: the
// same text compiles for the host, where tests/raypaths_walk_host.cpp runs it on the CPU (bounds and results, no device needed).
//
// With d = b - a the point a + t d, t in [0, 1], is monotonic in both axes, so the crossings with the lines x = xg[i] and with the lines z = zg[k] are two
// increasing sequences of t: the walk keeps the index of its cell (ix, iz), the parameter of the next crossing on either axis, and takes the smaller one (both
// when the ray goes through a node).  Crossing an x-line puts the point's x ON the grid value, so its hat function is exactly 0 or 1 there and a ray along a
// grid line weights that line only.  The part outside the grid is clipped first (Liang-Barsky).
//
// A segment from p1 to p2 of length l inside cell (ix, iz), with u = (x - xg[ix]) / hx and v = (z - zg[iz]) / hz clamped to [0, 1], gives corner
// (ix + i, iz + k) l times the mean of the product of its two hats, both linear along the segment: with f = (i ? u : 1 - u), g = (k ? v : 1 - v) at the ends
//   w = l (2 f1 g1 + f1 g2 + f2 g1 + 2 f2 g2) / 6
// -- the reference's closed form a_x a_z - (a_x b_z + a_z b_x) / 2 + b_x b_z / 3 with a = (f1, g1), b = (f1 - f2, g1 - g2) multiplied out: a sum of products
// of numbers in [0, 1], so no weight is negative whatever the rounding.  The four weights sum to l.
//
// The walk is a `for` over the K = X + Z + 1 slots: its trip count never depends on a floating-point value.  A ray with a non-finite coordinate, of zero
// length or past the grid emits nothing; so does a cell whose edges are not increasing (a NaN in the grid), and whatever a broken grid holds, the weights
// that are emitted are finite and not negative and their indices lie inside the grid.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QDAS_RAYP_HD __host__ __device__ inline
#else
#define QDAS_RAYP_HD inline
#endif

namespace qdas {
namespace rayp {

// the cell of coordinate p on the axis g[0 .. n-1] (n >= 2): the largest i in [0, n - 2] with g[i] <= p -- g[i] < p when the ray runs down this axis, so
// that a start ON a grid line belongs to the cell the ray walks into.  At most 32 halvings of an integer interval.
template <typename R> QDAS_RAYP_HD int find_cell(const R *g, int n, R p, bool down) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32; ++it) {
        if (hi - lo <= 1) break;
        const int mid = (lo + hi) >> 1;
        const R gm = g[mid];
        if (down ? (gm < p) : (gm <= p)) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename R> QDAS_RAYP_HD R clamp01(R v) { return v > R(0) ? (v < R(1) ? v : R(1)) : R(0); }          // (NaN -> 0)
template <typename R> QDAS_RAYP_HD R clampr(R v, R lo, R hi) { return v < lo ? lo : (v > hi ? hi : v); }
template <typename R> QDAS_RAYP_HD bool finite(R v) { return v - v == R(0); }

// xs, zs: the grid vectors less their first value (xs[0] = zs[0] = 0); a, b: the end points in the same frame.  Calls slot(s, emit, ix, iz, w00, w10, w01,
// w11) for s = 0, 1, ... : with ALL for every one of the K slots (an empty one: emit = false, weights 0), otherwise until the ray has ended.  emit: the
// weights belong to the corners (ix, iz), (ix + 1, iz), (ix, iz + 1), (ix + 1, iz + 1), 0 <= ix <= X - 2, 0 <= iz <= Z - 2.
template <typename R, bool ALL, typename Slot>
QDAS_RAYP_HD void walk(const R *xs, const R *zs, int X, int Z, R ax, R az, R bx, R bz, Slot &&slot) {
    const int K = X + Z + 1;
    const R dx = bx - ax, dz = bz - az;
    const R L = sqrt(dx * dx + dz * dz);
    const R xhi = xs[X - 1], zhi = zs[Z - 1];
    const R INF = R(INFINITY);

    // ---- clip to the grid: t in [t0, t1]
    bool live = finite(ax) && finite(az) && finite(bx) && finite(bz) && L > R(0) && finite(L);
    R t0 = R(0), t1 = R(1);
    if (dx != R(0)) {
        const R ta = (R(0) - ax) / dx, tb = (xhi - ax) / dx;
        const R lo = dx > R(0) ? ta : tb, hi = dx > R(0) ? tb : ta;
        if (lo > t0) t0 = lo;
        if (hi < t1) t1 = hi;
    } else live = live && ax >= R(0) && ax <= xhi;
    if (dz != R(0)) {
        const R ta = (R(0) - az) / dz, tb = (zhi - az) / dz;
        const R lo = dz > R(0) ? ta : tb, hi = dz > R(0) ? tb : ta;
        if (lo > t0) t0 = lo;
        if (hi < t1) t1 = hi;
    } else live = live && az >= R(0) && az <= zhi;
    live = live && t0 < t1;

    // ---- the first cell and the first crossings
    R px = ax, pz = az;                       // the current point; exact at t0 = 0
    if (t0 > R(0)) { px = clampr(ax + t0 * dx, R(0), xhi); pz = clampr(az + t0 * dz, R(0), zhi); }
    if (!live) { px = R(0); pz = R(0); }
    int ix = find_cell(xs, X, px, dx < R(0)), iz = find_cell(zs, Z, pz, dz < R(0));
    const int sx = dx > R(0) ? 1 : (dx < R(0) ? -1 : 0), sz = dz > R(0) ? 1 : (dz < R(0) ? -1 : 0);
    const R rdx = R(1) / dx, rdz = R(1) / dz;   // (inf when the ray does not move on the axis: then never used)
    // length per unit of the dominant axis: segment lengths come from differences of that coordinate, which are exact between two of its grid lines
    const bool xdom = fabs(dx) >= fabs(dz);
    const R lscale = L / (xdom ? fabs(dx) : fabs(dz));
    R tx = sx ? (xs[ix + (sx > 0)] - ax) * rdx : INF;
    R tz = sz ? (zs[iz + (sz > 0)] - az) * rdz : INF;
    R tc = t0;

    for (int s = 0; s < K; ++s) {
        R w00 = R(0), w10 = R(0), w01 = R(0), w11 = R(0);
        bool emit = false;
        const int cx = ix, cz = iz;
        if (live) {
            // the next event: the end of the clipped ray, or a grid line
            R tn = t1;
            if (tx < tn) tn = tx;
            if (tz < tn) tn = tz;
            const bool hitx = tx <= tn, hitz = tz <= tn, last = !(tn < t1);
            const R gx0 = xs[ix], gx1 = xs[ix + 1], gz0 = zs[iz], gz1 = zs[iz + 1];
            R qx, qz;                                     // the point at tn
            if (last && t1 == R(1)) { qx = bx; qz = bz; }
            else { qx = ax + tn * dx; qz = az + tn * dz; }
            if (hitx) qx = sx > 0 ? gx1 : gx0;
            if (hitz) qz = sz > 0 ? gz1 : gz0;
            qx = clampr(qx, gx0, gx1);
            qz = clampr(qz, gz0, gz1);
            const R hx = gx1 - gx0, hz = gz1 - gz0;
            const R l = (xdom ? fabs(qx - px) : fabs(qz - pz)) * lscale;
            if (tn > tc && l > R(0) && l < INF && hx > R(0) && hz > R(0)) {
                const R u1 = clamp01((px - gx0) / hx), u2 = clamp01((qx - gx0) / hx);
                const R v1 = clamp01((pz - gz0) / hz), v2 = clamp01((qz - gz0) / hz);
                const R m1 = R(1) - u1, m2 = R(1) - u2, n1 = R(1) - v1, n2 = R(1) - v2;
                const R l6 = l / R(6);
                w00 = l6 * (R(2) * m1 * n1 + m1 * n2 + m2 * n1 + R(2) * m2 * n2);
                w10 = l6 * (R(2) * u1 * n1 + u1 * n2 + u2 * n1 + R(2) * u2 * n2);
                w01 = l6 * (R(2) * m1 * v1 + m1 * v2 + m2 * v1 + R(2) * m2 * v2);
                w11 = l6 * (R(2) * u1 * v1 + u1 * v2 + u2 * v1 + R(2) * u2 * v2);
                emit = true;
            }
            if (tn > tc) { tc = tn; px = qx; pz = qz; }
            // step into the next cell(s)
            if (hitx) {
                ix += sx;
                if (ix < 0 || ix > X - 2) { ix = ix < 0 ? 0 : X - 2; tx = INF; }
                else tx = (xs[ix + (sx > 0)] - ax) * rdx;
            }
            if (hitz) {
                iz += sz;
                if (iz < 0 || iz > Z - 2) { iz = iz < 0 ? 0 : Z - 2; tz = INF; }
                else tz = (zs[iz + (sz > 0)] - az) * rdz;
            }
            if (last || !(hitx || hitz)) live = false;      // (neither: a NaN in the grid; stop)
        }
        slot(s, emit, cx, cz, w00, w10, w01, w11);
        if (!ALL && !live) break;
    }
}

}  // namespace rayp
}  // namespace qdas
