// raypaths_node.h -- the weight one straight ray gives ONE grid node: the walk of raypaths_walk.h turned round for the transposed product (raypaths.hip,
// qdas_raypaths_backproject), where a lane owns a node and asks every ray for its weight -- a gather, so no atomics.  Plain C++ with no HIP in it: the same
// text compiles for the host, where tests/raypaths_node_host.cpp runs it on the CPU.
//
// The hat of node (i, k) is supported on [xg[i-1], xg[i+1]] x [zg[k-1], zg[k+1]] (one-sided on the border).  Along the ray a + t d it is the product of two
// piecewise linear functions of t, with one break where x = xg[i] and one where z = zg[k].  So: clip t in [0, 1] to the support (Liang-Barsky, as the walk
// clips to the grid), insert the two breaks -- at most three pieces -- and on each piece, with f and g the two hats at its ends and l its length,
//   w += l (2 f1 g1 + f1 g2 + f2 g1 + 2 f2 g2) / 6
// the walk's formula: a sum of products of numbers in [0, 1], so no weight is negative whatever the rounding.
//
// The walk's habits are kept.  A point that an event produced takes the grid value itself: where the ray enters or leaves the support on an axis its
// coordinate IS the support's edge (hat exactly 0), at a break it IS the node's (hat exactly 1), so a ray along a grid line weighs that line only.  A piece's
// length is the difference of the dominant coordinate times |d| / |d_dom|.  Nothing loops, so no trip count depends on the data.  A NaN, an Inf or a
// non-increasing grid value can only make a weight 0: every hat goes through clamp01 (NaN -> 0) and a piece counts only with 0 < l < inf.
//
// What depends on the node alone is a lane constant (Node: six grid values, four reciprocal spacings), what depends on the ray alone a ray constant (Ray:
// the reciprocals of d, the length scale).  node_weight itself divides nothing.
#pragma once
#include "raypaths_walk.h"

namespace qdas {
namespace rayp {

template <typename R> struct Node {
    R xm, x, xp, zm, z, zp;        // the support and the node, in the frame of the grid's first values; xm == x in the first column, xp == x in the last
    R rxm, rxp, rzm, rzp;          // 1 / (x - xm) ... ; 0 where the support is one-sided
};

// one axis of a Node: g the grid vector as the caller holds it (n values), i the node
template <typename R> QDAS_RAYP_HD void node_axis(const R *g, int n, int i, R &m, R &c, R &p, R &rm, R &rp) {
    const R g0 = g[0], INF = R(INFINITY);
    c = g[i] - g0;
    m = i > 0 ? g[i - 1] - g0 : c;
    p = i < n - 1 ? g[i + 1] - g0 : c;
    const R hm = c - m, hp = p - c;
    rm = (hm > R(0) && hm < INF) ? R(1) / hm : R(0);
    rp = (hp > R(0) && hp < INF) ? R(1) / hp : R(0);
    if (rm == R(0)) m = c;         // (a spacing that is not positive and finite: that side has no support)
    if (rp == R(0)) p = c;
}

template <typename R> QDAS_RAYP_HD Node<R> make_node(const R *xg, int X, int ix, const R *zg, int Z, int iz) {
    Node<R> n;
    node_axis(xg, X, ix, n.xm, n.x, n.xp, n.rxm, n.rxp);
    node_axis(zg, Z, iz, n.zm, n.z, n.zp, n.rzm, n.rzp);
    return n;
}

template <typename R> struct Ray {
    R ax, az, bx, bz;              // the end points, in the frame of the grid's first values
    R rdx, rdz;                    // 1 / d (inf where the ray does not move on the axis)
    R ls6;                         // |d| / |d_dom| / 6: a difference of the dominant coordinate times this is a piece's l / 6
    bool live;                     // finite, of non-zero length
};

template <typename R> QDAS_RAYP_HD Ray<R> make_ray(R ax, R az, R bx, R bz) {
    Ray<R> q;
    q.ax = ax; q.az = az; q.bx = bx; q.bz = bz;
    const R dx = bx - ax, dz = bz - az;
    const R L = sqrt(dx * dx + dz * dz);
    q.live = finite(ax) && finite(az) && finite(bx) && finite(bz) && L > R(0) && finite(L);
    q.rdx = R(1) / dx;
    q.rdz = R(1) / dz;
    q.ls6 = L / (fabs(dx) >= fabs(dz) ? fabs(dx) : fabs(dz)) / R(6);
    return q;
}

// Liang-Barsky on one axis: where a + t d enters and leaves [lo, hi] (-inf / inf for a ray that does not move there: then it must lie inside).  The same
// rounded expressions serve a node's support and a tile's box, and rounding is monotonic: a box that contains another never clips tighter than it.
template <typename R> QDAS_RAYP_HD bool clip_axis(R a, R d, R rd, R lo, R hi, R &tin, R &tout) {
    tin = -R(INFINITY);
    tout = R(INFINITY);
    if (d == R(0)) return a >= lo && a <= hi;
    const R ta = (lo - a) * rd, tb = (hi - a) * rd;
    tin = d > R(0) ? ta : tb;
    tout = d > R(0) ? tb : ta;
    return true;
}

// the kernel gives a wave a tile of TILE x TILE nodes; on one axis the supports of the nodes TILE t .. TILE t + TILE - 1 lie inside [lo, hi]: the tile grown
// by one grid line on either side
constexpr int TILE = 8;
template <typename R> QDAS_RAYP_HD void tile_axis(const R *g, int n, int t, R &lo, R &hi) {
    const int i0 = TILE * t - 1, i1 = TILE * t + TILE;
    lo = g[i0 > 0 ? i0 : 0] - g[0];
    hi = g[i1 < n - 1 ? i1 : n - 1] - g[0];
}

// does the part t in [0, 1] of the ray meet the box?  (conservative: a NaN edge does not clip)
template <typename R> QDAS_RAYP_HD bool ray_meets_box(const Ray<R> &q, R xlo, R xhi, R zlo, R zhi) {
    R xin, xout, zin, zout;
    bool ok = q.live;
    ok = clip_axis(q.ax, q.bx - q.ax, q.rdx, xlo, xhi, xin, xout) && ok;
    ok = clip_axis(q.az, q.bz - q.az, q.rdz, zlo, zhi, zin, zout) && ok;
    R t0 = R(0), t1 = R(1);
    if (xin > t0) t0 = xin;
    if (zin > t0) t0 = zin;
    if (xout < t1) t1 = xout;
    if (zout < t1) t1 = zout;
    return ok && t0 < t1;
}

// one hat at coordinate v (already inside [m, p]): exactly 1 at the node, exactly 0 at the support's edge
template <typename R> QDAS_RAYP_HD R hat(R v, R m, R c, R p, R rm, R rp) {
    return v == c ? R(1) : clamp01(v < c ? (v - m) * rm : (p - v) * rp);
}

template <typename R> QDAS_RAYP_HD R node_weight(const Node<R> &n, const Ray<R> &q) {
    const R INF = R(INFINITY);
    const R dx = q.bx - q.ax, dz = q.bz - q.az;
    const bool xdom = fabs(dx) >= fabs(dz);
    // ---- clip to the support: t in [t0, t1]
    R xin, xout, zin, zout;
    bool ok = q.live;
    ok = clip_axis(q.ax, dx, q.rdx, n.xm, n.xp, xin, xout) && ok;
    ok = clip_axis(q.az, dz, q.rdz, n.zm, n.zp, zin, zout) && ok;
    R t0 = R(0), t1 = R(1);
    if (xin > t0) t0 = xin;
    if (zin > t0) t0 = zin;
    if (xout < t1) t1 = xout;
    if (zout < t1) t1 = zout;
    ok = ok && t0 < t1;
    // ---- the two breaks, where they fall strictly inside (a ray that does not move on an axis: 0 x inf or inf, never inside)
    R tbx = (n.x - q.ax) * q.rdx, tbz = (n.z - q.az) * q.rdz;
    const bool xbrk = tbx > t0 && tbx < t1, zbrk = tbz > t0 && tbz < t1;
    if (!xbrk) tbx = t0;
    if (!zbrk) tbz = t0;
    const R t[4] = {t0, tbx < tbz ? tbx : tbz, tbx < tbz ? tbz : tbx, t1};
    const R xe_in = dx > R(0) ? n.xm : n.xp, xe_out = dx > R(0) ? n.xp : n.xm;
    const R ze_in = dz > R(0) ? n.zm : n.zp, ze_out = dz > R(0) ? n.zp : n.zm;
    // ---- the four points (a function of t alone: equal parameters give the same point, a piece of length exactly 0) and the hats there
    R c[4], f[4], g[4];
    for (int k = 0; k < 4; ++k) {
        const R tk = t[k];
        R x = tk >= R(1) ? q.bx : q.ax + tk * dx, z = tk >= R(1) ? q.bz : q.az + tk * dz;
        x = clampr(x, n.xm, n.xp);
        z = clampr(z, n.zm, n.zp);
        if (tk == xin) x = xe_in;
        if (tk == xout) x = xe_out;
        if (xbrk && tk == tbx) x = n.x;
        if (tk == zin) z = ze_in;
        if (tk == zout) z = ze_out;
        if (zbrk && tk == tbz) z = n.z;
        c[k] = xdom ? x : z;
        f[k] = hat(x, n.xm, n.x, n.xp, n.rxm, n.rxp);
        g[k] = hat(z, n.zm, n.z, n.zp, n.rzm, n.rzp);
    }
    // ---- the three pieces
    R w = R(0);
    for (int k = 0; k < 3; ++k) {
        const R l6 = fabs(c[k + 1] - c[k]) * q.ls6;
        if (l6 > R(0) && l6 < INF) w += l6 * (R(2) * f[k] * g[k] + f[k] * g[k + 1] + f[k + 1] * g[k] + R(2) * f[k + 1] * g[k + 1]);
    }
    return ok ? w : R(0);
}

}  // namespace rayp
}  // namespace qdas
