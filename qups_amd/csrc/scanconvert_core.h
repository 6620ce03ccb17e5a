// scanconvert_core.h -- one output pixel of the scan conversion of scanconvert.hip: the Cartesian point's polar / spherical coordinates, the cell search on
// the source axes, `pre` on the corner samples and the lerps.  Plain C++ with no HIP in it: the same text compiles for the host, where
// tests/scanconvert_core_host.cpp runs it on the CPU under the sanitizers (bounds and results, no device needed).
//
// Geometry is float64 whatever the data: rho = hypot(dz, dx), alpha = atan2(dx, dz) (cart2pol(Z - oz, X - ox)); for a volume rho = sqrt(dx^2 + dy^2 + dz^2),
// alpha = atan2(dx, dz), eps = atan2(dy, hypot(dz, dx)) (cart2sph).  A coordinate p is INSIDE an axis g[0 .. n-1] iff g[0] <= p <= g[n-1] -- both ends closed,
// a NaN is outside; its cell is the largest k <= n - 2 with g[k] <= p, its weight (p - g[k]) / (g[k+1] - g[k]): a point on the last node has the last cell
// and the weight 1.  The weights are rounded to the data's real type R and the lerps run in R, along r first, then a, then e:
//   lo = b[k, l] + u (b[k+1, l] - b[k, l]);  hi = b[k, l+1] + u (b[k+1, l+1] - b[k, l+1]);  out = lo + v (hi - lo)
// so non-finite samples follow IEEE rules (a NaN corner gives NaN even under a zero weight).  `pre` acts on the corner samples BEFORE the lerps:
// PRE_ABS |b|, PRE_DB 20 log10 |b| raised to db_floor (a NaN stays a NaN); both give a real value.
//
// The cell search never leaves the axis whatever it holds: the bisection halves an integer interval, the uniform guess is clamped before it becomes an
// integer and is checked against the actual nodes.  With a repeated node (the caller broke its promise) the weight is Inf or NaN, the indices are not.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QDAS_SC_HD __host__ __device__ inline
#else
#define QDAS_SC_HD inline
#endif

namespace qdas {
namespace sc {

enum { PRE_NONE = 0, PRE_ABS = 1, PRE_DB = 2 };

// ---- the axes
// the largest k in [0, n - 2] with g[k] <= p, for g[0] <= p (n >= 2): at most 32 halvings of an integer interval
QDAS_SC_HD int bisect(const double *g, int n, double p) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32; ++it) {
        if (hi - lo <= 1) break;
        const int mid = (lo + hi) >> 1;
        if (g[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// the pitch an axis would have if it were uniform, and whether node i (of value gi) lies within a quarter of it of its place: when every node does, the
// guess floor((p - g[0]) / pitch) is at most one cell off.  A NaN anywhere says no.
QDAS_SC_HD double pitch_of(double g0, double glast, int n) { return (glast - g0) / (double)(n - 1); }
QDAS_SC_HD bool on_pitch(double gi, double g0, int i, double pitch) { return fabs(gi - (g0 + (double)i * pitch)) <= 0.25 * pitch; }
// 1 / pitch when the axis may take the O(1) path, else 0 (= bisect)
QDAS_SC_HD double inv_pitch(double pitch, bool uniform) { return (uniform && pitch > 0.0 && pitch < (double)INFINITY) ? 1.0 / pitch : 0.0; }

// the cell of an INSIDE coordinate.  inv > 0: guess from the constant pitch, correct the guess against the nodes a step or two either way, and bisect when
// it is further off; inv = 0: bisect.  Either way the result is the cell `bisect` names on the actual vector.
QDAS_SC_HD int cell_of(const double *g, int n, double p, double inv) {
    if (inv > 0.0) {
        double t = (p - g[0]) * inv;
        t = t > 0.0 ? t : 0.0;                                  // (a NaN becomes 0)
        t = t < (double)(n - 2) ? t : (double)(n - 2);
        int k = (int)t;
        for (int s = 0; s < 2; ++s) {
            if (k > 0 && g[k] > p) --k;
            else if (k < n - 2 && g[k + 1] <= p) ++k;
        }
        if (g[k] <= p && (k == n - 2 || p < g[k + 1])) return k;
    }
    return bisect(g, n, p);
}

// inside test, cell and weight of one coordinate on one axis; outside: false, k = 0, w = 0
QDAS_SC_HD bool locate(const double *g, int n, double p, double inv, int &k, double &w) {
    k = 0;
    w = 0.0;
    if (!(g[0] <= p && p <= g[n - 1])) return false;
    k = cell_of(g, n, p, inv);
    w = (p - g[k]) / (g[k + 1] - g[k]);
    return true;
}

QDAS_SC_HD void polar_of(double dz, double dx, double &rho, double &alpha) {
    rho = hypot(dz, dx);
    alpha = atan2(dx, dz);
}
QDAS_SC_HD void spherical_of(double dz, double dx, double dy, double &rho, double &alpha, double &eps) {
    rho = sqrt(dx * dx + dy * dy + dz * dz);
    alpha = atan2(dx, dz);
    eps = atan2(dy, hypot(dz, dx));
}

// ---- the values
template <typename R> struct alignas(2 * sizeof(R)) Cx { R re, im; };          // one complex sample: a single 8- or 16-byte load / store

QDAS_SC_HD float mag2(float re, float im) { return hypotf(re, im); }
QDAS_SC_HD double mag2(double re, double im) { return hypot(re, im); }
QDAS_SC_HD float lg10(float v) { return log10f(v); }
QDAS_SC_HD double lg10(double v) { return log10(v); }
template <typename R> QDAS_SC_HD R to_db(R m, R db_floor) {
    const R v = R(20) * lg10(m);
    return v < db_floor ? db_floor : v;                          // (not fmax: a NaN stays)
}

// the type of a corner sample after `pre`, which is the type of the output
template <typename R, bool CPLX, int PRE> struct Value { using T = R; };
template <typename R> struct Value<R, true, PRE_NONE> { using T = Cx<R>; };

template <typename R> QDAS_SC_HD R lerp(R a, R b, R t) { return a + t * (b - a); }
template <typename R> QDAS_SC_HD Cx<R> lerp(Cx<R> a, Cx<R> b, R t) {
    Cx<R> o;
    o.re = a.re + t * (b.re - a.re);
    o.im = a.im + t * (b.im - a.im);
    return o;
}

// sample `idx` (in elements: complex samples when CPLX) of b, after `pre`
template <typename R, bool CPLX, int PRE> QDAS_SC_HD typename Value<R, CPLX, PRE>::T corner(const void *b, int64_t idx, R db_floor) {
    if constexpr (CPLX) {
        const Cx<R> c = ((const Cx<R> *)b)[idx];
        if constexpr (PRE == PRE_NONE) return c;
        else if constexpr (PRE == PRE_ABS) return mag2(c.re, c.im);
        else return to_db(mag2(c.re, c.im), db_floor);
    } else {
        const R c = ((const R *)b)[idx];
        if constexpr (PRE == PRE_NONE) return c;
        else if constexpr (PRE == PRE_ABS) return (R)fabs(c);
        else return to_db((R)fabs(c), db_floor);
    }
}

template <typename R, bool CPLX, int PRE> QDAS_SC_HD typename Value<R, CPLX, PRE>::T filled(R fill) {
    if constexpr (CPLX && PRE == PRE_NONE) {
        Cx<R> o;
        o.re = fill;
        o.im = R(0);
        return o;
    } else return fill;
}

// three lerps in the cell whose first corner is sample o: along r (stride sr), then along a (stride sa)
template <typename R, bool CPLX, int PRE>
QDAS_SC_HD typename Value<R, CPLX, PRE>::T bilerp(const void *b, int64_t o, int64_t sr, int64_t sa, R u, R v, R db_floor) {
    const auto lo = lerp(corner<R, CPLX, PRE>(b, o, db_floor), corner<R, CPLX, PRE>(b, o + sr, db_floor), u);
    const auto hi = lerp(corner<R, CPLX, PRE>(b, o + sa, db_floor), corner<R, CPLX, PRE>(b, o + sa + sr, db_floor), u);
    return lerp(lo, hi, v);
}

// seven lerps: four along r, two along a, one along e (stride se)
template <typename R, bool CPLX, int PRE>
QDAS_SC_HD typename Value<R, CPLX, PRE>::T trilerp(const void *b, int64_t o, int64_t sr, int64_t sa, int64_t se, R u, R v, R w, R db_floor) {
    const auto near = bilerp<R, CPLX, PRE>(b, o, sr, sa, u, v, db_floor);
    const auto far = bilerp<R, CPLX, PRE>(b, o + se, sr, sa, u, v, db_floor);
    return lerp(near, far, w);
}

}  // namespace sc
}  // namespace qdas
