// eikonal3.hip -- travel times through a sound-speed VOLUME and the delay tables sampled from them: qdas_eikonal3, qdas_eikonal3_tables.
//
// What the reference's bfEikonal asks of kern/msfm.m when the grid has three non-singleton dimensions (src/UltrasoundSystem.m:4251-4308): msfm3d with
// two arguments, first-order fast marching over the six neighbours of a node.  With s = 1 / max(c / dp, eps) the time across one cell and the smaller
// neighbour along each axis sorted t1 <= t2 <= t3 (absent: +inf), the value fast marching leaves at a node is the classical upwind one:
//     T = t1 + s;
//     if T > t2:  T = (t1 + t2 + sqrt(2 s^2 - (t1 - t2)^2)) / 2;
//     if that T > t3:  T = (t1 + t2 + t3 + sqrt(3 s^2 - (t1 - t2)^2 - (t1 - t3)^2 - (t2 - t3)^2)) / 3;
// and T = 0 at the (floored) source nodes.  (msfm3d itself puts ALL frozen neighbours into one quadratic and falls back to t1 + s when the root lies below
// one of them; that rule is not monotone, but a heap solver freezes nodes in ascending order and keeps the minimum of the candidates a node ever receives,
// which is the value above -- DESIGN.md 4.12.)  The classical update is monotone in its arguments, so T <- min(T, update(T)) applied in ANY order from
// T = +inf reaches the system's only fixed point.  Both discriminants are >= s^2 where their branch is taken, so the roots are well conditioned.
//
// Here: a block-based fast iterative method over an ACTIVE LIST.  A map is cut into tiles of 8 x 8 x 8 nodes; a workgroup of 512 threads loads one
// tile with a one-node FACE halo into LDS (10^3 doubles; the halo's edges and corners are never read) and applies the update to all of its nodes at once
// (Jacobi) at most ITERS times, stopping early when an application changes nothing.  A pass is ONE launch of a bounded grid that strides over the current
// list of (source set, tile) pairs, reading the list's length from device memory.  A tile whose last application still changed a node enlists itself
// for the next pass; a tile one of whose faces changed enlists the neighbour that reads that face as halo; a source on a tile face enlists that neighbour
// at seeding (up to three of them for a source in a tile corner).  Enlisting is atomicExch(flag, 1) == 0 followed by an integer atomicAdd on the next
// list's length, so a pair is on a list at most once and has one writer per pass.  The host reads the lengths back every CHUNK passes and stops at the first
// empty list: then every tile has seen an application that changed nothing with the halo values that are final -- the fixed point, not "change below a
// tolerance".  No floating-point atomics anywhere.
// What the concurrent halo read rests on: (a) values only fall; (b) whoever rewrites a face enlists its reader for the NEXT launch; (c) a map value is
// an aligned 8-byte word, loaded and stored as one transaction, so a reader sees the old or the new value, never a mix; (d) a value written in one pass
// is only RELIED on in a later launch -- kernel boundaries are the only point where one tile's writes must be visible to another.  Iterating passes
// inside one persistent kernel would break (d): the L2 of each XCD is not coherent with the others' within a launch.  So one pass = one launch.
//
// LDS: node (x, y, z) of the haloed tile at double index 100 z + 10 y + x.  A ds_read_b64 is served in two groups of 32 lanes = 4 rows of 8 nodes, at
// double indices r, 10 + r, 20 + r, 30 + r (r = 0 .. 7) plus a common offset; 32 double-wide banks make the fourth row's last six nodes share banks with
// the first row's: a 2-way conflict on 6 of 32 lanes, i.e. 3 LDS cycles per read instead of 2.  A row stride that avoids it (8 mod 32) would put the x halo
// elsewhere; the seven reads per application stand beside some forty fp64 operations and two barriers, so the layout stays the plain one.
//
// Work space (the CALLER's: this file constructs no arena and allocates nothing), every part 256-byte aligned:
//   head    visits (uint64: the sum of the list lengths of all passes, i.e. tile visits), then the CHUNK + 1 list lengths of one chunk of passes
//   flags   2 x K x tiles ints: "is on list A / B"
//   lists   2 x K x tiles (tile, set) pairs
//   points  npts (i, j, l, set) source nodes
// head and flags are zeroed by the call, the points uploaded, and of a list only the entries below its length are read: nothing the work space held
// before the call is read.
//
// The sampler is separable cubic convolution (Keys, a = -1/2) along dimension 1, then 2, then 3 (64 taps), NaN outside the grid
// (griddedInterpolant({g1, g2, g3}, T, 'cubic', 'none'), src/UltrasoundSystem.m:4298); the border rule and the Keys weights restate eikonal.hip's, which
// keeps its own: that file is not touched by this one.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "../../include/qdas.h"
#include "api_util.h"

namespace qdas {
namespace eik3 {

constexpr int TS = 8;               // tile side: TS^3 nodes, one per thread
constexpr int NT = TS * TS * TS;
constexpr int LS = TS + 2;          // side of the haloed tile in LDS
constexpr int ITERS = 24;           // applications of the update per visit of a tile (3 TS - 3 = 21 carry a front across the tile's diagonal)
constexpr int CHUNK = 8;            // passes between two reads of the list lengths
constexpr unsigned MAX_GRID = 2048; // workgroups of a pass (two of 512 threads fit a CU at <= 128 VGPRs: four rounds of 256 CUs)

struct Head {
    unsigned long long visits;
    uint32_t len[CHUNK + 1];        // len[q]: the list pass q of the chunk works off; pass q fills len[q + 1]
};

constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout {
    size_t flags, lists, points, bytes;
    Layout(size_t npairs, size_t npts) {
        flags = align256(sizeof(Head));
        lists = flags + align256(2 * npairs * sizeof(int));
        points = lists + align256(2 * npairs * sizeof(uint2));
        bytes = points + align256(npts * sizeof(uint4));
    }
};

__global__ void __launch_bounds__(256) fill_kernel(double *T, size_t n, double v) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) T[i] = v;
}

// put (tile, set k) on a list unless it is there already
__device__ inline void enlist(int *flag, uint2 *list, uint32_t *len, size_t pair, uint32_t tile, uint32_t k) {
    if (atomicExch(flag + pair, 1) == 0) list[atomicAdd(len, 1u)] = make_uint2(tile, k);
}

// pts: (i, j, l, source set) per source point
__global__ void __launch_bounds__(256) seed_kernel(const uint4 *pts, uint32_t npts, double *T, int *flag, uint2 *list, uint32_t *len,
                                                    uint32_t C1, uint32_t C2, uint32_t C3, uint32_t n1, uint32_t n2, uint32_t n3) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npts) return;
    const uint32_t i = pts[p].x, j = pts[p].y, l = pts[p].z, k = pts[p].w;
    T[(((size_t)k * C3 + l) * C2 + j) * C1 + i] = 0.0;
    const uint32_t a = i / TS, b = j / TS, c = l / TS, tile = (c * n2 + b) * n1 + a, plane = n1 * n2;
    const size_t at = (size_t)k * plane * n3 + tile;
    enlist(flag, list, len, at, tile, k);
    // a source on a tile's face is halo of the next tile, which nothing else would enlist (the source's own value never changes)
    if (i % TS == 0 && a > 0) enlist(flag, list, len, at - 1, tile - 1, k);
    if (i % TS == TS - 1 && a + 1 < n1) enlist(flag, list, len, at + 1, tile + 1, k);
    if (j % TS == 0 && b > 0) enlist(flag, list, len, at - n1, tile - n1, k);
    if (j % TS == TS - 1 && b + 1 < n2) enlist(flag, list, len, at + n1, tile + n1, k);
    if (l % TS == 0 && c > 0) enlist(flag, list, len, at - plane, tile - plane, k);
    if (l % TS == TS - 1 && c + 1 < n3) enlist(flag, list, len, at + plane, tile + plane, k);
}

// the classical first-order upwind update of one node from the smaller neighbour along each axis (absent: +inf)
__device__ inline double update(double a, double b, double c, double s) {
    const double lo = fmin(a, b), hi = fmax(a, b);
    const double t1 = fmin(lo, c), t2 = fmax(lo, fmin(hi, c)), t3 = fmax(hi, c);
    double v = t1 + s;
    if (v > t2) {                                       // (false for an absent t2; then s > t2 - t1 and the discriminant exceeds s^2)
        const double d12 = t1 - t2;
        v = 0.5 * (t1 + t2 + sqrt(2.0 * s * s - d12 * d12));
        if (v > t3) {                                   // (the discriminant is >= s^2 here as well: file head)
            const double d13 = t1 - t3, d23 = t2 - t3;
            v = (t1 + t2 + t3 + sqrt(3.0 * s * s - d12 * d12 - d13 * d13 - d23 * d23)) * (1.0 / 3.0);
        }
    }
    return v;
}

// pass q of a chunk: works off the list lcur of h->len[q] pairs, fills lnext / h->len[q + 1]
__global__ void __launch_bounds__(NT) pass_kernel(const double *__restrict__ c, double *T, int *fcur, int *fnext, const uint2 *lcur, uint2 *lnext, Head *h, int q,
                                                   uint32_t C1, uint32_t C2, uint32_t C3, uint32_t n1, uint32_t n2, uint32_t n3, double dp) {
    __shared__ double t[LS * LS * LS];
    __shared__ int faces;
    const int tid = threadIdx.x, lx = tid % TS, ly = (tid / TS) % TS, lz = tid / (TS * TS);
    const uint32_t n = h->len[q];
    uint32_t *len_next = h->len + q + 1;
    if (blockIdx.x == 0 && tid == 0) h->visits += n;     // (one writer per launch)
    const uint32_t plane = n1 * n2;
    const size_t ntiles = (size_t)plane * n3, CC = (size_t)C1 * C2 * C3;
    const double inf = INFINITY;
    const int me = (lz + 1) * LS * LS + (ly + 1) * LS + lx + 1;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint32_t tile = lcur[e].x, k = lcur[e].y;
        const size_t pair = (size_t)k * ntiles + tile;
        if (tid == 0) { fcur[pair] = 0; faces = 0; }
        const uint32_t a = tile % n1, b = (tile / n1) % n2, cc = tile / plane;
        const int64_t i0 = (int64_t)a * TS, j0 = (int64_t)b * TS, l0 = (int64_t)cc * TS;
        double *Tk = T + (size_t)k * CC;
        auto at = [&](int64_t i, int64_t j, int64_t l) -> double {
            return (i >= 0 && j >= 0 && l >= 0 && i < (int64_t)C1 && j < (int64_t)C2 && l < (int64_t)C3) ? Tk[((size_t)l * C2 + (size_t)j) * C1 + (size_t)i] : inf;
        };
        const int64_t gi = i0 + lx, gj = j0 + ly, gl = l0 + lz;
        const bool in = gi < (int64_t)C1 && gj < (int64_t)C2 && gl < (int64_t)C3;
        const size_t node = ((size_t)gl * C2 + (size_t)gj) * C1 + (size_t)gi;
        const double first = at(gi, gj, gl);
        t[me] = first;
        if (tid < 6 * TS * TS) {                        // the halo: six faces of TS x TS nodes
            const int f = tid / (TS * TS), u = tid % TS, v = (tid / TS) % TS;
            if (f == 0) t[(v + 1) * LS * LS + (u + 1) * LS] = at(i0 - 1, j0 + u, l0 + v);
            else if (f == 1) t[(v + 1) * LS * LS + (u + 1) * LS + TS + 1] = at(i0 + TS, j0 + u, l0 + v);
            else if (f == 2) t[(v + 1) * LS * LS + u + 1] = at(i0 + u, j0 - 1, l0 + v);
            else if (f == 3) t[(v + 1) * LS * LS + (TS + 1) * LS + u + 1] = at(i0 + u, j0 + TS, l0 + v);
            else if (f == 4) t[(v + 1) * LS + u + 1] = at(i0 + u, j0 + v, l0 - 1);
            else t[(TS + 1) * LS * LS + (v + 1) * LS + u + 1] = at(i0 + u, j0 + v, l0 + TS);
        }
        const double s = in ? 1.0 / fmax(c[node] / dp, DBL_EPSILON) : inf;      // (msfm3d: 1 / max(F, eps))
        __syncthreads();
        double cur = first;
        int last = 0;
        for (int it = 0; it < ITERS; ++it) {
            double nv = cur;
            if (in) nv = fmin(cur, update(fmin(t[me - 1], t[me + 1]), fmin(t[me - LS], t[me + LS]), fmin(t[me - LS * LS], t[me + LS * LS]), s));
            last = __syncthreads_or(nv < cur);           // (every neighbour has been read)
            if (!last) break;
            cur = nv;
            t[me] = cur;
            __syncthreads();
        }
        const bool ch = cur < first;
        if (ch) {
            Tk[node] = cur;
            const int bits = (lx == 0) | (lx == TS - 1) << 1 | (ly == 0) << 2 | (ly == TS - 1) << 3 | (lz == 0) << 4 | (lz == TS - 1) << 5;
            if (bits) atomicOr(&faces, bits);
        }
        __syncthreads();
        if (tid < 7) {                                  // thread 0: the tile itself; threads 1 .. 6: the neighbour behind face tid - 1
            const int fc = faces;
            bool go = false;
            int64_t step = 0;
            if (tid == 0) go = last != 0;
            else if (tid == 1) { go = (fc & 1) && a > 0; step = -1; }
            else if (tid == 2) { go = (fc & 2) && a + 1 < n1; step = 1; }
            else if (tid == 3) { go = (fc & 4) && b > 0; step = -(int64_t)n1; }
            else if (tid == 4) { go = (fc & 8) && b + 1 < n2; step = n1; }
            else if (tid == 5) { go = (fc & 16) && cc > 0; step = -(int64_t)plane; }
            else { go = (fc & 32) && cc + 1 < n3; step = plane; }
            if (go) enlist(fnext, lnext, len_next, (size_t)((int64_t)pair + step), (uint32_t)((int64_t)tile + step), k);
        }
        __syncthreads();                                // (t and faces are reused by the next pair)
    }
}

// ---- sampler
// Node i of a line of C nodes extended by one ghost node on either side, as a sum of `count` terms coef(m) f(first + m step), taken in the order of m.
// A node of the line is itself.  A ghost node is Keys' own boundary condition f(-1) = 3 f(0) - 3 f(1) + f(2) (the far side by symmetry); a line of two
// nodes continues linearly, 2 f(0) - f(1); a single node is constant (the ASSUMPTION of DESIGN.md 4.6, as eikonal.hip's ghost(): change it here).
struct Terms {
    int64_t first;
    int step, count;
    bool ghost;
};
__device__ inline Terms terms(int64_t i, uint32_t C) {
    if (i >= 0 && i < (int64_t)C) return {i, 0, 1, false};
    const bool lo = i < 0;
    return {lo ? 0 : (int64_t)C - 1, lo ? 1 : -1, C >= 3 ? 3 : (int)C, true};
}
__device__ inline double coef(const Terms &t, int m) {
    if (!t.ghost || t.count == 1) return 1.0;
    if (t.count == 2) return m == 0 ? 2.0 : -1.0;
    return m == 0 ? 3.0 : (m == 1 ? -3.0 : 1.0);
}

// a node of the map extended by one ghost node on every side: along dimension 1 first, then 2, then 3 (one copy of the loops, not unrolled: a corner
// ghost node is 27 loads, an inner node one, and the kernel stays at a few dozen registers)
__device__ inline double ext3(const double *T, const Terms &t1, const Terms &t2, const Terms &t3, uint32_t C1, uint32_t C2) {
    double v3 = 0.0;
#pragma unroll 1
    for (int m3 = 0; m3 < t3.count; ++m3) {
        double v2 = 0.0;
#pragma unroll 1
        for (int m2 = 0; m2 < t2.count; ++m2) {
            const double *col = T + ((size_t)(t3.first + m3 * t3.step) * C2 + (size_t)(t2.first + m2 * t2.step)) * C1;
            double v1 = 0.0;
#pragma unroll 1
            for (int m1 = 0; m1 < t1.count; ++m1) v1 += coef(t1, m1) * col[t1.first + m1 * t1.step];
            v2 += coef(t2, m2) * v1;
        }
        v3 += coef(t3, m3) * v2;
    }
    return v3;
}

// cell and fraction of coordinate u on a line of C nodes; false: outside (or NaN)
__device__ inline bool cell(double u, uint32_t C, int64_t &i0, double &f) {
    if (!(u >= 0.0 && u <= (double)(C - 1))) return false;
    double fl = floor(u);
    if (C >= 2 && fl > (double)(C - 2)) fl = (double)(C - 2);       // the last node belongs to the last cell (f = 1)
    f = u - fl;
    i0 = (int64_t)fl;
    return true;
}

// Keys weight of tap a = 0 .. 3 (node i0 - 1 + a) at fraction f
__device__ inline double keys(double f, int a) {
    const double f2 = f * f, f3 = f2 * f;
    return a == 0 ? -0.5 * f3 + f2 - 0.5 * f : (a == 1 ? 1.5 * f3 - 2.5 * f2 + 1.0 : (a == 2 ? -1.5 * f3 + 2.0 * f2 + 0.5 * f : 0.5 * f3 - 0.5 * f2));
}

__global__ void __launch_bounds__(256) tables_kernel(const double *__restrict__ T, const double *__restrict__ Pi, double *__restrict__ tau,
                                                      uint64_t I, uint32_t C1, uint32_t C2, uint32_t C3, double base) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= I) return;
    const uint32_t k = blockIdx.y;
    const double *Tk = T + (size_t)k * C1 * C2 * C3;
    int64_t i0 = 0, j0 = 0, l0 = 0;
    double fu = 0.0, fv = 0.0, fw = 0.0;
    double v = NAN;
    if (cell(Pi[3 * p] - base, C1, i0, fu) && cell(Pi[3 * p + 1] - base, C2, j0, fv) && cell(Pi[3 * p + 2] - base, C3, l0, fw)) {
        v = 0.0;
#pragma unroll 1
        for (int cz = 0; cz < 4; ++cz) {
            const double wz = keys(fw, cz);
            if (wz == 0.0) continue;                    // (a pixel on a grid plane reads that plane alone: weights 0, 1, 0, 0)
            const Terms t3 = terms(l0 - 1 + cz, C3);
            double gz = 0.0;
#pragma unroll 1
            for (int b = 0; b < 4; ++b) {
                const double wy = keys(fv, b);
                if (wy == 0.0) continue;
                const Terms t2 = terms(j0 - 1 + b, C2);
                double g = 0.0;
#pragma unroll 1
                for (int a = 0; a < 4; ++a) {
                    const double wx = keys(fu, a);
                    if (wx != 0.0) g += wx * ext3(Tk, terms(i0 - 1 + a, C1), t2, t3, C1, C2);
                }
                gz += wy * g;
            }
            v += wz * gz;
        }
    }
    tau[(size_t)k * I + p] = v;
}

}  // namespace eik3
}  // namespace qdas

using qdas::fail;
using qdas::DeviceGuard;

extern "C" uint32_t qdas_eikonal3_pass_cap(uint64_t C1, uint64_t C2, uint64_t C3) {
    const uint64_t cap = 8 * (C1 + C2 + C3) + 64;
    return cap > 0x7fffffffull ? 0x7fffffffu : (uint32_t)cap;
}

static uint64_t eik3_tiles(const qdas_eikonal3_desc *d) {
    return ((d->C1 + 7) / 8) * ((d->C2 + 7) / 8) * ((d->C3 + 7) / 8);
}

static int eik3_check_grid(const qdas_eikonal3_desc *d) {
    if (!d) return fail(QDAS_EINVAL, "eikonal3: null descriptor");
    if (d->C1 >= (1ull << 31) || d->C2 >= (1ull << 31) || d->C3 >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "eikonal3: at most 2^31 - 1 nodes per dimension");
    if (d->K > 65535) return fail(QDAS_EUNSUPPORTED, "eikonal3: at most 65535 source sets per call");
    // (each factor is below 2^28, so the test cannot wrap: the product of two is checked first)
    if (((d->C1 + 7) / 8) * ((d->C2 + 7) / 8) >= (1ull << 24) || eik3_tiles(d) >= (1ull << 24))
        return fail(QDAS_EUNSUPPORTED, "eikonal3: at most 2^24 - 1 tiles of 8 x 8 x 8 nodes per map");
    if (d->base != 0 && d->base != 1) return fail(QDAS_EINVAL, "eikonal3: coordinates are 0- or 1-based");
    return QDAS_OK;
}

static int eik3_check_solve(const qdas_eikonal3_desc *d) {
    if (int rc = eik3_check_grid(d)) return rc;
    if (d->set_begin ? false : d->npts != d->K) return fail(QDAS_EINVAL, "eikonal3: without set_begin every source set is one point (npts == K)");
    if (d->npts >= (1ull << 32)) return fail(QDAS_EUNSUPPORTED, "eikonal3: at most 2^32 - 1 source points per call");
    if (!(d->dp > 0.0) || !std::isfinite(d->dp)) return fail(QDAS_EINVAL, "eikonal3: the grid step must be positive");
    return QDAS_OK;
}

extern "C" int qdas_eikonal3_work_bytes(const qdas_eikonal3_desc *d, uint64_t *bytes) {
    if (!bytes) return fail(QDAS_EINVAL, "eikonal3: null pointer for the work space size");
    *bytes = 0;
    if (int rc = eik3_check_solve(d)) return rc;
    if (d->C1 * d->C2 * d->C3 == 0 || d->K == 0) return QDAS_OK;
    *bytes = qdas::eik3::Layout(d->K * eik3_tiles(d), d->npts).bytes;
    return QDAS_OK;
}

extern "C" int qdas_eikonal3(const qdas_eikonal3_desc *d, const double *c, const double *src, double *T, void *work, uint64_t work_bytes, uint32_t *passes) {
    using namespace qdas::eik3;
    if (passes) *passes = 0;
    if (int rc = eik3_check_solve(d)) return rc;
    const uint64_t CC = d->C1 * d->C2 * d->C3;
    if (CC == 0 || d->K == 0) return QDAS_OK;            // an empty grid or no sources: nothing is launched
    if (!c || !src || !T || !work) return fail(QDAS_EINVAL, "eikonal3: null data pointer");
    const uint32_t C1 = (uint32_t)d->C1, C2 = (uint32_t)d->C2, C3 = (uint32_t)d->C3, K = (uint32_t)d->K;
    // source points: floored to a node, every one inside the grid (kern/msfm.m:96-99)
    std::vector<uint4> pts;
    pts.reserve(d->npts);
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t b = d->set_begin ? d->set_begin[k] : k, e = d->set_begin ? d->set_begin[k + 1] : k + 1;
        if (e < b || e > d->npts) return fail(QDAS_EINVAL, "eikonal3: set_begin must ascend and end at npts");
        if (e == b) return fail(QDAS_EINVAL, "eikonal3: a source set is empty");
        for (uint64_t p = b; p < e; ++p) {
            const double u = src[3 * p] - d->base, v = src[3 * p + 1] - d->base, w = src[3 * p + 2] - d->base;
            if (!(u >= 0.0 && v >= 0.0 && w >= 0.0 && u <= (double)(C1 - 1) && v <= (double)(C2 - 1) && w <= (double)(C3 - 1)))
                return fail(QDAS_EINVAL, "eikonal3: a source point lies outside the grid");
            pts.push_back(make_uint4((uint32_t)floor(u), (uint32_t)floor(v), (uint32_t)floor(w), k));
        }
    }
    const uint32_t n1 = (C1 + TS - 1) / TS, n2 = (C2 + TS - 1) / TS, n3 = (C3 + TS - 1) / TS;
    const size_t npairs = (size_t)K * n1 * n2 * n3;
    const Layout lay(npairs, pts.size());
    if (work_bytes < lay.bytes) return fail(QDAS_EINVAL, "eikonal3: the work space is too small (%llu bytes, qdas_eikonal3_work_bytes asks for %llu)", (unsigned long long)work_bytes, (unsigned long long)lay.bytes);
    if ((uintptr_t)work % 16) return fail(QDAS_EINVAL, "eikonal3: the work space must be aligned to 16 bytes");
    const uint32_t cap = d->max_passes ? d->max_passes : qdas_eikonal3_pass_cap(C1, C2, C3);
    DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)d->queue;
    char *ws = (char *)work;
    Head *head = (Head *)ws;
    int *flags = (int *)(ws + lay.flags);
    uint2 *lists = (uint2 *)(ws + lay.lists);
    uint4 *dpts = (uint4 *)(ws + lay.points);
    auto hip_fail = [&](hipError_t e) { (void)hipStreamSynchronize(s); return fail(QDAS_EHIP, "%s", hipGetErrorString(e)); };
    hipError_t e = hipMemsetAsync(ws, 0, lay.flags + 2 * npairs * sizeof(int), s);
    if (e == hipSuccess) e = hipMemcpyAsync(dpts, pts.data(), pts.size() * sizeof(uint4), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e);
    const size_t ntot = (size_t)K * CC;
    fill_kernel<<<(unsigned)std::min<size_t>((ntot + 255) / 256, 65536), 256, 0, s>>>(T, ntot, INFINITY);
    seed_kernel<<<(unsigned)((pts.size() + 255) / 256), 256, 0, s>>>(dpts, (uint32_t)pts.size(), T, flags, lists, head->len, C1, C2, C3, n1, n2, n3);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
    const unsigned grid = (unsigned)std::min<size_t>(npairs, MAX_GRID);
    uint32_t done = 0;
    bool converged = false;
    uint32_t host_len[CHUNK];
    while (done < cap && !converged) {
        const uint32_t n = std::min<uint32_t>(CHUNK, cap - done);
        if (done) {                                      // the chunk's lengths are reused: the list the last pass filled becomes list 0, the others empty
            e = hipMemcpyAsync(head->len, head->len + CHUNK, sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemsetAsync(head->len + 1, 0, CHUNK * sizeof(uint32_t), s);
            if (e != hipSuccess) return hip_fail(e);
        }
        for (uint32_t q = 0; q < n; ++q) {
            const uint32_t p = done + q, cur = p & 1, nxt = cur ^ 1;
            pass_kernel<<<grid, NT, 0, s>>>(c, T, flags + cur * npairs, flags + nxt * npairs, lists + cur * npairs, lists + nxt * npairs, head, (int)q,
                                            C1, C2, C3, n1, n2, n3, d->dp);
        }
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
        e = hipMemcpyAsync(host_len, head->len + 1, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
        for (uint32_t q = 0; q < n && !converged; ++q)
            if (host_len[q] == 0) { converged = true; if (passes) *passes = done + q + 1; }
        done += n;
    }
    if (!converged) {                                    // never an unconverged map: the output is NaN and the call fails
        if (passes) *passes = done;
        fill_kernel<<<(unsigned)std::min<size_t>((ntot + 255) / 256, 65536), 256, 0, s>>>(T, ntot, NAN);
        (void)hipStreamSynchronize(s);
        return fail(QDAS_ENOCONV, "eikonal3: no fixed point within %u passes (the maps are set to NaN)", cap);
    }
    return QDAS_OK;
}

extern "C" int qdas_eikonal3_tables(const qdas_eikonal3_desc *d, const double *T, const double *Pi, double *tau) {
    using namespace qdas::eik3;
    if (int rc = eik3_check_grid(d)) return rc;
    if (d->I > 0xffffff00ull) return fail(QDAS_EUNSUPPORTED, "eikonal3: at most 2^32 - 256 pixels per call (one launch covers them)");
    if (d->I == 0 || d->K == 0) return QDAS_OK;
    if (d->C1 * d->C2 * d->C3 == 0) return fail(QDAS_EINVAL, "eikonal3: tables of an empty grid");
    if (!T || !Pi || !tau) return fail(QDAS_EINVAL, "eikonal3: null data pointer");
    DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    tables_kernel<<<dim3((unsigned)((d->I + 255) / 256), (unsigned)d->K), 256, 0, (hipStream_t)d->queue>>>(T, Pi, tau, d->I, (uint32_t)d->C1, (uint32_t)d->C2, (uint32_t)d->C3, (double)d->base);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
