// eikonal.hip -- travel times through a sound-speed map and the delay tables sampled from them: qdas_eikonal, qdas_eikonal_tables.
//
// What the reference's bfEikonal asks of kern/msfm.m with two arguments (src/UltrasoundSystem.m:4295-4308): first-order fast marching over the four
// neighbours of a node.  With a, b the smaller neighbour along each axis and s = 1 / max(c / dp, eps) the time across one cell,
//     T = min(a, b) + s                              if |a - b| >= s or one of them is absent,
//     T = (a + b + sqrt(2 s^2 - (a - b)^2)) / 2      otherwise,
// and T = 0 at the (floored) source nodes.  Fast marching is one way to solve that system; its solution is the system's only fixed point, and the
// update is monotone, so T <- min(T, update(T)) applied in ANY order from T = +inf reaches the same numbers.  Here: a block-based fast iterative
// method.  The map is cut into TS x TS tiles; a workgroup loads one tile with a one-node halo into LDS and applies the update to all of its
// nodes at once (Jacobi) at most ITERS times, stopping early when an application changes nothing.  One int per (source set, tile) says whether the tile must
// be visited in the next pass: a tile whose last application still changed a node flags itself, a tile whose edge row / column changed flags the
// neighbour that reads it as halo.  All source sets are solved by the same launches (blockIdx.y), sharing the speed map.  Values only fall, so a
// neighbour that is being rewritten while its halo is read does no harm: whoever rewrites an edge flags its reader for the next pass.  The host
// reads the per-pass activation counters back every few passes and stops at the first pass that flagged nothing: then every tile has seen an
// application that changed nothing with the halo values that are final -- the fixed point, not "change below a tolerance".
// No floating-point atomics; the flags are plain stores of 1, the counters integer atomics.
// What the concurrent halo read rests on: (a) values only fall; (b) whoever rewrites an edge flags its reader for the NEXT launch; (c) a map value is
// an aligned 8-byte word, loaded and stored as one transaction, so a reader sees the old or the new value, never a mix; (d) a value written in one pass
// is only RELIED on in a later launch -- kernel boundaries are the only point where one tile's writes must be visible to another.  Iterating passes
// inside one persistent kernel would break (d): the L2 of each XCD is not coherent with the others' within a launch.
//
// The sampler is separable cubic convolution (Keys, a = -1/2) of a map at fractional grid coordinates, NaN outside the grid
// (griddedInterpolant(grd, T, 'cubic', 'none'), src/UltrasoundSystem.m:4291); the border rule lives in one function, ghost().
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/qdas.h"
#include "api_util.h"
#include "qdas_kernels.h"

namespace qdas {
namespace eik {

constexpr int TS = 16;              // tile side: TS x TS nodes, one per thread
constexpr int ITERS = 32;           // applications of the update per visit of a tile (2 TS - 2 carry a front across the tile's diagonal)
constexpr int CHUNK = 4;            // passes between two reads of the counters

__global__ void __launch_bounds__(256) fill_kernel(double *T, size_t n, double v) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) T[i] = v;
}

// pts: (node index within a map, source set) per source point
__global__ void __launch_bounds__(256) seed_kernel(const uint2 *pts, uint32_t npts, double *T, int *flags, uint32_t C1, uint32_t C2, uint32_t tiles1, uint32_t ntiles) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npts) return;
    const uint32_t node = pts[p].x, k = pts[p].y;
    T[(size_t)k * C1 * C2 + node] = 0.0;
    const uint32_t i = node % C1, j = node / C1;
    int *f = flags + (size_t)k * ntiles;
    const uint32_t t1 = i / TS, t2 = j / TS, tile = t2 * tiles1 + t1, tiles2 = ntiles / tiles1;
    f[tile] = 1;
    // a source on a tile's edge is halo of the next tile, which nothing else would flag (the source's own value never changes)
    if (i % TS == 0 && t1 > 0) f[tile - 1] = 1;
    if (i % TS == TS - 1 && t1 + 1 < tiles1) f[tile + 1] = 1;
    if (j % TS == 0 && t2 > 0) f[tile - tiles1] = 1;
    if (j % TS == TS - 1 && t2 + 1 < tiles2) f[tile + tiles1] = 1;
}

// the first-order update of one node from its four neighbours (absent: +inf)
__device__ inline double update(double l, double r, double u, double d, double s) {
    const double a = fmin(l, r), b = fmin(u, d);
    const double lo = fmin(a, b), hi = fmax(a, b);
    if (hi - lo < s) return 0.5 * (a + b + sqrt(2.0 * s * s - (a - b) * (a - b)));   // (false for an absent side and for inf - inf)
    return lo + s;
}

__global__ void __launch_bounds__(TS * TS) pass_kernel(const double *__restrict__ c, double *T, int *fin, int *fout, int *counter,
                                                        uint32_t C1, uint32_t C2, uint32_t tiles1, uint32_t tiles2, double dp) {
    __shared__ double t[TS + 2][TS + 2];
    __shared__ int act;
    const uint32_t tile = blockIdx.x, k = blockIdx.y, ntiles = tiles1 * tiles2;
    const int tid = threadIdx.x, lx = tid % TS, ly = tid / TS;
    int *mine = fin + (size_t)k * ntiles + tile;
    if (tid == 0) { act = *mine; *mine = 0; }
    __syncthreads();
    if (!act) return;
    const uint32_t t1 = tile % tiles1, t2 = tile / tiles1;
    const int64_t i0 = (int64_t)t1 * TS, j0 = (int64_t)t2 * TS;
    double *Tk = T + (size_t)k * C1 * C2;
    const double inf = INFINITY;
    auto at = [&](int64_t i, int64_t j) -> double { return (i >= 0 && j >= 0 && i < (int64_t)C1 && j < (int64_t)C2) ? Tk[(size_t)j * C1 + (size_t)i] : inf; };
    const int64_t gi = i0 + lx, gj = j0 + ly;
    const bool in = gi < (int64_t)C1 && gj < (int64_t)C2;
    const double first = at(gi, gj);
    t[ly + 1][lx + 1] = first;
    if (tid < 4 * TS) {                                 // the halo: four edges of TS nodes (the corners are never read)
        const int e = tid / TS, q = tid % TS;
        if (e == 0) t[q + 1][0] = at(i0 - 1, j0 + q);
        else if (e == 1) t[q + 1][TS + 1] = at(i0 + TS, j0 + q);
        else if (e == 2) t[0][q + 1] = at(i0 + q, j0 - 1);
        else t[TS + 1][q + 1] = at(i0 + q, j0 + TS);
    }
    const double s = in ? 1.0 / fmax(c[(size_t)gj * C1 + (size_t)gi] / dp, DBL_EPSILON) : inf;   // (kern/msfm2d.m: 1 / max(F, eps))
    __syncthreads();
    double cur = first;
    int last = 0;
    for (int it = 0; it < ITERS; ++it) {
        double nv = cur;
        if (in) nv = fmin(cur, update(t[ly + 1][lx], t[ly + 1][lx + 2], t[ly][lx + 1], t[ly + 2][lx + 1], s));
        last = __syncthreads_or(nv < cur);               // (every neighbour has been read)
        if (!last) break;
        cur = nv;
        t[ly + 1][lx + 1] = cur;
        __syncthreads();
    }
    const bool ch = cur < first;
    if (ch) Tk[(size_t)gj * C1 + (size_t)gi] = cur;
    const int w = __syncthreads_or(ch && lx == 0), e = __syncthreads_or(ch && lx == TS - 1);
    const int n = __syncthreads_or(ch && ly == 0), so = __syncthreads_or(ch && ly == TS - 1);
    if (tid == 0) {
        int *f = fout + (size_t)k * ntiles;
        int cnt = 0;
        if (last) { f[tile] = 1; ++cnt; }
        if (w && t1 > 0) { f[tile - 1] = 1; ++cnt; }
        if (e && t1 + 1 < tiles1) { f[tile + 1] = 1; ++cnt; }
        if (n && t2 > 0) { f[tile - tiles1] = 1; ++cnt; }
        if (so && t2 + 1 < tiles2) { f[tile + tiles1] = 1; ++cnt; }
        if (cnt) atomicAdd(counter, cnt);
    }
}

// ---- sampler
// The value one node outside a line of C nodes, f(-1) from f(0), f(1), f(2) (the far side by symmetry).  Keys' own boundary condition
// f(-1) = 3 f(0) - 3 f(1) + f(2); a line of two nodes continues linearly, a single node is constant.  This is an ASSUMPTION about what
// griddedInterpolant's 'cubic' does in the outermost cell: change it here.
__device__ inline double ghost(double f0, double f1, double f2, uint32_t C) {
    return C >= 3 ? 3.0 * f0 - 3.0 * f1 + f2 : (C == 2 ? 2.0 * f0 - f1 : f0);
}

// node (i, j) of the map extended by one ghost node on every side
__device__ inline double ext1(const double *col, int64_t i, uint32_t C1) {
    if (i >= 0 && i < (int64_t)C1) return col[i];
    const bool lo = i < 0;
    const double f0 = lo ? col[0] : col[C1 - 1];
    const double f1 = C1 >= 2 ? (lo ? col[1] : col[C1 - 2]) : 0.0;
    const double f2 = C1 >= 3 ? (lo ? col[2] : col[C1 - 3]) : 0.0;
    return ghost(f0, f1, f2, C1);
}
__device__ inline double ext2(const double *T, int64_t i, int64_t j, uint32_t C1, uint32_t C2) {
    if (j >= 0 && j < (int64_t)C2) return ext1(T + (size_t)j * C1, i, C1);
    const bool lo = j < 0;
    const double f0 = ext1(T + (size_t)(lo ? 0 : C2 - 1) * C1, i, C1);
    const double f1 = C2 >= 2 ? ext1(T + (size_t)(lo ? 1 : C2 - 2) * C1, i, C1) : 0.0;
    const double f2 = C2 >= 3 ? ext1(T + (size_t)(lo ? 2 : C2 - 3) * C1, i, C1) : 0.0;
    return ghost(f0, f1, f2, C2);
}

// cell and Keys weights of coordinate u on a line of C nodes; false: outside (or NaN)
__device__ inline bool keys(double u, uint32_t C, int64_t &i0, double (&w)[4]) {
    if (!(u >= 0.0 && u <= (double)(C - 1))) return false;
    double fl = floor(u);
    if (C >= 2 && fl > (double)(C - 2)) fl = (double)(C - 2);       // the last node belongs to the last cell (f = 1)
    const double f = u - fl, f2 = f * f, f3 = f2 * f;
    i0 = (int64_t)fl;
    w[0] = -0.5 * f3 + f2 - 0.5 * f;
    w[1] = 1.5 * f3 - 2.5 * f2 + 1.0;
    w[2] = -1.5 * f3 + 2.0 * f2 + 0.5 * f;
    w[3] = 0.5 * f3 - 0.5 * f2;
    return true;
}

__global__ void __launch_bounds__(256) tables_kernel(const double *__restrict__ T, const double *__restrict__ Pi, double *__restrict__ tau,
                                                      uint64_t I, uint32_t C1, uint32_t C2, double base) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= I) return;
    const uint32_t k = blockIdx.y;
    const double *Tk = T + (size_t)k * C1 * C2;
    int64_t i0 = 0, j0 = 0;
    double wu[4], wv[4];
    double v = NAN;
    if (keys(Pi[2 * p] - base, C1, i0, wu) && keys(Pi[2 * p + 1] - base, C2, j0, wv)) {
        v = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (wv[b] == 0.0) continue;                 // (a pixel on a grid line reads that line alone: weights 0, 1, 0, 0)
            double g = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (wu[a] != 0.0) g += wu[a] * ext2(Tk, i0 - 1 + a, j0 - 1 + b, C1, C2);
            v += wv[b] * g;
        }
    }
    tau[(size_t)k * I + p] = v;
}

}  // namespace eik
}  // namespace qdas

using qdas::fail;
using qdas::DeviceGuard;
static thread_local int g_eik_passes = 0;

extern "C" int qdas_eikonal_last_passes(void) { return g_eik_passes; }

extern "C" uint32_t qdas_eikonal_pass_cap(uint64_t C1, uint64_t C2) {
    const uint64_t cap = 8 * (C1 + C2) + 64;
    return cap > 0x7fffffffull ? 0x7fffffffu : (uint32_t)cap;
}

static int eik_check_grid(const qdas_eikonal_desc *d) {
    if (!d) return fail(QDAS_EINVAL, "eikonal: null descriptor");
    if (d->C1 >= (1ull << 31) || d->C2 >= (1ull << 31) || d->C1 * d->C2 >= (1ull << 32)) return fail(QDAS_EUNSUPPORTED, "eikonal: at most 2^32 - 1 nodes per map");
    if (d->K > 65535) return fail(QDAS_EUNSUPPORTED, "eikonal: at most 65535 source sets per call");
    if (((d->C1 + 15) / 16) * ((d->C2 + 15) / 16) >= (1ull << 24)) return fail(QDAS_EUNSUPPORTED, "eikonal: at most 2^24 - 1 tiles of 16 x 16 nodes per map (one launch covers them)");
    if (d->base != 0 && d->base != 1) return fail(QDAS_EINVAL, "eikonal: coordinates are 0- or 1-based");
    return QDAS_OK;
}

extern "C" int qdas_eikonal(const qdas_eikonal_desc *d, const double *c, const double *src, double *T, void *stream) {
    using namespace qdas::eik;
    g_eik_passes = 0;
    if (int rc = eik_check_grid(d)) return rc;
    if (d->set_begin ? false : d->npts != d->K) return fail(QDAS_EINVAL, "eikonal: without set_begin every source set is one point (npts == K)");
    if (!(d->dp > 0.0) || !std::isfinite(d->dp)) return fail(QDAS_EINVAL, "eikonal: the grid step must be positive");
    const uint64_t CC = d->C1 * d->C2;
    if (CC == 0 || d->K == 0) return QDAS_OK;            // an empty grid or no sources: nothing is launched
    if (!c || !src || !T) return fail(QDAS_EINVAL, "eikonal: null data pointer");
    const uint32_t C1 = (uint32_t)d->C1, C2 = (uint32_t)d->C2, K = (uint32_t)d->K;
    // source points: floored to a node (kern/msfm2d.m:97), every one inside the grid (kern/msfm.m:96-99)
    std::vector<uint2> pts;
    pts.reserve(d->npts);
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t b = d->set_begin ? d->set_begin[k] : k, e = d->set_begin ? d->set_begin[k + 1] : k + 1;
        if (e < b || e > d->npts) return fail(QDAS_EINVAL, "eikonal: set_begin must ascend and end at npts");
        if (e == b) return fail(QDAS_EINVAL, "eikonal: a source set is empty");
        for (uint64_t p = b; p < e; ++p) {
            const double u = src[2 * p] - d->base, v = src[2 * p + 1] - d->base;
            if (!(u >= 0.0 && v >= 0.0 && u <= (double)(C1 - 1) && v <= (double)(C2 - 1))) return fail(QDAS_EINVAL, "eikonal: a source point lies outside the grid");
            pts.push_back(make_uint2((uint32_t)floor(v) * C1 + (uint32_t)floor(u), k));
        }
    }
    const uint32_t cap = d->max_passes ? d->max_passes : qdas_eikonal_pass_cap(C1, C2);
    DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t tiles1 = (C1 + TS - 1) / TS, tiles2 = (C2 + TS - 1) / TS, ntiles = tiles1 * tiles2;
    const size_t nflag = (size_t)K * ntiles;
    // work space of this call, from the arena of the caller's stream (csrc/scratch.hip): the two flag arrays, the counters of one chunk of passes, the source points
    const size_t off_cnt = 2 * nflag * sizeof(int), off_pts = off_cnt + 8 * sizeof(int), bytes = off_pts + pts.size() * sizeof(uint2);
    static_assert(CHUNK <= 8, "the counters of a chunk");
    qdas::Scratch scratch(s);
    char *ws = (char *)scratch.get(bytes);
    if (!ws) return fail(QDAS_ENOMEM, "eikonal: no memory for the work space");
    int *flags = (int *)ws, *counters = (int *)(ws + off_cnt);
    uint2 *dpts = (uint2 *)(ws + off_pts);
    auto hip_fail = [&](hipError_t e) { (void)hipStreamSynchronize(s); return fail(QDAS_EHIP, "%s", hipGetErrorString(e)); };
    hipError_t e = hipMemsetAsync(ws, 0, off_pts, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dpts, pts.data(), pts.size() * sizeof(uint2), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e);
    const size_t ntot = (size_t)K * CC;
    fill_kernel<<<(unsigned)std::min<size_t>((ntot + 255) / 256, 65536), 256, 0, s>>>(T, ntot, INFINITY);
    seed_kernel<<<(unsigned)((pts.size() + 255) / 256), 256, 0, s>>>(dpts, (uint32_t)pts.size(), T, flags, C1, C2, tiles1, ntiles);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
    uint32_t done = 0;
    bool converged = false;
    int host_cnt[CHUNK];
    while (done < cap && !converged) {
        const uint32_t n = std::min<uint32_t>(CHUNK, cap - done);
        if (done && (e = hipMemsetAsync(counters, 0, CHUNK * sizeof(int), s)) != hipSuccess) return hip_fail(e);    // (the chunk's counters are reused)
        for (uint32_t q = 0; q < n; ++q) {
            const uint32_t p = done + q;
            pass_kernel<<<dim3(ntiles, K), TS * TS, 0, s>>>(c, T, flags + (p & 1) * nflag, flags + ((p + 1) & 1) * nflag, counters + q, C1, C2, tiles1, tiles2, d->dp);
        }
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
        e = hipMemcpyAsync(host_cnt, counters, n * sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
        for (uint32_t q = 0; q < n && !converged; ++q)
            if (host_cnt[q] == 0) { converged = true; g_eik_passes = (int)(done + q + 1); }
        done += n;
    }
    if (!converged) {                                    // never an unconverged map: the output is NaN and the call fails
        g_eik_passes = (int)done;
        fill_kernel<<<(unsigned)std::min<size_t>((ntot + 255) / 256, 65536), 256, 0, s>>>(T, ntot, NAN);
        (void)hipStreamSynchronize(s);
        return fail(QDAS_ENOCONV, "eikonal: no fixed point within %u passes (the map is set to NaN)", cap);
    }
    return QDAS_OK;
}

extern "C" int qdas_eikonal_tables(const qdas_eikonal_desc *d, const double *T, const double *Pi, double *tau, void *stream) {
    using namespace qdas::eik;
    if (int rc = eik_check_grid(d)) return rc;
    if (d->I > 0xffffff00ull) return fail(QDAS_EUNSUPPORTED, "eikonal: at most 2^32 - 256 pixels per call (one launch covers them)");
    if (d->I == 0 || d->K == 0) return QDAS_OK;
    if (d->C1 * d->C2 == 0) return fail(QDAS_EINVAL, "eikonal: tables of an empty grid");
    if (!T || !Pi || !tau) return fail(QDAS_EINVAL, "eikonal: null data pointer");
    DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    tables_kernel<<<dim3((unsigned)((d->I + 255) / 256), (unsigned)d->K), 256, 0, (hipStream_t)stream>>>(T, Pi, tau, d->I, (uint32_t)d->C1, (uint32_t)d->C2, (double)d->base);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
