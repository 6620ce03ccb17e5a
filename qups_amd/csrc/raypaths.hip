// raypaths.hip -- straight-ray line integrals over a rectilinear grid: qdas_raypaths_weights, qdas_raypaths_integrate, qdas_raypaths_backproject.  The
// reference's kern/wbilerpg.m (bilinear ray weights), kern/rayPaths.m (the tomography system matrix A; integrate is y = A s, backproject g = A' r) and
// kern/globalAverageC.m (the integral of a slowness map) without the crossing list, the sort and -- for the two products -- without the triplets.
//
// One lane per ray, in the order given: the fans callers send (one origin, neighbouring end points) put similar paths in neighbouring lanes.  The walk itself
// is raypaths_walk.h (shared with a host test).  The grid vectors, less their first value, live in LDS.  Sums run in path order in the data's precision, no
// atomics: two runs give the same bits.  `weights` writes all K = X + Z + 1 slots of its ray (4 values of a slot in one store); `integrate` gathers the map at
// the four corners of every segment as it goes -- one workgroup row per map -- and never forms a triplet.
//
// The transposed product turns the walk round (raypaths_node.h): one WAVE per 8 x 8 tile of nodes, a lane per node.  The wave scans the rays 64 at a time, a
// lane per ray: the lane derives the ray's constants and tests it against the tile's box (the tile grown by one grid line); the ballot of that test is the
// list of rays worth a look, taken in increasing order, each broadcast from its lane with v_readlane and weighed by every lane for its own node.  A gather:
// no atomics, no LDS, no barrier, no work space; ray order is the order of the sum whatever the tile shape or the launch geometry.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"
#include "raypaths_node.h"
#include "raypaths_walk.h"

namespace qdas {
namespace rayp {

constexpr int BLOCK = 256;
constexpr uint64_t LDS_LIMIT = 64 * 1024;

struct Params {
    const void *xg, *zg, *pa, *pb;
    const void *maps;                     // integrate: F maps, one after the other
    void *w, *y, *len;
    int32_t *ix, *iz;
    int64_t xstride, zstride, mapstride;  // elements
    int64_t pa_stride, pb_stride;         // 0 | 1 points
    int64_t J;
    int32_t X, Z;
};

template <typename R> struct V4;
template <> struct V4<float> { using T = float4; };
template <> struct V4<double> { using T = double4; };

template <typename R, bool WEIGHTS>
__global__ void __launch_bounds__(BLOCK) raypaths_kernel(Params P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rayp_lds[];
    R *xs = (R *)rayp_lds, *zs = xs + P.X;
    const int X = P.X, Z = P.Z;
    const R x0 = ((const R *)P.xg)[0], z0 = ((const R *)P.zg)[0];
    for (int i = threadIdx.x; i < X; i += BLOCK) xs[i] = ((const R *)P.xg)[i] - x0;
    for (int i = threadIdx.x; i < Z; i += BLOCK) zs[i] = ((const R *)P.zg)[i] - z0;
    __syncthreads();

    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= P.J) return;
    const int K = X + Z + 1;
    const R *pa = (const R *)P.pa + 2 * j * P.pa_stride, *pb = (const R *)P.pb + 2 * j * P.pb_stride;
    const R ax = pa[0] - x0, az = pa[1] - z0, bx = pb[0] - x0, bz = pb[1] - z0;
    if constexpr (WEIGHTS) {
        typename V4<R>::T *wo = (typename V4<R>::T *)P.w + j * K;
        int4 *ixo = (int4 *)P.ix + j * K, *izo = (int4 *)P.iz + j * K;
        walk<R, true>(xs, zs, X, Z, ax, az, bx, bz, [&](int s, bool emit, int cx, int cz, R w00, R w10, R w01, R w11) {
            typename V4<R>::T wv;
            wv.x = w00; wv.y = w10; wv.z = w01; wv.w = w11;
            wo[s] = wv;
            ixo[s] = emit ? make_int4(cx, cx + 1, cx, cx + 1) : make_int4(-1, -1, -1, -1);
            izo[s] = emit ? make_int4(cz, cz, cz + 1, cz + 1) : make_int4(-1, -1, -1, -1);
        });
    } else {
        const R *map = (const R *)P.maps + (int64_t)blockIdx.y * P.mapstride;
        const int64_t xst = P.xstride, zst = P.zstride;
        R acc = R(0), total = R(0);
        walk<R, false>(xs, zs, X, Z, ax, az, bx, bz, [&](int, bool emit, int cx, int cz, R w00, R w10, R w01, R w11) {
            if (!emit) return;
            const R *m = map + (int64_t)cz * zst + (int64_t)cx * xst;
            acc += w00 * m[0] + w10 * m[xst] + w01 * m[zst] + w11 * m[zst + xst];
            total += (w00 + w10) + (w01 + w11);
        });
        ((R *)P.y)[j + P.J * (int64_t)blockIdx.y] = acc;
        if (P.len && blockIdx.y == 0) ((R *)P.len)[j] = total;
    }
}

constexpr int BP_WAVES = 4;              // tiles (waves) per workgroup

struct BackParams {
    const void *xg, *zg, *pa, *pb;
    const void *r;                        // F residual vectors of J values; unused without g
    void *g, *colsum;                     // either may be null
    int64_t xstride, zstride, mapstride;  // elements
    int64_t pa_stride, pb_stride;         // 0 | 1 points
    int64_t J;
    int32_t X, Z, TX, tiles;              // TX: tiles along x; tiles: all of them
};

// what lane `l` (wave-uniform) holds: v_readlane, 64-bit values in two halves -- the value lands in scalar registers
__device__ inline float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ inline double lane_value(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

template <typename R>
__global__ void __launch_bounds__(64 * BP_WAVES) backproject_kernel(BackParams P) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * BP_WAVES + (int)(threadIdx.x >> 6);
    if (tile >= P.tiles) return;          // (the whole wave)
    const int X = P.X, Z = P.Z;
    const int tx = tile % P.TX, tz = tile / P.TX;
    const int ix = TILE * tx + (lane & (TILE - 1)), iz = TILE * tz + lane / TILE;
    const bool mine = ix < X && iz < Z;   // a lane past the grid weighs the last node of its row / column and stores nothing
    const R *xg = (const R *)P.xg, *zg = (const R *)P.zg;
    const Node<R> n = make_node(xg, X, ix < X ? ix : X - 1, zg, Z, iz < Z ? iz : Z - 1);
    R xlo, xhi, zlo, zhi;
    tile_axis(xg, X, tx, xlo, xhi);
    tile_axis(zg, Z, tz, zlo, zhi);
    const R x0 = xg[0], z0 = zg[0];
    const R *r = P.g ? (const R *)P.r + P.J * (int64_t)blockIdx.y : nullptr;
    R acc = R(0), total = R(0);
    for (int64_t j0 = 0; j0 < P.J; j0 += 64) {
        const bool have = j0 + lane < P.J;
        const int64_t j = have ? j0 + lane : P.J - 1;                    // (a lane past the last ray reads the last one and reports no hit)
        const R *pa = (const R *)P.pa + 2 * j * P.pa_stride, *pb = (const R *)P.pb + 2 * j * P.pb_stride;
        const Ray<R> q = make_ray(pa[0] - x0, pa[1] - z0, pb[0] - x0, pb[1] - z0);
        const R rj = r ? r[j] : R(0);
        unsigned long long hits = __ballot(have && ray_meets_box(q, xlo, xhi, zlo, zhi));
        while (hits) {
            const int l = __builtin_ctzll(hits);
            hits &= hits - 1;
            Ray<R> h;
            h.ax = lane_value(q.ax, l); h.az = lane_value(q.az, l); h.bx = lane_value(q.bx, l); h.bz = lane_value(q.bz, l);
            h.rdx = lane_value(q.rdx, l); h.rdz = lane_value(q.rdz, l); h.ls6 = lane_value(q.ls6, l);
            h.live = true;                                                 // (a ray that is not never hits)
            const R w = node_weight(n, h);
            if (w > R(0)) {
                acc += w * lane_value(rj, l);
                total += w;
            }
        }
    }
    if (!mine) return;
    const int64_t at = (int64_t)iz * P.zstride + (int64_t)ix * P.xstride;
    if (P.g) ((R *)P.g)[(int64_t)blockIdx.y * P.mapstride + at] = acc;
    if (P.colsum && blockIdx.y == 0) ((R *)P.colsum)[at] = total;
}

static int validate(const qdas_raypaths_desc *d, const char *who, uint64_t *lds) {
    if (!d) return fail(QDAS_EINVAL, "%s: null descriptor", who);
    if (d->dtype != QDAS_F64 && d->dtype != QDAS_F32) return fail(QDAS_EINVAL, "%s: datatype must be double or single", who);
    if (d->X < 2 || d->Z < 2) return fail(QDAS_EINVAL, "%s: the grid needs at least 2 x 2 nodes, got X = %llu, Z = %llu", who, (unsigned long long)d->X, (unsigned long long)d->Z);
    if ((d->pa_stride != 0 && d->pa_stride != 1) || (d->pb_stride != 0 && d->pb_stride != 1)) return fail(QDAS_EINVAL, "%s: pa_stride and pb_stride are 0 or 1", who);
    if (d->X >= (1ull << 31) || d->Z >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "%s: at most 2^31 - 1 nodes per axis", who);
    const uint64_t rs = d->dtype == QDAS_F64 ? 8 : 4;
    *lds = (d->X + d->Z) * rs;
    if (*lds > LDS_LIMIT)
        return fail(QDAS_EUNSUPPORTED, "%s: the grid vectors (X + Z = %llu values) need %llu bytes of LDS per workgroup (limit %llu)", who,
                    (unsigned long long)(d->X + d->Z), (unsigned long long)*lds, (unsigned long long)LDS_LIMIT);
    if (d->J > (uint64_t)BLOCK * 2147483647ull) return fail(QDAS_EUNSUPPORTED, "%s: at most 2^31 - 1 workgroups of %d rays per call", who, BLOCK);
    return QDAS_OK;
}

static void fill(Params &p, const qdas_raypaths_desc *d) {
    memset(&p, 0, sizeof p);
    p.xg = d->xg; p.zg = d->zg; p.pa = d->pa; p.pb = d->pb;
    p.xstride = d->xstride; p.zstride = d->zstride;
    p.pa_stride = d->pa_stride; p.pb_stride = d->pb_stride;
    p.J = (int64_t)d->J; p.X = (int32_t)d->X; p.Z = (int32_t)d->Z;
}

}  // namespace rayp
}  // namespace qdas

using qdas::fail;

extern "C" uint64_t qdas_raypaths_slots(uint64_t X, uint64_t Z) { return X + Z + 1; }

extern "C" int qdas_raypaths_weights(const qdas_raypaths_desc *d, void *w, int32_t *ix, int32_t *iz) {
    using namespace qdas::rayp;
    uint64_t lds = 0;
    if (int rc = validate(d, "raypaths_weights", &lds)) return rc;
    if (d->J == 0) return QDAS_OK;
    if (!d->xg || !d->zg || !d->pa || !d->pb || !w || !ix || !iz) return fail(QDAS_EINVAL, "raypaths_weights: null data pointer");
    Params p;
    fill(p, d);
    p.w = w; p.ix = ix; p.iz = iz;
    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    const dim3 grid((uint32_t)((d->J + BLOCK - 1) / BLOCK));
    if (d->dtype == QDAS_F32) raypaths_kernel<float, true><<<grid, dim3(BLOCK), (uint32_t)lds, s>>>(p);
    else                      raypaths_kernel<double, true><<<grid, dim3(BLOCK), (uint32_t)lds, s>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}

extern "C" int qdas_raypaths_integrate(const qdas_raypaths_desc *d, const void *maps, void *y, void *len) {
    using namespace qdas::rayp;
    uint64_t lds = 0;
    if (int rc = validate(d, "raypaths_integrate", &lds)) return rc;
    if (d->F > 65535) return fail(QDAS_EUNSUPPORTED, "raypaths_integrate: at most 65535 maps per call");
    // the farthest element a lane may address: (Z - 1) |zstride| + (X - 1) |xstride|, and the F maps follow each other X Z elements apart
    const long double zs = d->zstride < 0 ? -(long double)d->zstride : (long double)d->zstride, xs = d->xstride < 0 ? -(long double)d->xstride : (long double)d->xstride;
    const long double span = (long double)(d->Z - 1) * zs + (long double)(d->X - 1) * xs + (long double)d->X * (long double)d->Z * (long double)(d->F ? d->F : 1);
    if (span >= 1152921504606846976.0L || (long double)d->J * (long double)(d->F ? d->F : 1) >= 1152921504606846976.0L)
        return fail(QDAS_EUNSUPPORTED, "raypaths_integrate: map strides or J F past 2^60 elements");
    if (d->J == 0 || d->F == 0) return QDAS_OK;
    if (!d->xg || !d->zg || !d->pa || !d->pb || !maps || !y) return fail(QDAS_EINVAL, "raypaths_integrate: null data pointer");
    Params p;
    fill(p, d);
    p.maps = maps; p.y = y; p.len = len;
    p.mapstride = (int64_t)(d->X * d->Z);
    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    const dim3 grid((uint32_t)((d->J + BLOCK - 1) / BLOCK), (uint32_t)d->F);
    if (d->dtype == QDAS_F32) raypaths_kernel<float, false><<<grid, dim3(BLOCK), (uint32_t)lds, s>>>(p);
    else                      raypaths_kernel<double, false><<<grid, dim3(BLOCK), (uint32_t)lds, s>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}

extern "C" int qdas_raypaths_backproject(const qdas_raypaths_desc *d, const void *r, void *g, void *colsum) {
    using namespace qdas::rayp;
    uint64_t lds = 0;                                                      // (the forward entries' limit: the same grids are taken both ways)
    if (int rc = validate(d, "raypaths_backproject", &lds)) return rc;
    if (d->F > 65535) return fail(QDAS_EUNSUPPORTED, "raypaths_backproject: at most 65535 residual vectors per call");
    const long double zs = d->zstride < 0 ? -(long double)d->zstride : (long double)d->zstride, xs = d->xstride < 0 ? -(long double)d->xstride : (long double)d->xstride;
    const long double span = (long double)(d->Z - 1) * zs + (long double)(d->X - 1) * xs + (long double)d->X * (long double)d->Z * (long double)(d->F ? d->F : 1);
    if (span >= 1152921504606846976.0L || (long double)d->J * (long double)(d->F ? d->F : 1) >= 1152921504606846976.0L)
        return fail(QDAS_EUNSUPPORTED, "raypaths_backproject: map strides or J F past 2^60 elements");
    const uint64_t TX = (d->X + TILE - 1) / TILE, TZ = (d->Z + TILE - 1) / TILE;
    if (TX * TZ > (uint64_t)BP_WAVES * 2147483647ull)                      // (out of reach while the LDS limit above stands; kept for the day it does not)
        return fail(QDAS_EUNSUPPORTED, "raypaths_backproject: at most 2^31 - 1 workgroups of %d tiles of %d x %d nodes per call", BP_WAVES, TILE, TILE);
    if (d->F == 0 && !colsum) return QDAS_OK;                              // nothing to write
    if (!d->xg || !d->zg || (d->J && (!d->pa || !d->pb)) || (d->F && (!g || (d->J && !r)))) return fail(QDAS_EINVAL, "raypaths_backproject: null data pointer");
    BackParams p;
    memset(&p, 0, sizeof p);
    p.xg = d->xg; p.zg = d->zg; p.pa = d->pa; p.pb = d->pb;
    p.r = r; p.g = d->F ? g : nullptr; p.colsum = colsum;
    p.xstride = d->xstride; p.zstride = d->zstride; p.mapstride = (int64_t)(d->X * d->Z);
    p.pa_stride = d->pa_stride; p.pb_stride = d->pb_stride;
    p.J = (int64_t)d->J; p.X = (int32_t)d->X; p.Z = (int32_t)d->Z; p.TX = (int32_t)TX; p.tiles = (int32_t)(TX * TZ);
    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    const dim3 grid((uint32_t)((TX * TZ + BP_WAVES - 1) / BP_WAVES), (uint32_t)(d->F ? d->F : 1));
    if (d->dtype == QDAS_F32) backproject_kernel<float><<<grid, dim3(64 * BP_WAVES), 0, s>>>(p);
    else                      backproject_kernel<double><<<grid, dim3(64 * BP_WAVES), 0, s>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
