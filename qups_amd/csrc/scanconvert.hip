// scanconvert.hip -- qdas_scanconvert: an image on a polar grid (pages of R x A images) or a volume on a spherical grid (R x A x E) onto a Cartesian grid, the
// reference's ScanPolar.scanConvert (src/ScanPolar.m:143-201: cart2pol + interp2, NaN outside) and ScanSpherical.scanConvert (src/ScanSpherical.m:121-188:
// cart2sph + interp3), with the envelope / log compression its examples apply just before (mod2db) fused into the same pass.
//
// A gather kernel.  Lanes run along the output's z, its fastest dimension, so neighbouring lanes walk along r in the source -- the fastest dimension of the view
// DAS returns.  A lane computes the coordinates of its pixel, its cells and its weights once (scanconvert_core.h, shared with a host test), then loops over
// the pages.  The source axes live in LDS as float64; the output axes are read from global memory (x and y are the same for a whole workgroup).  Every output
// element is written exactly once by the lane that owns it -- inside or not -- and there are no atomics: two runs give the same bits.
//
// CELL SEARCH.  The axes are DEVICE vectors the entry may not read (it synchronises nothing), so the workgroup itself finds out, while it copies an axis into
// LDS, whether every node lies within a quarter of the constant pitch (g[n-1] - g[0]) / (n - 1) of its place.  If so a lane guesses its cell from the inverse
// pitch and corrects the guess against the nodes in LDS; otherwise, and when the guess is more than two cells off, it bisects.  Either way the cell is the one
// the contract names on the actual vector, and the inside test uses the actual end nodes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"
#include "scanconvert_core.h"

namespace qdas {
namespace sc {

constexpr int BLOCK = 256;
constexpr uint64_t MAX_NODES = 8192;      // R + A + E float64 values: 64 KiB of LDS

struct Params {
    const double *r, *a, *e, *x, *y, *z;
    const void *b;
    void *out;
    int64_t sr, sa, se, sp;               // source strides, elements
    int64_t Z, X, Y, P;                   // Y >= 1
    int32_t R, A, E;
    uint32_t nzb;                         // workgroups along z
    int32_t bisect;                       // 1: never take the O(1) path (QDAS_SCANCONVERT_BISECT=1: tests)
    double ox, oy, oz, fill, db_floor;
};

// copies axis g (n nodes) into LDS and returns 1 / pitch when the whole workgroup found it uniform, else 0.  Ends with a barrier: s[] is complete on return.
__device__ inline double stage_axis(const double *g, int n, double *s, bool force_bisect) {
    const double g0 = g[0], pitch = pitch_of(g0, g[n - 1], n);
    int off = 0;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const double v = g[i];
        s[i] = v;
        off |= !on_pitch(v, g0, i, pitch);
    }
    const bool uniform = __syncthreads_or(off) == 0;
    return inv_pitch(pitch, uniform && !force_bisect);
}

template <typename R, bool CPLX, int PRE, bool SPH>
__global__ void __launch_bounds__(BLOCK) scanconvert_kernel(Params p) {
    using V = typename Value<R, CPLX, PRE>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
    double *rs = (double *)sc_lds, *as = rs + p.R, *es = as + p.A;
    const double inv_r = stage_axis(p.r, p.R, rs, p.bisect != 0);
    const double inv_a = stage_axis(p.a, p.A, as, p.bisect != 0);
    double inv_e = 0.0;
    if constexpr (SPH) inv_e = stage_axis(p.e, p.E, es, p.bisect != 0);

    const uint32_t zb = blockIdx.x % p.nzb;
    const int64_t rest = blockIdx.x / p.nzb;
    const int64_t j = rest % p.X, yy = rest / p.X;
    const int64_t i = (int64_t)zb * BLOCK + threadIdx.x;
    if (i >= p.Z) return;

    const double dz = p.z[i] - p.oz, dx = p.x[j] - p.ox;
    int k = 0, l = 0, m = 0;
    double wu = 0.0, wv = 0.0, ww = 0.0;
    bool in;
    if constexpr (SPH) {
        double rho, alpha, eps;
        spherical_of(dz, dx, p.y[yy] - p.oy, rho, alpha, eps);
        in = locate(rs, p.R, rho, inv_r, k, wu);
        in = locate(as, p.A, alpha, inv_a, l, wv) && in;
        in = locate(es, p.E, eps, inv_e, m, ww) && in;
    } else {
        double rho, alpha;
        polar_of(dz, dx, rho, alpha);
        in = locate(rs, p.R, rho, inv_r, k, wu);
        in = locate(as, p.A, alpha, inv_a, l, wv) && in;
    }
    const R u = (R)wu, v = (R)wv, w = (R)ww, fl = (R)p.db_floor;
    const int64_t o = (int64_t)k * p.sr + (int64_t)l * p.sa + (int64_t)m * p.se;
    const int64_t ostride = p.Z * p.X * p.Y;
    V *out = (V *)p.out + i + p.Z * (j + p.X * yy);
    const V outside = filled<R, CPLX, PRE>((R)p.fill);
    for (int64_t pg = 0; pg < p.P; ++pg) {
        V val = outside;
        if (in) {
            if constexpr (SPH) val = trilerp<R, CPLX, PRE>(p.b, o + pg * p.sp, p.sr, p.sa, p.se, u, v, w, fl);
            else               val = bilerp<R, CPLX, PRE>(p.b, o + pg * p.sp, p.sr, p.sa, u, v, fl);
        }
        out[pg * ostride] = val;
    }
}

template <typename R, bool CPLX, int PRE>
static void launch2(const Params &p, bool sph, dim3 grid, uint32_t lds, hipStream_t s) {
    if (sph) scanconvert_kernel<R, CPLX, PRE, true><<<grid, dim3(BLOCK), lds, s>>>(p);
    else     scanconvert_kernel<R, CPLX, PRE, false><<<grid, dim3(BLOCK), lds, s>>>(p);
}
template <typename R, bool CPLX>
static void launch1(const Params &p, int pre, bool sph, dim3 grid, uint32_t lds, hipStream_t s) {
    if (pre == QDAS_SC_PRE_NONE)     launch2<R, CPLX, PRE_NONE>(p, sph, grid, lds, s);
    else if (pre == QDAS_SC_PRE_ABS) launch2<R, CPLX, PRE_ABS>(p, sph, grid, lds, s);
    else                             launch2<R, CPLX, PRE_DB>(p, sph, grid, lds, s);
}

static long double span_of(uint64_t n, int64_t stride) { return n ? (long double)(n - 1) * (stride < 0 ? -(long double)stride : (long double)stride) : 0.0L; }

}  // namespace sc
}  // namespace qdas

using qdas::fail;

extern "C" int qdas_scanconvert(const qdas_scanconvert_desc *d, const void *b, void *out) {
    using namespace qdas::sc;
    static_assert(QDAS_SC_PRE_NONE == PRE_NONE && QDAS_SC_PRE_ABS == PRE_ABS && QDAS_SC_PRE_DB == PRE_DB, "pre codes");
    if (!d) return fail(QDAS_EINVAL, "scanconvert: null descriptor");
    if (d->dtype != QDAS_F64 && d->dtype != QDAS_F32) return fail(QDAS_EINVAL, "scanconvert: dtype must be QDAS_F32 or QDAS_F64 (half-precision images are not built), got %d", d->dtype);
    if (d->cplx != 0 && d->cplx != 1) return fail(QDAS_EINVAL, "scanconvert: cplx is 0 or 1, got %d", d->cplx);
    if (d->pre != QDAS_SC_PRE_NONE && d->pre != QDAS_SC_PRE_ABS && d->pre != QDAS_SC_PRE_DB) return fail(QDAS_EINVAL, "scanconvert: unknown pre %d", d->pre);
    if (d->R < 2 || d->A < 2) return fail(QDAS_EINVAL, "scanconvert: the source needs at least 2 x 2 nodes, got R = %llu, A = %llu", (unsigned long long)d->R, (unsigned long long)d->A);
    if (d->E == 1) return fail(QDAS_EINVAL, "scanconvert: E is 0 (polar) or at least 2 (spherical), got 1");
    if (d->E == 0 && d->Y != 0) return fail(QDAS_EINVAL, "scanconvert: a polar source (E = 0) has no y axis: Y must be 0, got %llu", (unsigned long long)d->Y);
    if (d->E >= 2 && d->Y == 0) return fail(QDAS_EINVAL, "scanconvert: a spherical source (E >= 2) needs Y >= 1, got 0");
    for (int k = 0; k < 3; ++k)
        if (!isfinite(d->origin[k])) return fail(QDAS_EINVAL, "scanconvert: origin[%d] is not finite", k);
    if (d->db_floor != d->db_floor) return fail(QDAS_EINVAL, "scanconvert: db_floor is NaN");
    const bool sph = d->E >= 2;
    if (d->R + d->A + d->E > MAX_NODES || d->R > MAX_NODES || d->A > MAX_NODES || d->E > MAX_NODES)
        return fail(QDAS_EUNSUPPORTED, "scanconvert: the source axes (R + A + E = %llu float64 values) need more than 64 KiB of LDS per workgroup (limit %llu values)",
                    (unsigned long long)(d->R + d->A + d->E), (unsigned long long)MAX_NODES);
    const uint64_t Ye = sph ? d->Y : 1;
    const long double LIM = 1152921504606846976.0L;          // 2^60
    const long double nout = (long double)d->Z * (long double)d->X * (long double)Ye * (long double)d->P;
    const long double nsrc = span_of(d->R, d->sr) + span_of(d->A, d->sa) + span_of(d->E, d->se) + span_of(d->P, d->sp);
    if (nout >= LIM || nsrc >= LIM) return fail(QDAS_EUNSUPPORTED, "scanconvert: Z X Y P or the source strides reach past 2^60 elements");
    if (nout == 0.0L) return QDAS_OK;
    const uint64_t nzb = (d->Z + BLOCK - 1) / BLOCK;
    if ((long double)nzb * (long double)d->X * (long double)Ye > 2147483647.0L)
        return fail(QDAS_EUNSUPPORTED, "scanconvert: more than 2^31 - 1 workgroups (%d values of z each) for Z = %llu, X = %llu, Y = %llu", BLOCK,
                    (unsigned long long)d->Z, (unsigned long long)d->X, (unsigned long long)d->Y);
    if (!d->r || !d->a || !d->x || !d->z || (sph && (!d->e || !d->y))) return fail(QDAS_EINVAL, "scanconvert: null axis pointer (r, a, x, z%s)", sph ? ", e, y" : "");
    if (!b || !out) return fail(QDAS_EINVAL, "scanconvert: null data pointer (%s)", !b ? "b" : "out");

    Params p;
    memset(&p, 0, sizeof p);
    p.r = d->r; p.a = d->a; p.e = d->e; p.x = d->x; p.y = d->y; p.z = d->z;
    p.b = b; p.out = out;
    p.sr = d->sr; p.sa = d->sa; p.se = sph ? d->se : 0; p.sp = d->sp;
    p.Z = (int64_t)d->Z; p.X = (int64_t)d->X; p.Y = (int64_t)Ye; p.P = (int64_t)d->P;
    p.R = (int32_t)d->R; p.A = (int32_t)d->A; p.E = (int32_t)d->E;
    p.nzb = (uint32_t)nzb;
    const char *env = getenv("QDAS_SCANCONVERT_BISECT");
    p.bisect = env && env[0] == '1';
    p.ox = d->origin[0]; p.oy = d->origin[1]; p.oz = d->origin[2];
    p.fill = d->fill; p.db_floor = d->db_floor;

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    const dim3 grid((uint32_t)(nzb * d->X * Ye));
    const uint32_t lds = (uint32_t)((d->R + d->A + d->E) * sizeof(double));
    if (d->dtype == QDAS_F32) { if (d->cplx) launch1<float, true>(p, d->pre, sph, grid, lds, s); else launch1<float, false>(p, d->pre, sph, grid, lds, s); }
    else                      { if (d->cplx) launch1<double, true>(p, d->pre, sph, grid, lds, s); else launch1<double, false>(p, d->pre, sph, grid, lds, s); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
