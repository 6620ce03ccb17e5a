// pwznxcorr.hip -- pair-wise windowed zero-normalized cross-correlation: qdas_pwznxcorr.  The base-MATLAB branch of the reference's
// kern/pwznxcorr.m (iflt = false: convn(., w, 'same'), a zero pad of max|lags| samples at the end of the record, circshift), every lag in
// ONE launch.
//
// With K(a)[s] = sum_k w[k] a[s + h - k], h = floor(W/2), a = 0 outside [0, Tp), Tp = T + P:
//   xlz = xl - K(xl)                      (zero; else xl)         xln = K(|xlz|^2)
//   c_l[s] = conj(xr[(s + l) mod Tp])     cz = c_l - K(c_l)       y_l = K(xlz cz) / (sqrt(xln) sqrt(K(|cz|^2)))     (norm; else y_l = K(xlz cz))
//
// A workgroup owns one (channel pair, batch index) and TILE output times.  It stages, once, the raw left record of the tile plus a halo of
// 2 (W - 1) samples and the periodically extended right record of the same span widened by the lag span; forms xlz for tile + (W - 1) in LDS
// and xln in a register; then per lag forms the products xlz cz and |cz|^2 for tile + (W - 1) in LDS and sums them over the window.  Every
// sum is a direct weighted sum over the window in the data's precision, in a fixed order: no prefix sums, no atomics, bit-reproducible.
// The weights are read through the scalar cache (the tap index is uniform), so a tap costs the LDS reads of its operands only.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"

namespace qdas {
namespace pwz {

constexpr int BLOCK = 256;
constexpr int TILE = QDAS_PWZNXCORR_TIME_TILE;      // output times per workgroup: one per lane
constexpr int MAX_LAGS = QDAS_PWZNXCORR_MAX_LAGS;   // the lag table travels in the kernel arguments
constexpr uint64_t LDS_LIMIT = 64 * 1024;
static_assert(TILE == BLOCK, "one output time per lane");

struct Params {
    const void *xl, *xr, *w;
    void *y;
    int32_t T, Tp, W, h;                  // record, padded record, window, floor(W / 2)
    int32_t lmin, span;                   // smallest lag; largest - smallest
    uint32_t nlags, ntiles, N, B0;        // (B1 = the rest of the grid)
    int64_t lsN, lsB0, lsB1;              // element strides of the left operand, ...
    int64_t rsN, rsB0, rsB1;              // ... the right operand (0 broadcasts) ...
    int64_t ysN, ysB0, ysB1, ysL;         // ... and the output
    int16_t lags[MAX_LAGS];
};

#define QDAS_CONST_AS __attribute__((address_space(4)))

template <typename R, bool CPLX> struct V;
template <typename R> struct V<R, false> { R re; };
template <typename R> struct alignas(2 * sizeof(R)) V<R, true> { R re, im; };
template <typename R> struct V2;
template <> struct V2<float> { using T = float2; };
template <> struct V2<double> { using T = double2; };

template <typename R, bool CPLX> __device__ inline V<R, CPLX> vzero() {
    V<R, CPLX> v;
    v.re = R(0);
    if constexpr (CPLX) v.im = R(0);
    return v;
}
template <typename R, bool CPLX> __device__ inline V<R, CPLX> ldg(const R *x, int64_t t) {     // x: the record's first real
    V<R, CPLX> v;
    if constexpr (CPLX) { const typename V2<R>::T u = *(const typename V2<R>::T *)(x + 2 * t); v.re = u.x; v.im = u.y; }
    else v.re = x[t];
    return v;
}
template <typename R, bool CPLX> __device__ inline void wfma(V<R, CPLX> &a, R w, V<R, CPLX> v) {   // a += w v
    a.re += w * v.re;
    if constexpr (CPLX) a.im += w * v.im;
}
template <typename R, bool CPLX> __device__ inline V<R, CPLX> vsub(V<R, CPLX> a, V<R, CPLX> b) {
    a.re -= b.re;
    if constexpr (CPLX) a.im -= b.im;
    return a;
}
template <typename R, bool CPLX> __device__ inline V<R, CPLX> mulconj(V<R, CPLX> a, V<R, CPLX> b) {   // a conj(b)
    V<R, CPLX> v;
    if constexpr (CPLX) { v.re = a.re * b.re + a.im * b.im; v.im = a.im * b.re - a.re * b.im; }
    else v.re = a.re * b.re;
    return v;
}
template <typename R, bool CPLX> __device__ inline R mag2(V<R, CPLX> a) {
    if constexpr (CPLX) return a.re * a.re + a.im * a.im;
    else return a.re * a.re;
}

// lag i of the table, read from the kernel-argument segment (Params is the kernel's only argument): indexing the by-value argument with a
// run-time index would copy the whole struct to private memory
__device__ inline int lag_at(uint32_t i) {
    const int16_t *t = (const int16_t *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(Params, lags));
    return t[i];
}

// LDS of one workgroup [bytes]: xlz, products (tile + W - 1 elements), |cz|^2 (reals), the raw left and the extended right record
__host__ __device__ inline uint64_t lds_bytes(uint64_t esize, uint64_t rsize, uint64_t W, uint64_t span) {
    const uint64_t nA = TILE + W - 1, nRaw = TILE + 2 * (W - 1), nR = nRaw + span;
    return (2 * nA + nRaw + nR) * esize + nA * rsize;
}

template <typename R, bool CPLX, bool ZERO, bool NORM>
__global__ void __launch_bounds__(BLOCK) pwz_kernel(Params P) {
    using E = V<R, CPLX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char pwz_lds[];
    const int W = P.W, h = P.h, T = P.T, Tp = P.Tp;
    const int nA = TILE + W - 1, nRaw = TILE + 2 * (W - 1), nR = nRaw + P.span;
    E *xlz = (E *)pwz_lds;                  // xlz[j],      j = jb + a, a in [0, nA)
    E *prod = xlz + nA;                     // (xlz cz)[j]
    E *lraw = prod + nA;                    // xl[i],       i = ib + a, a in [0, nRaw), 0 outside [0, T)
    E *rr = lraw + nRaw;                    // xr[q mod Tp], q = ib + lmin + a, a in [0, nR), 0 in the pad
    R *qq = (R *)(rr + nR);                 // |cz|^2[j]
    const QDAS_CONST_AS R *w = (const QDAS_CONST_AS R *)P.w;

    uint32_t r = blockIdx.x;
    const uint32_t tile = r % P.ntiles; r /= P.ntiles;
    const uint32_t n = r % P.N; r /= P.N;
    const uint32_t b0 = r % P.B0, b1 = r / P.B0;
    constexpr int64_t ES = CPLX ? 2 : 1;
    const R *xl = (const R *)P.xl + ES * ((int64_t)n * P.lsN + (int64_t)b0 * P.lsB0 + (int64_t)b1 * P.lsB1);
    const R *xr = (const R *)P.xr + ES * ((int64_t)n * P.rsN + (int64_t)b0 * P.rsB0 + (int64_t)b1 * P.rsB1);
    R *y = (R *)P.y + ES * ((int64_t)n * P.ysN + (int64_t)b0 * P.ysB0 + (int64_t)b1 * P.ysB1);

    const int tid = threadIdx.x;
    const int s0 = (int)tile * TILE;
    const int jb = s0 + h - (W - 1);        // first time of the windowed arrays
    const int ib = jb + h - (W - 1);        // first time of the raw arrays
    const int qb = ib + P.lmin;
    const int ctr = W - 1 - h;              // raw index of time j = jb + a is a + ctr

    // ---- stage the raw records
    if constexpr (ZERO) {
        for (int a = tid; a < nRaw; a += BLOCK) {
            const int i = ib + a;
            lraw[a] = (i >= 0 && i < T) ? ldg<R, CPLX>(xl, i) : vzero<R, CPLX>();
        }
    }
    for (int a = tid; a < nR; a += BLOCK) {
        int m = (qb + a) % Tp;
        if (m < 0) m += Tp;
        rr[a] = m < T ? ldg<R, CPLX>(xr, m) : vzero<R, CPLX>();
    }
    __syncthreads();

    // ---- the left side, once: xlz = xl - K(xl) on [0, Tp), 0 outside
    for (int a = tid; a < nA; a += BLOCK) {
        const int j = jb + a;
        E v = vzero<R, CPLX>();
        if constexpr (ZERO) {
            if (j >= 0 && j < Tp) {
                E acc = vzero<R, CPLX>();
                const E *p = lraw + a + W - 1;
#pragma unroll 8
                for (int k = 0; k < W; ++k) wfma(acc, w[k], p[-k]);
                v = vsub(lraw[a + ctr], acc);
            }
        } else {
            if (j >= 0 && j < T) v = ldg<R, CPLX>(xl, j);
        }
        xlz[a] = v;
    }
    __syncthreads();
    R xln = R(0);
    if constexpr (NORM) {
        const E *p = xlz + tid + W - 1;
#pragma unroll 8
        for (int k = 0; k < W; ++k) xln += w[k] * mag2(p[-k]);
        xln = sqrt(xln);
    }

    // the raw samples of the tile's taps all lie inside [0, Tp): no tap of K(c) has to be masked
    const bool interior = ib >= 0 && ib + nRaw <= Tp;
    const int s = s0 + tid;
    for (uint32_t li = 0; li < P.nlags; ++li) {
        const int dl = lag_at(li) - P.lmin;   // c_l[i] = conj(rr[i - ib + dl]) for i in [0, Tp), 0 outside
        // ---- z = xr_l - K(xr_l) (cz = conj(z)); the products xlz cz and |cz|^2
        for (int a = tid; a < nA; a += BLOCK) {
            const int j = jb + a;
            E pv = vzero<R, CPLX>();
            R qv = R(0);
            if (j >= 0 && j < Tp) {
                E z = rr[a + ctr + dl];
                if constexpr (ZERO) {
                    E acc = vzero<R, CPLX>();
                    const E *p = rr + a + W - 1 + dl;
                    if (interior) {
#pragma unroll 8
                        for (int k = 0; k < W; ++k) wfma(acc, w[k], p[-k]);
                    } else {
                        const int top = ib + a + W - 1;      // time of tap k = 0; tap k is inside [0, Tp) for klo <= k <= khi
                        const int klo = top - Tp + 1, khi = top;
#pragma unroll 8
                        for (int k = 0; k < W; ++k) wfma(acc, w[k], (k >= klo && k <= khi) ? p[-k] : vzero<R, CPLX>());
                    }
                    z = vsub(z, acc);
                }
                pv = mulconj(xlz[a], z);
                if constexpr (NORM) qv = mag2(z);
            }
            prod[a] = pv;
            if constexpr (NORM) qq[a] = qv;
        }
        __syncthreads();
        // ---- y = K(xlz cz), normalised
        {
            E acc = vzero<R, CPLX>();
            R den = R(0);
            const E *p = prod + tid + W - 1;
            const R *pq = qq + tid + W - 1;
#pragma unroll 8
            for (int k = 0; k < W; ++k) {
                const R wk = w[k];
                wfma(acc, wk, p[-k]);
                if constexpr (NORM) den += wk * pq[-k];
            }
            if (s < T) {
                if constexpr (NORM) {
                    const R d = xln * sqrt(den);          // 0 / 0 stays NaN
                    acc.re /= d;
                    if constexpr (CPLX) acc.im /= d;
                }
                R *yo = y + ES * ((int64_t)li * P.ysL + s);
                if constexpr (CPLX) { typename V2<R>::T o; o.x = acc.re; o.y = acc.im; *(typename V2<R>::T *)yo = o; }
                else *yo = acc.re;
            }
        }
        __syncthreads();
    }
}

template <typename R, bool CPLX>
static hipError_t launch(const Params &P, int zero, int norm, uint32_t blocks, uint32_t lds, hipStream_t s) {
#define QDAS_PWZ(Z, NM) pwz_kernel<R, CPLX, Z, NM><<<dim3(blocks), dim3(BLOCK), lds, s>>>(P)
    if (zero) { if (norm) QDAS_PWZ(true, true); else QDAS_PWZ(true, false); }
    else      { if (norm) QDAS_PWZ(false, true); else QDAS_PWZ(false, false); }
#undef QDAS_PWZ
    return hipGetLastError();
}

}  // namespace pwz
}  // namespace qdas

using qdas::fail;

extern "C" int qdas_pwznxcorr_time_tile(void) { return qdas::pwz::TILE; }

extern "C" uint64_t qdas_pwznxcorr_lds_bytes(int dtype, int cplx, uint64_t W, uint64_t span) {
    const uint64_t rs = dtype == QDAS_F64 ? 8 : 4;
    return qdas::pwz::lds_bytes(rs * (cplx ? 2 : 1), rs, W ? W : 1, span);
}

extern "C" int qdas_pwznxcorr(const qdas_pwznxcorr_desc *d, const void *xl, const void *xr, const void *w, const int64_t *lags, void *y, void *stream) {
    using namespace qdas::pwz;
    if (!d) return fail(QDAS_EINVAL, "pwznxcorr: null descriptor");
    if (d->dtype != QDAS_F64 && d->dtype != QDAS_F32) return fail(QDAS_EINVAL, "pwznxcorr: datatype must be double or single");
    if (d->W == 0) return fail(QDAS_EINVAL, "pwznxcorr: the window is empty (W = 0)");
    if (d->nlags && !lags) return fail(QDAS_EINVAL, "pwznxcorr: null lag table");
    if (d->T >= (1ull << 30) || d->W >= (1ull << 20)) return fail(QDAS_EUNSUPPORTED, "pwznxcorr: at most 2^30 - 1 samples per record and a window below 2^20");
    if (d->nlags > (uint64_t)MAX_LAGS) return fail(QDAS_EUNSUPPORTED, "pwznxcorr: at most %d lags per call", MAX_LAGS);
    int64_t lmin = 0, lmax = 0, labs = 0;
    for (uint64_t i = 0; i < d->nlags; ++i) {
        const int64_t l = lags[i];
        if (l > 32767 || l < -32767) return fail(QDAS_EUNSUPPORTED, "pwznxcorr: lags reach at most +-32767");
        if (i == 0 || l < lmin) lmin = l;
        if (i == 0 || l > lmax) lmax = l;
        if (l > labs) labs = l;
        if (-l > labs) labs = -l;
    }
    const uint64_t rs = d->dtype == QDAS_F64 ? 8 : 4, es = rs * (d->cplx ? 2 : 1);
    const uint64_t lds = lds_bytes(es, rs, d->W, (uint64_t)(lmax - lmin));
    if (lds > LDS_LIMIT)
        return fail(QDAS_EUNSUPPORTED, "pwznxcorr: a window of %llu samples and a lag span of %lld need %llu bytes of LDS per workgroup (limit %llu)",
                    (unsigned long long)d->W, (long long)(lmax - lmin), (unsigned long long)lds, (unsigned long long)LDS_LIMIT);
    const uint64_t Tp = d->T + (d->pad ? (uint64_t)labs : 0);
    const uint64_t ntiles = (d->T + TILE - 1) / TILE;
    const uint64_t B0 = d->bsize[0], B1 = d->bsize[1];
    if (d->N >= (1ull << 31) || B0 >= (1ull << 31) || B1 >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "pwznxcorr: at most 2^31 - 1 channel pairs and batch entries per group");
    const long double blocks = (long double)ntiles * (long double)d->N * (long double)B0 * (long double)B1;
    if (blocks >= 2147483648.0L) return fail(QDAS_EUNSUPPORTED, "pwznxcorr: at most 2^31 - 1 workgroups (time tiles x channel pairs x batch) per call");
    if (blocks == 0 || d->nlags == 0) return QDAS_OK;           // an empty result: nothing is launched
    if (!xl || !xr || !w || !y) return fail(QDAS_EINVAL, "pwznxcorr: null data pointer");

    Params p;
    memset(&p, 0, sizeof p);
    p.xl = xl; p.xr = xr; p.w = w; p.y = y;
    p.T = (int32_t)d->T; p.Tp = (int32_t)Tp; p.W = (int32_t)d->W; p.h = (int32_t)(d->W / 2);
    p.lmin = (int32_t)lmin; p.span = (int32_t)(lmax - lmin);
    p.nlags = (uint32_t)d->nlags; p.ntiles = (uint32_t)ntiles; p.N = (uint32_t)d->N; p.B0 = (uint32_t)B0;
    p.lsN = d->xl_strideN; p.lsB0 = d->xl_bstride[0]; p.lsB1 = d->xl_bstride[1];
    p.rsN = d->xr_strideN; p.rsB0 = d->xr_bstride[0]; p.rsB1 = d->xr_bstride[1];
    p.ysN = d->y_strideN; p.ysB0 = d->y_bstride[0]; p.ysB1 = d->y_bstride[1]; p.ysL = d->y_strideL;
    for (uint64_t i = 0; i < d->nlags; ++i) p.lags[i] = (int16_t)lags[i];

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t nb = (uint32_t)blocks;
    hipError_t e;
    if (d->dtype == QDAS_F32) e = d->cplx ? launch<float, true>(p, d->zero, d->norm, nb, (uint32_t)lds, s) : launch<float, false>(p, d->zero, d->norm, nb, (uint32_t)lds, s);
    else                      e = d->cplx ? launch<double, true>(p, d->zero, d->norm, nb, (uint32_t)lds, s) : launch<double, false>(p, d->zero, d->norm, nb, (uint32_t)lds, s);
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
