// coherence.hip -- aperture-reduction images of a receive-kept image: qdas_coherence.  The MATLAB branches of the reference's kern/slsc.m
// (average and ensemble estimators, optional time kernel), kern/dmas.m, kern/cohfac.m and kern/pcf.m, restated per pixel.
//
// One lane owns one output pixel and walks the aperture (and the time kernel) of that pixel in a fixed order: loads are coalesced across the
// lanes of a wave (pixels are the fastest dimension of the canonical layout, include/qdas.h), there are no atomics and the summation order does
// not depend on the launch, so results are bit-reproducible.
//
// The lag estimators (SLSC, DMAS over a lag subset) keep a window of C consecutive receivers in registers and one accumulator per lag of a chunk
// of C lags: receiver n meets its partners n + l0 .. n + l0 + C - 1 with one new load per step (two when the chunk does not start at lag 0), so
// one load feeds C products.  The loop over n is unrolled by C, which turns the ring buffer's slot indices into constants.  The per-lag
// weights of the reference (1 / (2 L (N - l)) for the average estimator) are applied once per chunk.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"

namespace qdas {
namespace coh {

constexpr int MASK_WORDS = 64;      // a lag set that is not a range travels as a bitmask in the kernel arguments: lags < 2048
constexpr uint32_t MASK_LAGS = 32u * MASK_WORDS;
constexpr int BLOCK = 256;

enum { AVG = QDAS_COH_SLSC_AVERAGE, ENS = QDAS_COH_SLSC_ENSEMBLE, DMAS = QDAS_COH_DMAS, COHFAC = QDAS_COH_COHFAC, PCF = QDAS_COH_PCF };

struct Params {
    const void *x;
    void *y, *y2;
    uint32_t P, s0, s1;             // pixels; sizes of pixel groups 0 and 1 (group 2 = P / (s0 s1))
    uint32_t N, K;                  // aperture, time kernel
    uint32_t lo, hi;                // lag range [lo, hi], lo >= 1 (use_mask == 0)
    uint32_t use_mask, zero_lag;    // the set is mask[]; lag 0 is in the set
    uint32_t maxlag;                // largest lag of the set that has pairs (<= N - 1); 0: none
    uint32_t ntot;                  // lags l of the set with 1 <= l <= maxlag
    int64_t st0, st1, st2, sN, sK;  // element strides
    double lnorm;                   // SLSC: L = numel(lags) as given
    double g;                       // PCF: gamma / sqrt(pi / 3)
    uint32_t mask[MASK_WORDS];
};

template <typename R> struct V2;
template <> struct V2<float> { using T = float2; };
template <> struct V2<double> { using T = double2; };

template <typename R> struct Cx { R re, im; };

// word i of the lag mask, read from the kernel-argument segment (every kernel here takes Params as its only argument): indexing the by-value
// argument with a run-time index would copy the whole struct to private memory
__device__ inline uint32_t mask_word(uint32_t i) {
    const uint32_t *m = (const uint32_t *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(Params, mask));
    return m[i];
}

__device__ inline bool inset(const Params &P, uint32_t l) {       // l >= 1
    if (l > P.maxlag) return false;
    return P.use_mask ? ((mask_word(l >> 5) >> (l & 31)) & 1u) != 0 : (l >= P.lo && l <= P.hi);
}

template <typename R, bool CPLX> __device__ inline Cx<R> ld(const R *x, int64_t off) {
    Cx<R> v;
    if constexpr (CPLX) { const typename V2<R>::T t = *(const typename V2<R>::T *)(x + 2 * off); v.re = t.x; v.im = t.y; }
    else { v.re = x[off]; v.im = R(0); }
    return v;
}
template <typename R> __device__ inline bool isnan_(Cx<R> v) { return v.re != v.re || v.im != v.im; }
template <typename R> __device__ inline R mag2(Cx<R> v) { return v.re * v.re + v.im * v.im; }
template <typename R> __device__ inline R rsq(R s) { return R(1) / sqrt(s); }
template <> __device__ inline float rsq<float>(float s) { return __builtin_amdgcn_rsqf(s); }   // v_rsq_f32 (1 ulp; 0 -> Inf, NaN -> NaN)

// x(n, k) as the estimator consumes it, from the address of x(n, 0) (in units of R) and the time-kernel offset.  AVG: x / ||x(n, :)||_2 over
// the time kernel with 0/0 (and any NaN) -> 0 (kern/slsc.m:190); ENS: the sums omit NaN products, i.e. a NaN sample counts as 0
// (kern/slsc.m:217-219); DMAS: as it is (NaN propagates, kern/dmas.m:77).
template <int MODE, typename R, bool CPLX, bool KD = false>
__device__ inline Cx<R> sample(const Params &P, const R *xn, int64_t koff) {
    Cx<R> v = ld<R, CPLX>(xn, koff);
    if constexpr (MODE == AVG) {
        R s;
        if constexpr (!KD) s = mag2(v);
        else { s = R(0); for (uint32_t q = 0; q < P.K; ++q) s += mag2(ld<R, CPLX>(xn, (int64_t)q * P.sK)); }
        const R r = rsq(s);
        v.re *= r; v.im *= r;
        if (isnan_(v)) { v.re = R(0); v.im = R(0); }
    } else if constexpr (MODE == ENS) {
        if (isnan_(v)) { v.re = R(0); v.im = R(0); }
    }
    return v;
}

// the lags l0 .. l0 + C - 1 that are in the set, as bits (C divides 32 and l0 is a multiple of C: one word of the table)
template <int C> __device__ inline uint32_t chunk_bits(const Params &P, uint32_t l0) {
    uint32_t b;
    if (P.use_mask) b = (mask_word(l0 >> 5) >> (l0 & 31)) & (C == 32 ? 0xffffffffu : ((1u << C) - 1u));
    else {
        b = 0;
        for (int c = 0; c < C; ++c) b |= (uint32_t)(l0 + c >= P.lo && l0 + c <= P.hi) << c;
    }
    const uint32_t top = P.maxlag >= l0 ? P.maxlag - l0 : 0;   // lags above maxlag have no pairs
    if (P.maxlag < l0) b = 0;
    else if (top + 1 < (uint32_t)C) b &= (1u << (top + 1)) - 1u;
    if (l0 == 0) b = (b & ~1u) | (P.zero_lag ? 1u : 0u);
    return b;
}

__device__ inline bool pixel(const Params &P, int64_t &base, uint32_t &p) {
    p = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if (p >= P.P) return false;
    const uint32_t i0 = p % P.s0, r = p / P.s0, i1 = r % P.s1, i2 = r / P.s1;
    base = (int64_t)i0 * P.st0 + (int64_t)i1 * P.st1 + (int64_t)i2 * P.st2;
    return true;
}

// one product of a lag accumulator: Re(a conj(b)) for SLSC (a pair and its mirror sum to twice this), a b (no conjugate) for DMAS
template <int MODE, bool CPLX, typename R> __device__ inline void pair(R &ar, R &ai, Cx<R> a, Cx<R> b) {
    if constexpr (MODE == DMAS && CPLX) {
        ar += a.re * b.re - a.im * b.im;
        ai += a.re * b.im + a.im * b.re;
    } else if constexpr (CPLX) {
        ar += a.re * b.re + a.im * b.im;
    } else {
        ar += a.re * b.re;
    }
}

// SLSC (average / ensemble) and DMAS over a lag subset.
template <int MODE, typename R, bool CPLX, int C, int WPE, bool KD>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE))) coh_lags_kernel(Params P) {
    int64_t base; uint32_t p;
    if (!pixel(P, base, p)) return;
    constexpr int64_t ES = CPLX ? 2 : 1;
    const R *x = (const R *)P.x + base * ES;
    const int64_t dN = P.sN * ES;
    const uint32_t N = P.N;
    constexpr bool CACC = MODE == DMAS && CPLX;              // DMAS sums x_n x_{n+l} (no conjugate): complex accumulators
    R zr = R(0), zi = R(0);
    for (uint32_t l0 = 0; l0 <= P.maxlag; l0 += C) {
        const uint32_t bits = chunk_bits<C>(P, l0);
        if (!bits) continue;
        R ar[C], ai[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { ar[c] = R(0); ai[c] = R(0); }
        const uint32_t nend = N - l0;                        // receivers with a partner at lag l0
        for (uint32_t k = 0; k < P.K; ++k) {
            const int64_t koff = (int64_t)k * P.sK;
            Cx<R> w[C];                                      // slot (j + c) % C holds x(n + j + l0 + c) at step j of a block
            const R *pw = x + (int64_t)l0 * dN;
#pragma unroll
            for (int c = 0; c < C; ++c, pw += dN) w[c] = l0 + c < N ? sample<MODE, R, CPLX, KD>(P, pw, koff) : Cx<R>{R(0), R(0)};
            const R *pa = x;
            uint32_t n = 0;
            // whole blocks whose loads are all in range: no guards, the ring's slots are constants
            for (; n + l0 + 2 * C <= N; n += C) {
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const Cx<R> a = l0 == 0 ? w[j] : sample<MODE, R, CPLX, KD>(P, pa, koff);
                    pa += dN;
#pragma unroll
                    for (int c = 0; c < C; ++c) pair<MODE, CPLX>(ar[c], ai[c], a, w[(j + c) % C]);
                    w[j] = sample<MODE, R, CPLX, KD>(P, pw, koff);
                    pw += dN;
                }
            }
            // the last receivers (fewer than 2C): partners loaded directly
            for (; n < nend; ++n, pa += dN) {
                const Cx<R> a = sample<MODE, R, CPLX, KD>(P, pa, koff);
                const R *pb = pa + (int64_t)l0 * dN;
#pragma unroll
                for (int c = 0; c < C; ++c, pb += dN)
                    if (n + l0 + c < N) pair<MODE, CPLX>(ar[c], ai[c], a, sample<MODE, R, CPLX, KD>(P, pb, koff));
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (!((bits >> c) & 1u)) continue;
            const uint32_t l = l0 + c;
            if constexpr (MODE == AVG) {
                const R wt = l == 0 ? R(1) / (R(2) * R(P.lnorm) * R(N)) : R(1) / (R(P.lnorm) * R(N - l));
                zr += ar[c] * wt;
            } else if constexpr (MODE == ENS) {
                zr += l == 0 ? ar[c] : R(2) * ar[c];
            } else {
                zr += ar[c];
                if constexpr (CACC) zi += ai[c];
            }
        }
    }
    if constexpr (MODE == AVG) {
        if constexpr (CPLX) { ((R *)P.y)[2 * (uint64_t)p] = zr; ((R *)P.y)[2 * (uint64_t)p + 1] = R(0); }
        else ((R *)P.y)[p] = zr;
    } else if constexpr (MODE == ENS) {
        // a = b = sum over the pairs of the set of |x_n|^2 = sum_n cnt_n |x_n|^2, cnt_n = [0 in set] + #{l in set : l <= n} + #{l in set : l <= N-1-n}
        R a = R(0);
        uint32_t clo = 0, chi = P.ntot;
        for (uint32_t n = 0; n < N; ++n) {
            R e = R(0);
            for (uint32_t k = 0; k < P.K; ++k) e += mag2(sample<ENS, R, CPLX>(P, x + (int64_t)n * dN, (int64_t)k * P.sK));
            a += R(clo + chi + P.zero_lag) * e;
            if (n + 1 < N && inset(P, n + 1)) ++clo;
            if (N - 1 - n >= 1 && inset(P, N - 1 - n)) --chi;
        }
        const R ra = rsq(a), f = ra * ra;                    // nan2zero(rsqrt(a) rsqrt(b)): a = 0 gives Inf, and 0 * Inf = NaN as in MATLAB
        if constexpr (CPLX) { ((R *)P.y)[2 * (uint64_t)p] = zr * f; ((R *)P.y)[2 * (uint64_t)p + 1] = zi * f; }
        else ((R *)P.y)[p] = zr * f;
    } else {
        if constexpr (CPLX) {                                // exp(i angle(b)) sqrt(|b|) = b / sqrt(|b|); 0 stays 0, NaN stays NaN
            const R m = hypot(zr, zi);
            const R s = m > R(0) ? sqrt(m) / m : R(1);
            ((R *)P.y)[2 * (uint64_t)p] = zr * s; ((R *)P.y)[2 * (uint64_t)p + 1] = zi * s;
        } else {
            ((R *)P.y)[p] = copysign(sqrt(fabs(zr)), zr);   // sign(b) sqrt(|b|)
        }
    }
}

// DMAS over every lag 1 .. N-1: sum_{n<m} x_n x_m = ((sum x)^2 - sum x^2) / 2, O(N).  Contraction is off so that N = 1 gives exactly 0.
template <typename R, bool CPLX>
__global__ void __launch_bounds__(BLOCK) coh_dmas_all_kernel(Params P) {
#pragma clang fp contract(off)
    int64_t base; uint32_t p;
    if (!pixel(P, base, p)) return;
    const R *x = (const R *)P.x;
    R sr = R(0), si = R(0), qr = R(0), qi = R(0);
    for (uint32_t n = 0; n < P.N; ++n) {
        const Cx<R> v = ld<R, CPLX>(x, base + (int64_t)n * P.sN);
        sr += v.re; si += v.im;
        qr += v.re * v.re - v.im * v.im; qi += R(2) * v.re * v.im;
    }
    const R br = ((sr * sr - si * si) - qr) * R(0.5), bi = (R(2) * sr * si - qi) * R(0.5);
    if constexpr (CPLX) {
        const R m = hypot(br, bi);
        const R s = m > R(0) ? sqrt(m) / m : R(1);
        ((R *)P.y)[2 * (uint64_t)p] = br * s; ((R *)P.y)[2 * (uint64_t)p + 1] = bi * s;
    } else {
        ((R *)P.y)[p] = copysign(sqrt(fabs(br)), br);
    }
}

// cohfac: |sum b|^2 / sum |b|^2 / (N K) over the aperture and the second reduced dimension (kern/cohfac.m:64).  Real output; 0/0 stays NaN.
template <typename R, bool CPLX>
__global__ void __launch_bounds__(BLOCK) coh_cohfac_kernel(Params P) {
    int64_t base; uint32_t p;
    if (!pixel(P, base, p)) return;
    const R *x = (const R *)P.x;
    R sr = R(0), si = R(0), e = R(0);
    for (uint32_t k = 0; k < P.K; ++k)
        for (uint32_t n = 0; n < P.N; ++n) {
            const Cx<R> v = ld<R, CPLX>(x, base + (int64_t)n * P.sN + (int64_t)k * P.sK);
            sr += v.re; si += v.im; e += mag2(v);
        }
    ((R *)P.y)[p] = (sr * sr + si * si) / e / (R(P.N) * R(P.K));
}

// pcf: population standard deviations (omitnan) of angle(b) and of angle(b) - pi sign(angle(b)); sf = their min, w = max(0, 1 - g sf)
// (kern/pcf.m:71-107).  The variances are shifted by the first sample's phase, so the small spread of an in-focus pixel is not lost to
// a sum of squares of phases near +-pi.
template <typename R>
__global__ void __launch_bounds__(BLOCK) coh_pcf_kernel(Params P) {
    int64_t base; uint32_t p;
    if (!pixel(P, base, p)) return;
    const R *x = (const R *)P.x;
    const R pi = R(M_PI);
    R k0 = R(0), ka = R(0), d0 = R(0), q0 = R(0), da = R(0), qa = R(0);
    uint32_t cnt = 0;
    for (uint32_t n = 0; n < P.N; ++n) {
        const Cx<R> v = ld<R, true>(x, base + (int64_t)n * P.sN);
        const R ph = atan2(v.im, v.re);
        if (ph != ph) continue;
        const R pa = ph - pi * (ph > R(0) ? R(1) : (ph < R(0) ? R(-1) : R(0)));
        if (cnt == 0) { k0 = ph; ka = pa; }
        const R u = ph - k0, t = pa - ka;
        d0 += u; q0 += u * u; da += t; qa += t * t;
        ++cnt;
    }
    R w, sf;
    if (cnt == 0) { sf = R(NAN); w = R(0); }                  // max(0, NaN) is 0 in MATLAB
    else {
        const R c = R(cnt);
        const R s0 = sqrt(fmax(q0 / c - (d0 / c) * (d0 / c), R(0))), sa = sqrt(fmax(qa / c - (da / c) * (da / c), R(0)));
        sf = fmin(s0, sa);
        w = R(1) - R(P.g) * sf;
        w = w > R(0) ? w : R(0);
    }
    ((R *)P.y)[p] = w;
    ((R *)P.y2)[p] = sf;
}

template <int MODE, typename R, bool CPLX>
static void launch_lags(const Params &P, dim3 g, hipStream_t s) {
    constexpr int C = sizeof(R) == 4 ? 16 : 8, WPE = 1;   // chunk of lags; kernel-resource-usage: no scratch, no VGPR spill (C = 32 spills)
    if constexpr (MODE == AVG) {
        if (P.K > 1) { coh_lags_kernel<MODE, R, CPLX, C, WPE, true><<<g, BLOCK, 0, s>>>(P); return; }   // (the norm over the time kernel)
    }
    coh_lags_kernel<MODE, R, CPLX, C, WPE, false><<<g, BLOCK, 0, s>>>(P);
}

template <typename R, bool CPLX>
static void launch(int method, int dmas_all, const Params &P, hipStream_t s) {
    const dim3 g((P.P + BLOCK - 1) / BLOCK);
    switch (method) {
        case AVG: launch_lags<AVG, R, CPLX>(P, g, s); break;
        case ENS: launch_lags<ENS, R, CPLX>(P, g, s); break;
        case DMAS:
            if (dmas_all) coh_dmas_all_kernel<R, CPLX><<<g, BLOCK, 0, s>>>(P);
            else launch_lags<DMAS, R, CPLX>(P, g, s);
            break;
        case COHFAC: coh_cohfac_kernel<R, CPLX><<<g, BLOCK, 0, s>>>(P); break;
        case PCF: if constexpr (CPLX) coh_pcf_kernel<R><<<g, BLOCK, 0, s>>>(P); break;
    }
}

}  // namespace coh
}  // namespace qdas

using qdas::fail;

extern "C" int qdas_coherence(const qdas_coherence_desc *d, const void *x, void *y, void *y2, void *stream) {
    using namespace qdas::coh;
    if (!d) return fail(QDAS_EINVAL, "coherence: null descriptor");
    if (d->method < QDAS_COH_SLSC_AVERAGE || d->method > QDAS_COH_PCF) return fail(QDAS_EINVAL, "coherence: unknown method");
    if (d->dtype != QDAS_F64 && d->dtype != QDAS_F32) return fail(QDAS_EINVAL, "coherence: datatype must be double or single");
    if (d->N == 0) return fail(QDAS_EINVAL, "coherence: the aperture dimension is empty (N = 0)");
    const uint64_t K = d->K ? d->K : 1;
    if (d->method == QDAS_COH_PCF && !d->cplx) return fail(QDAS_EINVAL, "pcf: Input must be complex.");
    if (d->method == QDAS_COH_PCF && K != 1) return fail(QDAS_EINVAL, "pcf: one reduced dimension (K = 1)");
    if (d->method == QDAS_COH_DMAS && K != 1) return fail(QDAS_EINVAL, "dmas: one reduced dimension (K = 1)");
    uint64_t P = 1, sz[3];
    for (int i = 0; i < 3; ++i) { sz[i] = d->size[i]; P *= sz[i]; }   // (a size of 0 is an empty image: nothing is launched)
    if (d->N >= (1ull << 31) || K >= (1ull << 31) || P >= (1ull << 32) || sz[0] >= (1ull << 32) || sz[1] >= (1ull << 32))
        return fail(QDAS_EUNSUPPORTED, "coherence: at most 2^32 - 1 pixels and 2^31 - 1 receivers per call");

    Params p;
    memset(&p, 0, sizeof p);
    p.N = (uint32_t)d->N; p.K = (uint32_t)K; p.P = (uint32_t)P; p.s0 = (uint32_t)sz[0]; p.s1 = (uint32_t)sz[1];
    p.st0 = d->stride[0]; p.st1 = d->stride[1]; p.st2 = d->stride[2]; p.sN = d->strideN; p.sK = d->strideK;
    p.g = d->gamma / sqrt(M_PI / 3.0);
    int dmas_all = 0;
    const bool lagged = d->method == QDAS_COH_SLSC_AVERAGE || d->method == QDAS_COH_SLSC_ENSEMBLE || d->method == QDAS_COH_DMAS;
    if (lagged) {
        const bool slsc = d->method != QDAS_COH_DMAS;
        const uint64_t top = d->N - 1;                   // largest lag with pairs
        if (!d->lags) {                                  // the range [lag_lo, lag_hi]
            if (d->lag_hi < d->lag_lo) { if (slsc) return fail(QDAS_EINVAL, "slsc: empty lag set"); }
            else {
                p.lnorm = (double)(d->lag_hi - d->lag_lo + 1);
                p.zero_lag = slsc && d->lag_lo == 0;
                p.lo = (uint32_t)(d->lag_lo ? (d->lag_lo < top + 1 ? d->lag_lo : top + 1) : 1);
                p.hi = (uint32_t)(d->lag_hi < top ? d->lag_hi : top);
                p.maxlag = p.hi >= p.lo ? p.hi : 0;
                p.ntot = p.maxlag ? p.hi - p.lo + 1 : 0;
            }
        } else {                                         // a table: ismember / intersect semantics, duplicates only count in L
            if (d->nlags == 0) { if (slsc) return fail(QDAS_EINVAL, "slsc: empty lag set"); }
            p.lnorm = (double)d->nlags;
            for (uint64_t i = 0; i < d->nlags; ++i) {
                const int64_t l = d->lags[i];
                if (l < 0) return fail(QDAS_EINVAL, "coherence: lags must be non-negative");
                if (l == 0) { p.zero_lag = slsc; continue; }
                if ((uint64_t)l > top) continue;
                if ((uint64_t)l >= MASK_LAGS) return fail(QDAS_EUNSUPPORTED, "coherence: a lag table reaches at most lag 2047 (a range has no limit)");
                p.mask[l >> 5] |= 1u << (l & 31);
                if ((uint32_t)l > p.maxlag) p.maxlag = (uint32_t)l;
            }
            for (int w = 0; w < MASK_WORDS; ++w) p.ntot += (uint32_t)__builtin_popcount(p.mask[w]);
            p.use_mask = 1;
        }
        if (d->method == QDAS_COH_DMAS) {                // the full set 1 .. N-1 takes the O(N) form
            p.zero_lag = 0;
            dmas_all = d->N >= 2 && p.ntot == top;
        }
    }
    if (P == 0) return QDAS_OK;
    if (!x || !y || (d->method == QDAS_COH_PCF && !y2)) return fail(QDAS_EINVAL, "coherence: null data pointer");
    p.x = x; p.y = y; p.y2 = y2;
    int prev = -1;
    if (d->device >= 0) { if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(d->device) != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed"); }
    const hipStream_t s = (hipStream_t)stream;
    if (d->dtype == QDAS_F32) { if (d->cplx) launch<float, true>(d->method, dmas_all, p, s); else launch<float, false>(d->method, dmas_all, p, s); }
    else                      { if (d->cplx) launch<double, true>(d->method, dmas_all, p, s); else launch<double, false>(d->method, dmas_all, p, s); }
    const hipError_t e = hipGetLastError();
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
