// resample.hip -- qdas_resample: a rational-rate polyphase FIR along time.  For x of T samples x C traces, real taps h[0 .. K-1], integers p, q >= 1, an
// offset off >= 0 and an output count J:
//
//   out[j + c out_ld] = sum_i h[off + j q - i p] X_c[i],   j = 0 .. J-1,   over every integer i with 0 <= off + j q - i p < K
//
// with X = x inside the record and zeros (edge ZERO) or the odd reflection (edge ODD) outside: upfirdn, MATLAB's uniform resample(x, p, q) / scipy's
// resample_poly, the FIR filtfilt (p = q = 1, h = b * flip(b), ODD) and a plain FIR at any integer offset are this one formula (include/qdas.h).
//
// MI355X mapping (the index arithmetic is resample_core.h, shared with a host test).  A workgroup of min(max(TJ, 64), 256) lanes owns TJ consecutive outputs of
// one trace, TJ a power of two chosen from (K, p, q, element bytes): 1024 when the taps and the span fit 40 KiB, fewer when q/p is large.
//   * The span the tile reads is staged ONCE, lanes along the global index (coalesced), the edge rule applied while staging, int16 widened there.
//   * The taps sit in LDS in their own order, K words: tap m of phase phi at word phi + m p (resample_core.h says why no per-phase rows).
//   * Lane t owns outputs j0 + t + r lanes, r = 0 .. 3: a wave's stores are consecutive without a transpose.  n = off + j q is carried as (n div p, n mod p):
//     one 64-bit division per tile (uniform), one 32-bit division per lane for its first output, a carry per output after that.
//   * The tap loop runs m = 0 .. Mmax - (phi > rem): only taps that exist, so no sample meets a zero coefficient and a NaN reaches exactly the outputs the
//     contract names.  One accumulator per output, taps in ascending m: fp32 FMAs (fp64 for double data), no rounding besides.
//   * p = 1 (filtfilt, a plain FIR, decimation): all outputs share the taps, and a lane reads each tap once for its up to four outputs (fir_shared_taps).
//   * LDS CONFLICTS.  Tap reads: the lanes of a wave hold at most p different phases, identical addresses broadcast, phases 32 apart collide (p > 32).  Sample
//     reads: lane t reads span element b_t + Mmax - m, b_t = ((f0 + t q) div p): a stride of q/p elements between lanes.  q <= p: neighbouring lanes share
//     elements (broadcast) or advance by one -- conflict-free.  q/p = 2, 4, ...: a 2-, 4-, ...-way conflict for 4-byte samples, left in place:
//     those are the decimating rates, where the loop is short (K/p taps for q/p times as many inputs) and the staging sweep, not the tap loop, sets the time.
//   * No atomics, every output written exactly once, no work space, no allocation, no synchronisation.
// LIMITS.  K <= 8192, p, q <= 4096 (QDAS_RESAMPLE_MAX_K, _MAX_PQ), and the K taps plus the span of ONE output
// ((K-1)/p + 1 samples) within 64 KiB; C ceil(J / TJ) < 2^31; T, C, J, off and the strides below 2^40.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"
#include "resample_core.h"

namespace qdas {
namespace rs {

struct Params {
    const void *x, *h;
    void *out;
    int64_t T, J, off;
    uint64_t x_ld, out_ld;
    uint32_t ntiles;
    int32_t K, p, q, edge;
    int32_t qd, qm;         // q div p, q mod p
    int32_t sd, sm;         // (lanes q) div p, (lanes q) mod p
    Geom g;
};

__device__ __forceinline__ float  ld(const int16_t *p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ float  ld(const float *p, int64_t i)   { return p[i]; }
__device__ __forceinline__ float2 ld(const float2 *p, int64_t i)  { return p[i]; }
__device__ __forceinline__ double ld(const double *p, int64_t i)  { return p[i]; }
__device__ __forceinline__ double2 ld(const double2 *p, int64_t i) { return p[i]; }

__device__ __forceinline__ void zero(float &v)   { v = 0.f; }
__device__ __forceinline__ void zero(double &v)  { v = 0.0; }
__device__ __forceinline__ void zero(float2 &v)  { v = make_float2(0.f, 0.f); }
__device__ __forceinline__ void zero(double2 &v) { v = make_double2(0.0, 0.0); }

// 2 a - v: the odd reflection about the end sample a (2 a is exact: one rounding)
__device__ __forceinline__ float   reflect(float a, float v)     { return 2.f * a - v; }
__device__ __forceinline__ double  reflect(double a, double v)   { return 2.0 * a - v; }
__device__ __forceinline__ float2  reflect(float2 a, float2 v)   { return make_float2(2.f * a.x - v.x, 2.f * a.y - v.y); }
__device__ __forceinline__ double2 reflect(double2 a, double2 v) { return make_double2(2.0 * a.x - v.x, 2.0 * a.y - v.y); }

__device__ __forceinline__ void mac(float &a, float x, float h)     { a = fmaf(x, h, a); }
__device__ __forceinline__ void mac(double &a, double x, double h)  { a = fma(x, h, a); }
__device__ __forceinline__ void mac(float2 &a, float2 x, float h)   { a.x = fmaf(x.x, h, a.x); a.y = fmaf(x.y, h, a.y); }
__device__ __forceinline__ void mac(double2 &a, double2 x, double h) { a.x = fma(x.x, h, a.x); a.y = fma(x.y, h, a.y); }

// p = 1: every output has phase 0 and the taps h[0 .. K-1], so a lane reads each tap ONCE for its R outputs (j0 + t + r lanes: span element (t + r lanes) q +
// Mmax - m): R + 1 LDS reads per R FMAs instead of 2 R.  The same indices, the same ascending order and one accumulator per output as the general loop.
// An output beyond the tile's last (jj >= nj) computes output 0 again and is not stored.
template <int R, typename RT, typename TX>
__device__ __forceinline__ void fir_shared_taps(const RT *H, const TX *X, TX *__restrict__ out, int t, int lanes, int nj, int q, int Mmax) {
    TX acc[R];
    const TX *xp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        zero(acc[r]);
        const int jj = t + r * lanes;
        xp[r] = X + ((jj < nj ? jj : 0) * q + Mmax);
    }
    for (int m = 0; m <= Mmax; ++m) {
        const RT hm = H[m];
#pragma unroll
        for (int r = 0; r < R; ++r) mac(acc[r], xp[r][-m], hm);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (t + r * lanes < nj) out[t + r * lanes] = acc[r];
}

// RT: a tap; TX: a staged sample and an output element (RT or its complex); SIN: a sample in memory
template <typename RT, typename TX, typename SIN>
__global__ void __launch_bounds__(LANES_MAX) resample_kernel(const Params P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    RT *H = (RT *)rs_lds;
    TX *X = (TX *)(rs_lds + P.g.tap_bytes);
    const int t = threadIdx.x, lanes = P.g.lanes;
    const uint32_t tile = blockIdx.x % P.ntiles;
    const uint64_t c = blockIdx.x / P.ntiles;
    const SIN *__restrict__ x = (const SIN *)P.x + c * P.x_ld;
    const int K = P.K, p = P.p, Mmax = P.g.Mmax, rem = P.g.rem;
    const int64_t j0 = (int64_t)tile * P.g.TJ, T = P.T;
    const int nj = (int)(P.J - j0 < P.g.TJ ? P.J - j0 : P.g.TJ);
    const Tile tl = tile_extent(P.off, j0, nj, p, P.q, Mmax);

    {   // the taps
        const RT *__restrict__ h = (const RT *)P.h;
        for (int k = t; k < K; k += lanes) H[k] = h[k];
    }
    for (int e = t; e < tl.len; e += lanes) {           // the span, once, with the edge rule
        int64_t anchor;
        const int64_t src = edge_source(tl.i_lo + e, T, P.edge, anchor);
        TX v;
        zero(v);
        if (src >= 0) {
            v = ld(x, src);
            if (anchor >= 0) v = reflect(ld(x, anchor), v);
        }
        X[e] = v;
    }
    __syncthreads();

    TX *__restrict__ out = (TX *)P.out + c * P.out_ld + j0;
    if (p == 1) {                                       // (uniform)
        if (nj > 3 * lanes) fir_shared_taps<4>(H, X, out, t, lanes, nj, P.q, Mmax);
        else if (nj > 2 * lanes) fir_shared_taps<3>(H, X, out, t, lanes, nj, P.q, Mmax);
        else if (nj > lanes) fir_shared_taps<2>(H, X, out, t, lanes, nj, P.q, Mmax);
        else fir_shared_taps<1>(H, X, out, t, lanes, nj, P.q, Mmax);
        return;
    }
    int b, phi;
    lane_start(tl.f0, t, p, P.qd, P.qm, b, phi);
    for (int jj = t; jj < nj; jj += lanes) {
        TX acc;
        zero(acc);
        const int ms = last_tap(Mmax, rem, phi);
        const RT *hp = H + tap_word(phi, 0, p);
        const TX *xp = X + (b + Mmax);
        int m = 0;
        for (; m + 3 <= ms; m += 4) {
            const RT h0 = hp[m * p], h1 = hp[(m + 1) * p], h2 = hp[(m + 2) * p], h3 = hp[(m + 3) * p];
            const TX x0 = xp[-m], x1 = xp[-m - 1], x2 = xp[-m - 2], x3 = xp[-m - 3];
            mac(acc, x0, h0); mac(acc, x1, h1); mac(acc, x2, h2); mac(acc, x3, h3);
        }
        for (; m <= ms; ++m) mac(acc, xp[-m], hp[m * p]);
        out[jj] = acc;
        advance(b, phi, P.sd, P.sm, p);
    }
}

template <typename RT, typename TX, typename SIN>
static void launch(const Params &p, hipStream_t s, uint64_t nwg) {
    resample_kernel<RT, TX, SIN><<<dim3((uint32_t)nwg), dim3((uint32_t)p.g.lanes), p.g.lds_bytes, s>>>(p);
}

}  // namespace rs
}  // namespace qdas

using qdas::fail;

extern "C" uint64_t qdas_resample_len(uint64_t T, uint64_t p, uint64_t q) { return qdas::rs::resample_len(T, p, q); }
extern "C" uint64_t qdas_upfirdn_len(uint64_t T, uint64_t K, uint64_t p, uint64_t q) { return qdas::rs::upfirdn_len(T, K, p, q); }

extern "C" int qdas_resample(const qdas_resample_desc *d, const void *x, const void *h, void *out) {
    using namespace qdas::rs;
    typedef unsigned long long ull;
    static_assert(QDAS_RESAMPLE_MAX_K == MAX_K && QDAS_RESAMPLE_MAX_PQ == MAX_PQ && QDAS_RESAMPLE_ZERO == EDGE_ZERO && QDAS_RESAMPLE_ODD == EDGE_ODD,
                  "limits and codes of include/qdas.h");
    if (!d) return fail(QDAS_EINVAL, "resample: null descriptor");
    if (d->in_type < QDAS_RESAMPLE_I16 || d->in_type > QDAS_RESAMPLE_C128) return fail(QDAS_EINVAL, "resample: unknown in_type %d", d->in_type);
    if (d->edge != QDAS_RESAMPLE_ZERO && d->edge != QDAS_RESAMPLE_ODD) return fail(QDAS_EINVAL, "resample: edge is QDAS_RESAMPLE_ZERO or _ODD, got %d", d->edge);
    if (d->p == 0 || d->q == 0) return fail(QDAS_EINVAL, "resample: p and q must be at least 1, got p = %llu, q = %llu", (ull)d->p, (ull)d->q);
    if (d->K == 0) return fail(QDAS_EINVAL, "resample: the filter needs at least one tap (K = 0)");
    if (d->x_ld < d->T) return fail(QDAS_EINVAL, "resample: x_ld = %llu is less than T = %llu", (ull)d->x_ld, (ull)d->T);
    if (d->out_ld < d->J) return fail(QDAS_EINVAL, "resample: out_ld = %llu is less than J = %llu", (ull)d->out_ld, (ull)d->J);
    if (d->J == 0 || d->C == 0) return QDAS_OK;
    if (d->T == 0) return fail(QDAS_EINVAL, "resample: a record of T = 0 samples has no outputs to give (J = %llu)", (ull)d->J);
    if (d->K > (uint64_t)MAX_K || d->p > (uint64_t)MAX_PQ || d->q > (uint64_t)MAX_PQ)
        return fail(QDAS_EUNSUPPORTED, "resample: K = %llu, p = %llu, q = %llu: at most %lld taps and rate terms of %lld", (ull)d->K, (ull)d->p, (ull)d->q,
                    (long long)MAX_K, (long long)MAX_PQ);
    const uint64_t LIM = 1ull << 40;
    if (d->T >= LIM || d->x_ld >= LIM || d->out_ld >= LIM || d->C >= LIM || d->J >= LIM || d->off >= LIM)
        return fail(QDAS_EUNSUPPORTED, "resample: T, C, J, off, x_ld or out_ld reach 2^40");
    if (d->edge == QDAS_RESAMPLE_ODD) {
        int64_t lo = 0, hi = 0;
        if (reach((int64_t)d->off, (int64_t)d->J, (int64_t)d->p, (int64_t)d->q, (int64_t)d->K, lo, hi) &&
            (lo < -((int64_t)d->T - 1) || hi > 2 * ((int64_t)d->T - 1)))
            return fail(QDAS_EINVAL, "resample: with the odd edge the outputs read x[%lld .. %lld], beyond the reflection's reach [%lld, %lld] of T = %llu samples",
                        (long long)lo, (long long)hi, -((long long)d->T - 1), 2 * ((long long)d->T - 1), (ull)d->T);
    }
    if (!x || !h || !out) return fail(QDAS_EINVAL, "resample: null pointer (%s)", !x ? "x" : !h ? "h" : "out");
    const bool dbl = d->in_type == QDAS_RESAMPLE_F64 || d->in_type == QDAS_RESAMPLE_C128;
    const bool cplx = d->in_type == QDAS_RESAMPLE_C64 || d->in_type == QDAS_RESAMPLE_C128;
    const int real_bytes = dbl ? 8 : 4;
    Params P;
    memset(&P, 0, sizeof P);
    P.g = geometry((int64_t)d->K, (int64_t)d->p, (int64_t)d->q, cplx ? 2 * real_bytes : real_bytes, real_bytes);
    if (P.g.TJ < 1 || P.g.lds_bytes > LDS_MAX)
        return fail(QDAS_EUNSUPPORTED, "resample: K = %llu taps at p = %llu do not fit 64 KiB of LDS with the span of one output", (ull)d->K, (ull)d->p);
    const uint64_t ntiles = (d->J + (uint64_t)P.g.TJ - 1) / (uint64_t)P.g.TJ;
    if (ntiles * d->C >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "resample: more than 2^31 - 1 workgroups (%d outputs of one trace each)", P.g.TJ);
    P.x = x; P.h = h; P.out = out;
    P.T = (int64_t)d->T; P.J = (int64_t)d->J; P.off = (int64_t)d->off;
    P.x_ld = d->x_ld; P.out_ld = d->out_ld;
    P.ntiles = (uint32_t)ntiles;
    P.K = (int32_t)d->K; P.p = (int32_t)d->p; P.q = (int32_t)d->q; P.edge = d->edge;
    P.qd = P.q / P.p; P.qm = P.q % P.p;
    const int64_t lq = (int64_t)P.g.lanes * P.q;
    P.sd = (int32_t)(lq / P.p); P.sm = (int32_t)(lq % P.p);

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    const uint64_t nwg = ntiles * d->C;
    switch (d->in_type) {
        case QDAS_RESAMPLE_I16: launch<float, float, int16_t>(P, s, nwg); break;
        case QDAS_RESAMPLE_F32: launch<float, float, float>(P, s, nwg); break;
        case QDAS_RESAMPLE_C64: launch<float, float2, float2>(P, s, nwg); break;
        case QDAS_RESAMPLE_F64: launch<double, double, double>(P, s, nwg); break;
        default:                launch<double, double2, double2>(P, s, nwg); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
