// demod.hip -- qdas_demod: downmix, FIR low-pass and decimation of RF traces in one pass (the reference's recipe for baseband imaging, downmix -> filter ->
// downsample, src/ChannelData.m:757-807, :857-888, :1042-1058).  For x of T samples x C traces, real taps b[0 .. K-1] and an integer ratio R:
//
//   out[j, c] = sum_k b[k] x[jR - k, c] exp(-2 pi i frac(fc (t0_c + (jR - k) / fs))),   j = 0 .. ceil(T / R) - 1,   terms with jR - k < 0 omitted
//             = exp(-2 pi i (cyc0_c + j step)) sum_k (b[k] exp(+2 pi i k fc / fs)) x[jR - k]
//
// -- modulated taps once per workgroup, one phasor per output, two FMAs per tap for real input (four for complex input).
//
// MI355X mapping (the index arithmetic is demod_core.h, shared with a host test).  A workgroup is ONE wave and owns 256 consecutive outputs of one trace; a lane
// owns four consecutive outputs.  One wave, not four: the C3 record decimated by 4 has 704 outputs per trace -- three tiles of 256 waste 8 % of the lanes, a tile
// of 1024 would waste 31 % -- the barriers cost nothing, and the 5 - 13 KiB of LDS a tile needs leave a CU a dozen or more resident workgroups.
//   * The taps are split by k mod R into min(R, K) phases: phase s is a stride-1 FIR over the row x[nR - s].  The rows of up to 8 phases are staged in LDS at
//     a time (lanes along the global index: one coalesced sweep over the span when R <= 8), zero-filled before and behind the record, int16 widened there.
//     A phase without taps (K < R) is neither loaded nor multiplied, and a tap group's last, partial group multiplies only the taps that exist: no sample
//     meets a zero coefficient, so a NaN reaches exactly the outputs the contract names.
//   * LAYOUT.  A row is de-interleaved by (index mod 4), 4 = outputs per lane: a lane's sliding window advances by whole quads and the lanes of a wave read
//     consecutive elements of one plane -- conflict-free for 4-, 8- and 16-byte samples.  Splitting by (index mod R) alone would leave a stride of 4 between
//     lanes.  The planes are padded to 2 (mod 32) words (1 (mod 16) elements for wider samples) for the staging stores: demod_core.h.
//   * The workgroup forms the modulated taps itself: frac(k fc / fs) in float64, sincospi in the data's precision, K complex values in LDS, read uniformly
//     (one broadcast ds_read per tap per wave, next to one sample read per tap: 2 LDS reads per 8 (16) FMAs).
//   * The window is 8 registers for two tap groups: the second group loads into the upper half and reads the window rotated by 4 -- no copies (conv.hip).
//   * fp32 accumulators (fp64 for double data); the phasor is frac(cyc0 + frac(j step)) in float64, sincospi in the data's precision; one rounding at the
//     store.  The results go through LDS once so that the stores of a wave are consecutive.  No atomics: every output is written exactly once.
// LIMITS.  K <= 1024, R <= 4096 (QDAS_DEMOD_MAX_K, QDAS_DEMOD_MAX_R), C ceil(J / 256) < 2^31, T and the strides below 2^40.  With these every type fits 64 KiB of
// LDS (the worst case, K = 1024, R = 1, complex128: 16 KiB of taps and a 20.1 KiB row).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"
#include "demod_core.h"

namespace qdas {
namespace dm {

struct Params {
    const void *x, *b;
    void *out;
    const double *cyc0;
    int64_t T, J, K, R;
    uint64_t x_ld, out_ld, gdiv, G;
    uint32_t ntiles;
    Geom g;
    double fc_over_fs, step;
};

struct half2_t { _Float16 x, y; };

template <typename RT> struct Cx;
template <> struct Cx<float>  { using T = float2; };
template <> struct Cx<double> { using T = double2; };

__device__ __forceinline__ float  ld(const int16_t *p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ float  ld(const float *p, int64_t i)   { return p[i]; }
__device__ __forceinline__ float2 ld(const float2 *p, int64_t i)  { return p[i]; }
__device__ __forceinline__ double ld(const double *p, int64_t i)  { return p[i]; }
__device__ __forceinline__ double2 ld(const double2 *p, int64_t i) { return p[i]; }

__device__ __forceinline__ void zero(float &v)   { v = 0.f; }
__device__ __forceinline__ void zero(double &v)  { v = 0.0; }
__device__ __forceinline__ void zero(float2 &v)  { v = make_float2(0.f, 0.f); }
__device__ __forceinline__ void zero(double2 &v) { v = make_double2(0.0, 0.0); }

// acc += x * tap  (x real: 2 FMAs; x complex: 4)
__device__ __forceinline__ void mac(float2 &a, float x, float2 h)    { a.x = fmaf(x, h.x, a.x); a.y = fmaf(x, h.y, a.y); }
__device__ __forceinline__ void mac(double2 &a, double x, double2 h) { a.x = fma(x, h.x, a.x); a.y = fma(x, h.y, a.y); }
__device__ __forceinline__ void mac(float2 &a, float2 x, float2 h) {
    a.x = fmaf(x.x, h.x, a.x); a.x = fmaf(-x.y, h.y, a.x);
    a.y = fmaf(x.x, h.y, a.y); a.y = fmaf(x.y, h.x, a.y);
}
__device__ __forceinline__ void mac(double2 &a, double2 x, double2 h) {
    a.x = fma(x.x, h.x, a.x); a.x = fma(-x.y, h.y, a.x);
    a.y = fma(x.x, h.y, a.y); a.y = fma(x.y, h.x, a.y);
}

// cyc in [0, 1]: moved to [-1/2, 1/2] in float64 first, so that the rounding to the data's precision is at most 2^-26 cycles for float
__device__ __forceinline__ void sincos_cycles(double cyc, float &s, float &c)  { sincospif((float)(2.0 * centred(cyc)), &s, &c); }
__device__ __forceinline__ void sincos_cycles(double cyc, double &s, double &c) { sincospi(2.0 * centred(cyc), &s, &c); }

__device__ __forceinline__ void st(float2 *p, int64_t i, float2 v)   { p[i] = v; }
__device__ __forceinline__ void st(double2 *p, int64_t i, double2 v) { p[i] = v; }
__device__ __forceinline__ void st(half2_t *p, int64_t i, float2 v)  { p[i] = half2_t{(_Float16)v.x, (_Float16)v.y}; }

// RT: compute precision; TX: a staged sample (RT or its complex); SIN: a sample in memory; OUT: an output element
template <typename RT, typename TX, typename SIN, typename OUT>
__global__ void __launch_bounds__(LANES) demod_kernel(const Params P) {
    using CT = typename Cx<RT>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char dm_lds[];
    CT *H = (CT *)dm_lds;
    TX *X = (TX *)(dm_lds + P.g.tap_bytes);
    const int t = threadIdx.x;
    const uint32_t tile = blockIdx.x % P.ntiles;
    const uint64_t c = blockIdx.x / P.ntiles;
    const SIN *__restrict__ x = (const SIN *)P.x + c * P.x_ld;
    const int K = (int)P.K, NG = P.g.NG, QP = P.g.QP, EN = P.g.EN, S = P.g.S, PG = P.g.PG;
    const int64_t R = P.R, T = P.T;
    const int64_t j0 = (int64_t)tile * TILE;

    {   // the modulated taps
        const RT *__restrict__ b = (const RT *)P.b;
        for (int k = t; k < K; k += LANES) {
            RT s, co;
            sincos_cycles(tap_cycles(k, P.fc_over_fs), s, co);
            const RT bk = b[k];
            CT h; h.x = bk * co; h.y = bk * s;
            H[k] = h;
        }
    }

    CT acc[OPL];
#pragma unroll
    for (int r = 0; r < OPL; ++r) zero(acc[r]);

    for (int sa = 0; sa < S; sa += PG) {
        const int pg = (S - sa < PG) ? S - sa : PG;                       // (uniform)
        __syncthreads();                                                  // the previous group's window reads are done
        {   // stage EN elements of pg phases: lane index l = e pg + d along the global index (phase sa + d of element e is sample (n0 + e) R - sa - d)
            const int de = LANES / pg, dd = LANES % pg;
            int d = t % pg, e = t / pg;
            while (e < EN) {                                              // four loads in flight before the first LDS write
                TX v[4]; int w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    zero(v[q]);
                    w[q] = -1;
                    if (e < EN) {
                        const int64_t i = sample_index(j0, NG, e, R, sa + d);
                        if (i >= 0 && i < T) v[q] = ld(x, i);
                        w[q] = lds_word(d, e, QP);
                    }
                    d += dd; e += de;
                    if (d >= pg) { d -= pg; ++e; }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (w[q] >= 0) X[w[q]] = v[q];
            }
        }
        __syncthreads();
        for (int d = 0; d < pg; ++d) {
            const int s = sa + d;
            const int ms = last_tap(K, R, s);                             // (uniform) taps m = 0 .. ms of this phase: k = m R + s
            const TX *row = X + d * OPL * QP;
            const CT *h = H + s;
            TX win[2 * OPL];                                              // win[w + OPL] = row element OPL (NG + t - g) + w, w = -OPL .. OPL-1
            int q = window_quad(NG, t, 0, 0);
#pragma unroll
            for (int w = 0; w < OPL; ++w) win[OPL + w] = row[w * QP + q];
            for (int g = 0; OPL * g <= ms; g += 2) {
                q = window_quad(NG, t, g, -1);                            // group g brings the quad below its own: window entries -OPL .. -1
#pragma unroll
                for (int w = 0; w < OPL; ++w) win[w] = row[w * QP + q];
                const int m0 = OPL * g;
                if (m0 + OPL - 1 <= ms) {
#pragma unroll
                    for (int u = 0; u < OPL; ++u) {
                        const CT tap = h[(int64_t)(m0 + u) * R];
#pragma unroll
                        for (int r = 0; r < OPL; ++r) mac(acc[r], win[OPL + r - u], tap);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < OPL; ++u)
                        if (m0 + u <= ms) {
                            const CT tap = h[(int64_t)(m0 + u) * R];
#pragma unroll
                            for (int r = 0; r < OPL; ++r) mac(acc[r], win[OPL + r - u], tap);
                        }
                }
                if (m0 + OPL <= ms) {
                    q = window_quad(NG, t, g + 1, -1);
#pragma unroll
                    for (int w = 0; w < OPL; ++w) win[OPL + w] = row[w * QP + q];
                    const int m1 = m0 + OPL;
                    if (m1 + OPL - 1 <= ms) {
#pragma unroll
                        for (int u = 0; u < OPL; ++u) {
                            const CT tap = h[(int64_t)(m1 + u) * R];
#pragma unroll
                            for (int r = 0; r < OPL; ++r) mac(acc[r], win[(2 * OPL + r - u) & (2 * OPL - 1)], tap);
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < OPL; ++u)
                            if (m1 + u <= ms) {
                                const CT tap = h[(int64_t)(m1 + u) * R];
#pragma unroll
                                for (int r = 0; r < OPL; ++r) mac(acc[r], win[(2 * OPL + r - u) & (2 * OPL - 1)], tap);
                            }
                    }
                }
            }
        }
    }

    // lane-major results -> output-major through LDS, the phasor, one rounding, consecutive stores
    __syncthreads();
    CT *O = (CT *)(dm_lds + P.g.tap_bytes);
#pragma unroll
    for (int r = 0; r < OPL; ++r) O[out_word(OPL * t + r, (int)sizeof(CT))] = acc[r];
    __syncthreads();
    const double cyc0 = P.cyc0[(c / P.gdiv) % P.G];
    OUT *__restrict__ out = (OUT *)P.out + c * P.out_ld;
#pragma unroll
    for (int q = 0; q < OPL; ++q) {
        const int e = t + LANES * q;
        const int64_t j = j0 + e;
        if (j < P.J) {
            const CT a = O[out_word(e, (int)sizeof(CT))];
            RT s, co;
            sincos_cycles(out_cycles(cyc0, j, P.step), s, co);
            CT v;
            v.x = fma(a.y, s, a.x * co);
            v.y = fma(-a.x, s, a.y * co);
            st(out, j, v);
        }
    }
}

template <typename RT, typename TX, typename SIN, typename OUT>
static void launch(const Params &p, hipStream_t s, uint64_t nwg) {
    demod_kernel<RT, TX, SIN, OUT><<<dim3((uint32_t)nwg), dim3(LANES), p.g.lds_bytes, s>>>(p);
}

static bool is_finite(double v) { return v - v == 0.0; }

}  // namespace dm
}  // namespace qdas

using qdas::fail;

extern "C" uint64_t qdas_demod_len(uint64_t T, uint64_t R) { return qdas::dm::out_len(T, R); }

extern "C" int qdas_demod(const qdas_demod_desc *d, const void *x, const void *b, void *out) {
    using namespace qdas::dm;
    static_assert(QDAS_DEMOD_MAX_K == MAX_K && QDAS_DEMOD_MAX_R == MAX_R && QDAS_DEMOD_TILE == TILE, "limits of include/qdas.h");
    if (!d) return fail(QDAS_EINVAL, "demod: null descriptor");
    if (d->in_type < QDAS_DEMOD_I16 || d->in_type > QDAS_DEMOD_C128) return fail(QDAS_EINVAL, "demod: unknown in_type %d", d->in_type);
    if (d->out_half != 0 && d->out_half != 1) return fail(QDAS_EINVAL, "demod: out_half is 0 or 1, got %d", d->out_half);
    const bool dbl = d->in_type == QDAS_DEMOD_F64 || d->in_type == QDAS_DEMOD_C128;
    if (d->out_half && dbl) return fail(QDAS_EINVAL, "demod: out_half goes with int16, float32 and complex64 input, not with double data");
    if (d->R == 0) return fail(QDAS_EINVAL, "demod: the ratio R must be at least 1");
    if (d->K == 0) return fail(QDAS_EINVAL, "demod: the filter needs at least one tap (K = 0)");
    if (d->G == 0 || d->gdiv == 0) return fail(QDAS_EINVAL, "demod: G and gdiv must be at least 1, got G = %llu, gdiv = %llu", (unsigned long long)d->G, (unsigned long long)d->gdiv);
    if (!is_finite(d->fc_over_fs) || !is_finite(d->step)) return fail(QDAS_EINVAL, "demod: fc_over_fs and step must be finite");
    const uint64_t J = out_len(d->T, d->R);
    if (d->x_ld < d->T) return fail(QDAS_EINVAL, "demod: x_ld = %llu is less than T = %llu", (unsigned long long)d->x_ld, (unsigned long long)d->T);
    if (d->out_ld < J) return fail(QDAS_EINVAL, "demod: out_ld = %llu is less than J = ceil(T / R) = %llu", (unsigned long long)d->out_ld, (unsigned long long)J);
    if (d->T == 0 || d->C == 0) return QDAS_OK;
    if (!x || !b || !out || !d->cyc0) return fail(QDAS_EINVAL, "demod: null pointer (%s)", !x ? "x" : !b ? "b" : !out ? "out" : "cyc0");
    if (d->K > (uint64_t)MAX_K || d->R > (uint64_t)MAX_R)
        return fail(QDAS_EUNSUPPORTED, "demod: K = %llu, R = %llu: at most %lld taps and a ratio of %lld (the taps and one phase of the span live in 64 KiB of LDS)",
                    (unsigned long long)d->K, (unsigned long long)d->R, (long long)MAX_K, (long long)MAX_R);
    const uint64_t LIM = 1ull << 40;
    if (d->T >= LIM || d->x_ld >= LIM || d->out_ld >= LIM || d->C >= LIM) return fail(QDAS_EUNSUPPORTED, "demod: T, C, x_ld or out_ld reach 2^40");
    const uint64_t ntiles = (J + TILE - 1) / TILE;
    if (ntiles * d->C >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "demod: more than 2^31 - 1 workgroups (%d outputs of one trace each)", TILE);
    const bool cplx = d->in_type == QDAS_DEMOD_C64 || d->in_type == QDAS_DEMOD_C128;
    const int real_bytes = dbl ? 8 : 4;
    Params p;
    memset(&p, 0, sizeof p);
    p.g = geometry((int64_t)d->K, (int64_t)d->R, cplx ? 2 * real_bytes : real_bytes, 2 * real_bytes);
    if (p.g.PG < 1 || p.g.lds_bytes > LDS_MAX) return fail(QDAS_EUNSUPPORTED, "demod: K = %llu, R = %llu do not fit 64 KiB of LDS", (unsigned long long)d->K, (unsigned long long)d->R);
    p.x = x; p.b = b; p.out = out; p.cyc0 = d->cyc0;
    p.T = (int64_t)d->T; p.J = (int64_t)J; p.K = (int64_t)d->K; p.R = (int64_t)d->R;
    p.x_ld = d->x_ld; p.out_ld = d->out_ld; p.gdiv = d->gdiv; p.G = d->G;
    p.ntiles = (uint32_t)ntiles;
    p.fc_over_fs = d->fc_over_fs; p.step = d->step;

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    const uint64_t nwg = ntiles * d->C;
    switch (d->in_type) {
        case QDAS_DEMOD_I16: if (d->out_half) launch<float, float, int16_t, half2_t>(p, s, nwg); else launch<float, float, int16_t, float2>(p, s, nwg); break;
        case QDAS_DEMOD_F32: if (d->out_half) launch<float, float, float, half2_t>(p, s, nwg); else launch<float, float, float, float2>(p, s, nwg); break;
        case QDAS_DEMOD_C64: if (d->out_half) launch<float, float2, float2, half2_t>(p, s, nwg); else launch<float, float2, float2, float2>(p, s, nwg); break;
        case QDAS_DEMOD_F64: launch<double, double, double, double2>(p, s, nwg); break;
        default:             launch<double, double2, double2, double2>(p, s, nwg); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
