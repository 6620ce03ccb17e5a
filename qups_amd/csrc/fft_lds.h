// fft_lds.h -- the argument-independent pieces of the in-LDS mixed-radix Stockham transforms (internal): packed-complex helpers, the small DFT networks,
// the padded LDS index and the stage factorisation.  pre.hip (hilbert, FFT convolution) and migration.hip build their stages from these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qdas {

// Stage s has radix r[s]; the largest odd radix goes first (fft_factor)
struct FftStages { int n; int r[14]; };

// complex arithmetic on packed fp32 (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: one instruction per complex add, two per complex multiply)
typedef float pre_v2f __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ pre_v2f pv(float2 a) { return (pre_v2f){a.x, a.y}; }
static __device__ __forceinline__ float2 pf(pre_v2f a) { return make_float2(a.x, a.y); }
static __device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    const pre_v2f bb = pv(b);
    return pf((pre_v2f){-a.y, a.y} * bb.yx + (pre_v2f){a.x, a.x} * bb);
}
static __device__ __forceinline__ float2 caddf(float2 a, float2 b) { return pf(pv(a) + pv(b)); }
static __device__ __forceinline__ float2 csubf(float2 a, float2 b) { return pf(pv(a) - pv(b)); }
static __device__ __forceinline__ float2 cmulmi(float2 a) { return make_float2(a.y, -a.x); }              // a * (-i)

// length-4 DFT of (a, b, c, d) in place
static __device__ __forceinline__ void dft4(float2 &a, float2 &b, float2 &c, float2 &d) {
    const float2 s02 = caddf(a, c), d02 = csubf(a, c), s13 = caddf(b, d), d13 = cmulmi(csubf(b, d));
    a = caddf(s02, s13); c = csubf(s02, s13); b = caddf(d02, d13); d = csubf(d02, d13);
}

// exp(-2 pi i m / 16), m = 0..9
static __device__ __forceinline__ float2 w16(int m) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
    switch (m) {
        case 0: return make_float2(1.f, 0.f);
        case 1: return make_float2(C1, -S1);
        case 2: return make_float2(H, -H);
        case 3: return make_float2(S1, -C1);
        case 4: return make_float2(0.f, -1.f);
        case 5: return make_float2(-S1, -C1);
        case 6: return make_float2(-H, -H);
        case 7: return make_float2(-C1, -S1);
        case 8: return make_float2(-1.f, 0.f);
        default: return make_float2(-C1, S1);
    }
}

// length-R DFT of v in place.  2, 4, 8, 16: split-radix style networks with literal constants; odd R: the R x R product with
// wr[m] = exp(-2 pi i m / R) (uniform loads from the plan's table)
template <int R> static __device__ __forceinline__ void dft_small(float2 (&v)[R], const float2 *__restrict__ tw, uint32_t NR) {
    if constexpr (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = caddf(a, b); v[1] = csubf(a, b);
    } else if constexpr (R == 4) {
        dft4(v[0], v[1], v[2], v[3]);
    } else if constexpr (R == 8) {                                       // t = 2a + b, u = u1 + 4 u2
        dft4(v[0], v[2], v[4], v[6]);                                    // y0[u1]
        dft4(v[1], v[3], v[5], v[7]);                                    // y1[u1]
        v[3] = cmulf(v[3], w16(2)); v[5] = cmulmi(v[5]); v[7] = cmulf(v[7], w16(6));
        float2 o[8];
#pragma unroll
        for (int u1 = 0; u1 < 4; ++u1) { o[u1] = caddf(v[2 * u1], v[2 * u1 + 1]); o[u1 + 4] = csubf(v[2 * u1], v[2 * u1 + 1]); }
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = o[u];
    } else if constexpr (R == 16) {                                      // t = 4a + b, u = u1 + 4 u2
#pragma unroll
        for (int b = 0; b < 4; ++b) dft4(v[b], v[4 + b], v[8 + b], v[12 + b]);      // y_b[u1] sits in v[4 u1 + b]
#pragma unroll
        for (int u1 = 1; u1 < 4; ++u1)
#pragma unroll
            for (int b = 1; b < 4; ++b) v[4 * u1 + b] = cmulf(v[4 * u1 + b], w16(b * u1));
        float2 o[16];
#pragma unroll
        for (int u1 = 0; u1 < 4; ++u1) {
            dft4(v[4 * u1], v[4 * u1 + 1], v[4 * u1 + 2], v[4 * u1 + 3]);           // over b -> u2
#pragma unroll
            for (int u2 = 0; u2 < 4; ++u2) o[u1 + 4 * u2] = v[4 * u1 + u2];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = o[u];
    } else {                                                             // odd R: pair the points t and R - t
        static_assert(R % 2 == 1, "even radices have their own networks");
        constexpr int H = (R - 1) / 2;
        float c[H + 1], sn[H + 1];                                       // cos, sin of 2 pi m / R, m = 0..H (uniform loads; m = 0 occurs for R = 9)
        c[0] = 1.f; sn[0] = 0.f;
#pragma unroll
        for (int m = 1; m <= H; ++m) { const float2 w = tw[m * NR]; c[m] = w.x; sn[m] = -w.y; }
        float2 a[H + 1], b[H + 1];
#pragma unroll
        for (int t = 1; t <= H; ++t) { a[t] = caddf(v[t], v[R - t]); b[t] = csubf(v[t], v[R - t]); }
        const float2 v0 = v[0];
        float2 sum = v0;
#pragma unroll
        for (int t = 1; t <= H; ++t) sum = caddf(sum, a[t]);
        v[0] = sum;
#pragma unroll
        for (int u = 1; u <= H; ++u) {                                   // X[u] = P - i Q, X[R-u] = P + i Q
            float2 P = v0, Q = make_float2(0.f, 0.f);
#pragma unroll
            for (int t = 1; t <= H; ++t) {
                const int m = (u * t) % R;                               // cos(2 pi m/R) = cos(2 pi (R-m)/R), sin flips
                const float cc = m <= H ? c[m] : c[R - m], ss = m <= H ? sn[m] : -sn[R - m];
                P = pf(pv(a[t]) * cc + pv(P)); Q = pf(pv(b[t]) * ss + pv(Q));
            }
            v[u] = make_float2(P.x + Q.y, P.y - Q.x);
            v[R - u] = make_float2(P.x - Q.y, P.y + Q.x);
        }
    }
}

// LDS index of point i: one spare slot per 16 points, so that the stride-r writes of the early stages (points r j + t: 128-byte strides for
// r = 16 -- every second lane on the same pair of banks) spread over all banks
static __device__ __forceinline__ uint32_t lds_pad(uint32_t i) { return i + (i >> 4); }

// N <= 8192 = product of radices {16, 8, 4, 2, 9, 3, 5, 7, 11, 13} whose stages fit the workgroup (256 threads, or 512 with two butterflies per thread on radices <= 8)?  The largest odd radix goes first (the
// first stage has no twiddles).
static bool fft_factor(uint64_t N, FftStages &st, unsigned &threads) {
    st.n = 0;
    if (N < 2 || N > 8192) return false;
    uint64_t n = N;
    auto push = [&](int r) { if (st.n >= 14) return false; st.r[st.n++] = r; n /= r; return true; };
    const int odd[6] = {13, 11, 7, 5, 9, 3};
    for (int r : odd) while (n % r == 0) if (!push(r)) return false;
    int e = 0;
    while (((n >> e) & 1) == 0) ++e;                                     // 2^e: ceil(e/4) stages of (nearly) equal radix, e.g. 2^13 = 16 8 8 8
    if (e) {
        const int m = (e + 3) / 4, base = e / m, extra = e % m;
        for (int q = 0; q < m; ++q) if (!push(1 << (base + (q < extra ? 1 : 0)))) return false;
    }
    if (n != 1) return false;
    uint64_t small = 0, big = 0;                                         // threads the 256-thread / the 512-thread variant needs
    for (int s = 0; s < st.n; ++s) {
        const uint64_t nr = N / st.r[s], nb = st.r[s] <= 8 ? (nr + 1) / 2 : nr;
        if (nr > small) small = nr;
        if (nb > big) big = nb;
    }
    if (small <= 256) threads = (unsigned)((small + 63) / 64 * 64);
    else if (big <= 512) threads = 0x10000u | (unsigned)((big + 63) / 64 * 64);     // flag: the long-record variant
    else return false;
    return true;
}

}  // namespace qdas
