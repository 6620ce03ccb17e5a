// fft_lds.h -- the in-LDS mixed-radix Stockham transform (internal): packed-complex helpers, the small DFT networks, the padded LDS index, the stage
// factorisation, the twiddle table, and the stage drivers.  A stage of radix R loads R points, multiplies them by their twiddles and runs the
// length-R DFT (QDAS_FFT_BUTTERFLY), then scatters; fft_radix turns a run-time radix into a compile-time one.  Four users, and what each adds on top:
//   hilbert (pre.hip)          fused_stage with HilbertOps: the first stage reads two real traces from HBM, the first inverse stage applies the
//                              analytic weights, the last stage writes (x, H x) [* phasor]; plus the prebuilt stage lists (hilbert_fixed_kernel)
//   FFT convolution (pre.hip)  fused_stage with FftConvOps: zero-padded loads, times the filter's spectrum, the crop [off, off + L) on the way out
//   migration (migration.hip)  lds_fft on one trace per workgroup (passes A and C), and its own lat_stage: 16 rows out of place between two tiles
//   refocus (refocus.hip)      lds_fft with one or two thread groups per workgroup, each on a trace of its own
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

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

// points of the LDS tile of one transform of length N (lds_pad of the last point, plus one)
template <typename T> static __host__ __device__ constexpr T fft_lds_points(T N) { return N + N / 16 + 1; }

static __device__ __forceinline__ float2 conjf2(float2 a) { return make_float2(a.x, -a.y); }

// (c, s) of 2 pi * turns, the turns reduced in fp64 first
static __device__ __forceinline__ float2 phasor(double turns) {
    turns -= rint(turns);
    float s, c;
    sincospif(2.0f * (float)turns, &s, &c);
    return make_float2(c, s);
}

// exp(-2 pi i k / N), k < N: the table every transform of length N reads (`tw` below).  pre_create (pre.hip) fills hilbert's table on the host instead.
static __device__ __forceinline__ float2 fft_twiddle(uint32_t k, uint32_t N) {
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)N, &sn, &cs);
    return make_float2((float)cs, (float)sn);
}
__global__ void __launch_bounds__(256) fft_twiddles_kernel(float2 *tw, uint32_t N);           // the whole table, 256 threads per workgroup; one copy, in pre.hip

// Butterfly of radix R of a stage whose sub-transforms have length Ns so far (NR = N / R butterflies, this one at k = j % Ns), on float2 v[R]: the
// points times their twiddles exp(-2 pi i k t / (Ns R)) -- one table entry, the rest by products -- then the length-R DFT.
// A macro, not a function: behind a function boundary the optimiser splits the caller's point array differently, and with -ffp-contract=fast that
// decides which products of hilbert's last stage fuse with the subtraction that follows -- the results move in the last bit.
#define QDAS_FFT_BUTTERFLY(R, v, tw, k, NR, Ns) do { \
    if ((Ns) > 1) { \
        float2 w[R]; \
        w[1] = (tw)[(k) * ((NR) / (Ns))]; \
        _Pragma("unroll") \
        for (int t = 2; t < R; ++t) w[t] = cmulf(w[t / 2], w[t - t / 2]); \
        _Pragma("unroll") \
        for (int t = 1; t < R; ++t) (v)[t] = cmulf((v)[t], w[t]); \
    } \
    dft_small<R>(v, tw, NR); \
} while (0)

// f(std::integral_constant<int, R>) for the radix R of a stage list (fft_factor makes no others)
template <typename F> static __device__ __forceinline__ void fft_radix(const int R, F &&f) {
    switch (R) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 9: f(std::integral_constant<int, 9>{}); break;
        case 11: f(std::integral_constant<int, 11>{}); break;
        case 13: f(std::integral_constant<int, 13>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}
#define QDAS_FFT_INLINE __attribute__((always_inline))                   // on the lambdas handed to fft_radix: every call site keeps its own inlined stages

// ---- one transform of length N resident in LDS (padded index lds_pad), in place: thread j of its GROUP of `nth` threads owns butterfly j of every stage
// and keeps its R points in registers (BIG: two butterflies per thread on radices <= 8).  A workgroup is one group (FftBlock) or holds several, each
// on a trace of its own (FftGroup; `active`: the group has one); the barriers are the workgroup's, so every thread comes here the same number of
// times.  The caller has synchronised after filling `buf`; every stage ends with a barrier.
// FftBlock reads threadIdx.x and blockDim.x where they are used: handed in as values they are loop invariants that pull every radix's stage indices
// out of the stage loop, which costs mig_time<true> 26 VGPRs and makes mig_stolt<*, true> (at its 256) spill.
struct FftBlock {
    __device__ __forceinline__ uint32_t tid() const { return threadIdx.x; }
    __device__ __forceinline__ uint32_t nth() const { return blockDim.x; }
    __device__ __forceinline__ bool active() const { return true; }
};
struct FftGroup {
    uint32_t tid_, nth_; bool active_;
    __device__ __forceinline__ uint32_t tid() const { return tid_; }
    __device__ __forceinline__ uint32_t nth() const { return nth_; }
    __device__ __forceinline__ bool active() const { return active_; }
};

template <int R, bool BIG, typename G>
static __device__ __forceinline__ void lds_stage(float2 *buf, const float2 *__restrict__ tw, const uint32_t N, const uint32_t Ns, const G g) {
    constexpr int ITER = (BIG && R <= 8) ? 2 : 1;
    const uint32_t NR = N / R;
    float2 v[ITER][R];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const uint32_t j = g.tid() + it * g.nth();
        if (g.active() && j < NR) {
            const uint32_t k = j % Ns;
#pragma unroll
            for (int t = 0; t < R; ++t) v[it][t] = buf[lds_pad(j + t * NR)];
            QDAS_FFT_BUTTERFLY(R, v[it], tw, k, NR, Ns);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const uint32_t j = g.tid() + it * g.nth();
        if (g.active() && j < NR) {
            const uint32_t k = j % Ns, j0 = (j - k) * R + k;
#pragma unroll
            for (int t = 0; t < R; ++t) buf[lds_pad(j0 + t * Ns)] = v[it][t];
        }
    }
    __syncthreads();
}

template <bool BIG, typename G>
static __device__ __forceinline__ void lds_fft(float2 *buf, const float2 *__restrict__ tw, const FftStages &st, const uint32_t N, const G g) {
    uint32_t Ns = 1;
    for (int s = 0; s < st.n; ++s) {
        fft_radix(st.r[s], [&](auto r) QDAS_FFT_INLINE { lds_stage<decltype(r)::value, BIG>(buf, tw, N, Ns, g); });
        Ns *= st.r[s];
    }
}

// ---- a forward and an inverse transform of one workgroup's record, fused with the HBM traffic at both ends: thread j < N / R owns butterfly j of
// every stage, so the record lives in ONE LDS buffer (read -> barrier -> write -> barrier).  `ops` says what the ends do:
//   ING:  the stage opens the forward transform -- its points come from ops.load(idx), not from LDS (points j + t N/R: a coalesced pattern)
//   WGT:  the stage opens the inverse transform -- ops.weight(idx, v) on every loaded point (with the conjugate: ifft(X) = conj(fft(conj(X))) / N)
//   OUTG: the stage closes the inverse transform -- its results go to ops.store(i, v), not to LDS (Ns == N / R there: points j + t N/R again)
template <int R, bool ING, bool WGT, bool OUTG, bool BIG, typename Ops>
static __device__ __forceinline__ void fused_stage(float2 *buf, const float2 *tw, const uint32_t N, const uint32_t Ns, const Ops &ops) {
    constexpr int ITER = (BIG && R <= 8) ? 2 : 1;                        // butterflies per thread (the long-record variant doubles up on the light radices)
    const uint32_t NR = N / R;
    float2 v[ITER][R];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const uint32_t j = threadIdx.x + it * blockDim.x;
        if (j < NR) {
            const uint32_t k = j % Ns;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const uint32_t idx = j + t * NR;
                if constexpr (ING) v[it][t] = ops.load(idx);
                else v[it][t] = buf[lds_pad(idx)];
                if constexpr (WGT) v[it][t] = ops.weight(idx, v[it][t]);
            }
            QDAS_FFT_BUTTERFLY(R, v[it], tw, k, NR, Ns);
        }
    }
    if constexpr (!ING) __syncthreads();                                 // every butterfly has read its points
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const uint32_t j = threadIdx.x + it * blockDim.x;
        if (j < NR) {
            const uint32_t k = j % Ns, j0 = (j - k) * R + k;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                if constexpr (OUTG) ops.store(j0 + t * Ns, v[it][t]);
                else buf[lds_pad(j0 + t * Ns)] = v[it][t];
            }
        }
    }
    if constexpr (!OUTG) __syncthreads();
}

template <bool ING, bool WGT, bool OUTG, bool BIG, typename Ops>
static __device__ __forceinline__ void fused_stage_r(const int R, float2 *buf, const float2 *tw, const uint32_t N, const uint32_t Ns, const Ops &ops) {
    fft_radix(R, [&](auto r) QDAS_FFT_INLINE { fused_stage<decltype(r)::value, ING, WGT, OUTG, BIG>(buf, tw, N, Ns, ops); });
}

// the forward transform: radices r[0], ..., r[n-1]
template <bool BIG, typename Ops>
static __device__ __forceinline__ void fused_forward(float2 *buf, const float2 *tw, const FftStages &st, const uint32_t N, const Ops &ops) {
    fused_stage_r<true, false, false, BIG>(st.r[0], buf, tw, N, 1, ops);
    uint32_t Ns = st.r[0];
    for (int s = 1; s < st.n; ++s) { fused_stage_r<false, false, false, BIG>(st.r[s], buf, tw, N, Ns, ops); Ns *= st.r[s]; }
}

// the inverse transform: radices r[1], ..., r[n-1], then r[0], so that the last stage produces points j + t N/r[0] -- coalesced stores
template <bool BIG, typename Ops>
static __device__ __forceinline__ void fused_inverse(float2 *buf, const float2 *tw, const FftStages &st, const uint32_t N, const Ops &ops) {
    const int n = st.n;
    if (n == 1) { fused_stage_r<false, true, true, BIG>(st.r[0], buf, tw, N, 1, ops); return; }
    fused_stage_r<false, true, false, BIG>(st.r[1], buf, tw, N, 1, ops);
    uint32_t Ns = st.r[1];
    for (int s = 2; s < n; ++s) { fused_stage_r<false, false, false, BIG>(st.r[s], buf, tw, N, Ns, ops); Ns *= st.r[s]; }
    fused_stage_r<false, false, true, BIG>(st.r[0], buf, tw, N, Ns, ops);
}

}  // namespace qdas
