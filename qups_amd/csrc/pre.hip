// pre.hip -- the step in front of the DAS path: real RF traces -> analytic (complex) channel data, optionally downmixed.
//
// Replaces ChannelData.hilbert (reference src/ChannelData.m:935-966: fft along time to N points, weights
// w = [1; 2 x (floor(N/2)-1); 1 + mod(N,2); 0 ...], ifft) fused with ChannelData.downmix (src/ChannelData.m:757-766:
// data .* exp(-2i*pi*fc*time)), so that real (fp32 or int16) traces can be uploaded -- half / a quarter of the bytes of
// complex64 channel data over PCIe -- and turned into the beamformer's input on the device.  The FFTs are hipFFT plans
// (a library FFT, like the reference's MATLAB fft); the packing, weighting and downmix kernels are HIP.
//
// For real input, ifft(w .* fft(x)) = x + i*H(x): the real part IS the (padded / truncated) input, only the imaginary part
// needs an inverse transform, and it is real: H(x) = C2R of (-i sgn(f) X(f)) over the half spectrum.  So the pass is
// pad -> R2C -> half-spectrum weights -> C2R -> interleave (x, H(x)) [* phasor]: two half-size real transforms instead of a real
// forward + a full complex inverse one (whose length-2816 decomposition costs hipFFT two extra transposes).
//
// One-pass path (lengths N = 2^a 3^b 5^c 7^d 11^e 13^f up to 8192 whose stages fit a workgroup -- every record length of the BASELINE configurations, e.g. 2816 = 2^8 * 11):
// hilbert_lds_kernel keeps a whole trace pair in LDS.  Two real traces ride one complex transform (z = x1 + i x2; the analytic
// filter A = ifft(w .* fft(.)) is linear over C, so A z = (x1 - H x2) + i (x2 + H x1)), forward and inverse mixed-radix Stockham
// stages run in LDS, and the last stage writes (x, H x) [* phasor] -- HBM sees the real input once and the complex output once.
// Everything else (other lengths, QDAS_PRE_HIPFFT=1) takes the hipFFT passes below.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>
#include "qdas_kernels.h"
#include "fft_lds.h"
#include "api_util.h"

namespace qdas {

// ---------------------------------------------------------------------------------------------------------------- one-pass path
// Stage s has radix r[s]; thread j < N / r[s] owns butterfly j of every stage and keeps its r[s] points in registers, so the trace pair
// lives in ONE LDS buffer (read -> barrier -> write -> barrier) -- 8 N bytes per workgroup, seven workgroups per CU at N = 2816.
// The first forward stage reads the real traces from HBM straight into the butterfly (its points j + t N/r are a coalesced pattern);
// the inverse transform runs the radices in the order r[1], ..., r[n-1], r[0], so its last stage produces points j + t N/r[0] --
// again coalesced -- and writes the result to HBM from registers.

struct HilbertArgs {
    const void *x; float2 *y; const float2 *tw;
    uint32_t T, N; uint64_t K;
    FftStages st;
    double fd, t0, fs;
};

// What hilbert's transform does at its ends (fft_lds.h fused_stage): one workgroup's pair of real traces x1, x2 (two: the second exists) of T samples.
// FIXED: the ops of hilbert_fixed_kernel (see the downmix in store)
template <typename TI, bool FIXED>
struct HilbertOps {
    const TI *x1, *x2; float2 *y1, *y2;
    bool two; uint32_t T, N;
    double fd, t0, fs;
    __device__ __forceinline__ HilbertOps(const HilbertArgs &A, uint32_t N_, uint64_t k1, bool two_)
        : x1((const TI *)A.x + (uint64_t)A.T * k1), x2(x1 + A.T), y1(A.y + (uint64_t)N_ * k1), y2(y1 + N_), two(two_), T(A.T), N(N_), fd(A.fd), t0(A.t0), fs(A.fs) {}
    // z = x1 + i x2, zero beyond T
    __device__ __forceinline__ float2 load(uint32_t idx) const { return make_float2(idx < T ? (float)x1[idx] : 0.f, (two && idx < T) ? (float)x2[idx] : 0.f); }
    // w = [1; 2 ...; 1 + mod(N,2); 0 ...]  (src/ChannelData.m:961-963), conjugated
    __device__ __forceinline__ float2 weight(uint32_t idx, float2 v) const {
        const uint32_t h = N / 2;
        const float g = idx == 0 ? 1.f : idx < h ? 2.f : idx == h ? (float)(1 + (N & 1)) : 0.f;
        return make_float2(v.x * g, -v.y * g);
    }
    // conj(z) / N = (x1 - H x2) + i (x2 + H x1): the finished (x, H x) [* phasor] of both traces
    __device__ __forceinline__ void store(uint32_t i, float2 z) const {
        const float sc = 1.0f / (float)N;
        const float r1 = i < T ? (float)x1[i] : 0.f, r2 = (two && i < T) ? (float)x2[i] : 0.f;
        float2 v1 = make_float2(r1, -z.y * sc - r2), v2 = make_float2(r2, r1 - z.x * sc);
        if (fd != 0.0) {
            const double cyc = fd * (t0 + (double)i / fs);             // cycles; reduced in fp64 before the fp32 sincos
            const float ph = (float)(cyc - floor(cyc));
            const float c = __builtin_amdgcn_cosf(ph), sn = -__builtin_amdgcn_sinf(ph);
            // The rotation with its fused multiply-adds spelled out.  Left to -ffp-contract, which product of a pair is rounded on its own follows the
            // code around this one, and it came out differently in one place: the second trace's real part rounds x c in the prebuilt lists' kernels
            // and y sn in the run-time kernel.  Both are kept as they were, to the bit.
            v1 = make_float2(__builtin_fmaf(v1.x, c, -(v1.y * sn)), __builtin_fmaf(v1.y, c, v1.x * sn));
            v2 = make_float2(FIXED ? __builtin_fmaf(-v2.y, sn, v2.x * c) : __builtin_fmaf(v2.x, c, -(v2.y * sn)), __builtin_fmaf(v2.y, c, v2.x * sn));
        }
        y1[i] = v1;
        if (two) y2[i] = v2;
    }
};

// BIG: up to 512 threads, two butterflies per thread on radices <= 8 (records up to 8192 samples); otherwise up to 256 threads
template <typename TI, bool BIG>
__global__ void __launch_bounds__(BIG ? 512 : 256) hilbert_lds_kernel(const HilbertArgs A) {
    extern __shared__ float2 pre_lds[];
    const uint64_t k1 = 2ull * blockIdx.x;
    const HilbertOps<TI, false> ops(A, A.N, k1, k1 + 1 < A.K);
    fused_forward<BIG>(pre_lds, A.tw, A.st, A.N, ops);
    fused_inverse<BIG>(pre_lds, A.tw, A.st, A.N, ops);
}

// The same transform with the stage list (hence N, every stride and every twiddle step) known at compile time: the lists of the usual record
// lengths are prebuilt (FIXED_LISTS); other lengths take the run-time kernel above, whose register budget is the worst radix's.
template <typename TI, bool BIG, int R0, int R1, int R2, int R3>
__global__ void __launch_bounds__(BIG ? 512 : 256) hilbert_fixed_kernel(const HilbertArgs A) {
    extern __shared__ float2 pre_lds[];
    constexpr uint32_t N = (uint32_t)R0 * R1 * R2 * R3;
    const uint64_t k1 = 2ull * blockIdx.x;
    const HilbertOps<TI, true> ops(A, N, k1, k1 + 1 < A.K);
    fused_stage<R0, true, false, false, BIG>(pre_lds, A.tw, N, 1, ops);
    fused_stage<R1, false, false, false, BIG>(pre_lds, A.tw, N, R0, ops);
    if constexpr (R2 > 1) fused_stage<R2, false, false, false, BIG>(pre_lds, A.tw, N, R0 * R1, ops);
    if constexpr (R3 > 1) fused_stage<R3, false, false, false, BIG>(pre_lds, A.tw, N, R0 * R1 * R2, ops);
    fused_stage<R1, false, true, false, BIG>(pre_lds, A.tw, N, 1, ops);
    if constexpr (R2 > 1) fused_stage<R2, false, false, false, BIG>(pre_lds, A.tw, N, R1, ops);
    if constexpr (R3 > 1) fused_stage<R3, false, false, false, BIG>(pre_lds, A.tw, N, R1 * R2, ops);
    fused_stage<R0, false, false, true, BIG>(pre_lds, A.tw, N, R1 * R2 * R3, ops);
}

typedef void (*HilbertFn)(const HilbertArgs);
struct FixedList { int r[4]; bool big; HilbertFn f32, i16; };
#define QFIX(BIG, A, B, C, D) {{A, B, C, D}, BIG, hilbert_fixed_kernel<float, BIG, A, B, C, D>, hilbert_fixed_kernel<int16_t, BIG, A, B, C, D>}
static const FixedList FIXED_LISTS[] = {
    QFIX(false, 16, 16, 1, 1),    //  256
    QFIX(false, 8, 8, 8, 1),      //  512
    QFIX(false, 16, 8, 8, 1),     // 1024
    QFIX(false, 3, 8, 8, 8),      // 1536
    QFIX(false, 16, 16, 8, 1),    // 2048  (C1, C2, C5)
    QFIX(false, 5, 8, 8, 8),      // 2560
    QFIX(false, 11, 16, 16, 1),   // 2816  (C3)
    QFIX(true, 3, 16, 8, 8),      // 3072
    QFIX(false, 13, 16, 16, 1),   // 3328
    QFIX(true, 7, 8, 8, 8),       // 3584
    QFIX(false, 16, 16, 16, 1),   // 4096
    QFIX(true, 16, 8, 8, 8),      // 8192
};
#undef QFIX

static const FixedList *fixed_list(const FftStages &st, bool big) {
    for (const FixedList &f : FIXED_LISTS) {
        if (f.big != big) continue;
        bool same = true;
        for (int q = 0; q < 4; ++q) same = same && (q < st.n ? st.r[q] : 1) == f.r[q];
        if (same && st.n <= 4 && st.n >= 2) return &f;
    }
    return nullptr;
}


// real traces (T x K, fp32 or int16) -> zero-padded / truncated fp32 (N x K)
template <typename TI>
__global__ void __launch_bounds__(256) pre_pad_kernel(const TI *x, float *xr, uint64_t T, uint64_t N, uint64_t K) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * K) return;
    const uint64_t t = i % N, k = i / N;
    xr[i] = t < T ? (float)x[t + T * k] : 0.f;
}

// half spectrum X (N/2+1 bins per trace) -> spectrum of the Hilbert transform, scaled by the 1/N of the inverse transform:
// -i*sgn(f)*X(f)/N for 0 < f < N/2, 0 at DC and (even N) at Nyquist -- the imaginary part of what the reference's weights
// [1; 2...; 1 + mod(N,2); 0...] produce (src/ChannelData.m:961-963)
__global__ void __launch_bounds__(256) pre_spectrum_kernel(float2 *half, uint64_t N, uint64_t K, float scale) {
    const uint64_t H = N / 2 + 1;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= H * K) return;
    const uint64_t f = i % H;
    const bool zero = (f == 0) || ((N & 1) == 0 && f == N / 2);
    const float2 v = half[i];
    half[i] = zero ? make_float2(0.f, 0.f) : make_float2(v.y * scale, -v.x * scale);
}

// y = (x, H(x)) times the downmix phasor exp(-2j pi fd (t0 + t/fs)) (fd == 0: none)
__global__ void __launch_bounds__(256) pre_finish_kernel(const float *xr, const float *hr, float2 *y, uint64_t N, uint64_t K, double fd, double t0, double fs) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * K) return;
    float2 v = make_float2(xr[i], hr[i]);
    if (fd != 0.0) {
        const double cyc = fd * (t0 + (double)(i % N) / fs);           // cycles; reduced in fp64 before the fp32 sincos
        const float ph = (float)(cyc - floor(cyc));
        const float c = __builtin_amdgcn_cosf(ph), s = -__builtin_amdgcn_sinf(ph);
        v = make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
    }
    y[i] = v;
}

struct PrePlan {
    uint64_t T, K, N;
    int in_type;          // 0: fp32, 1: int16
    double fs, t0, fd;
    hipfftHandle r2c = 0, c2r = 0;
    float *xr = nullptr;  // N x K real (padded input)
    float *hr = nullptr;  // N x K real (its Hilbert transform)
    float2 *half = nullptr;
    bool have = false;
    bool lds = false;     // one-pass path
    FftStages st{};
    unsigned threads = 0;
    float2 *tw = nullptr; // exp(-2 pi i k / N), k < N
};

int pre_create(PrePlan **out, uint64_t T, uint64_t K, uint64_t N, int in_type, double fs, double t0, double fd) {
    PrePlan *p = new PrePlan();
    p->T = T; p->K = K; p->N = N ? N : T; p->in_type = in_type; p->fs = fs; p->t0 = t0; p->fd = fd;
    if (p->N == 0 || K == 0) { *out = p; return 0; }
    const char *force = getenv("QDAS_PRE_HIPFFT");
    if (!(force && force[0] == '1') && p->N <= 0xffffffffull && T <= 0xffffffffull && fft_factor(p->N, p->st, p->threads)) {
        std::vector<float2> h(p->N);                                     // the host's cos / sin: rounded differently from fft_twiddle's sincospi here and there, and
                                                                         // hilbert's results carry this table's bits -- it stays
        for (uint64_t k = 0; k < p->N; ++k) {
            const double a = -2.0 * M_PI * (double)k / (double)p->N;
            h[k] = make_float2((float)cos(a), (float)sin(a));
        }
        const size_t lds_bytes = sizeof(float2) * fft_lds_points(p->N);
        bool ok = hipMalloc(&p->tw, sizeof(float2) * p->N) == hipSuccess &&
                  qdas_internal_upload(p->tw, h.data(), sizeof(float2) * p->N) == (int)hipSuccess;
        if (ok && lds_bytes > 65536) {
            const void *fns[4] = {(const void *)hilbert_lds_kernel<float, false>, (const void *)hilbert_lds_kernel<float, true>,
                                  (const void *)hilbert_lds_kernel<int16_t, false>, (const void *)hilbert_lds_kernel<int16_t, true>};
            for (const void *fn : fns) ok = ok && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
            for (const FixedList &fl : FIXED_LISTS) ok = ok && hipFuncSetAttribute((const void *)fl.f32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess
                                                         && hipFuncSetAttribute((const void *)fl.i16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
        }
        if (ok) { p->lds = p->have = true; *out = p; return 0; }
        if (p->tw) { (void)hipFree(p->tw); p->tw = nullptr; }
        (void)hipGetLastError();
    }
    int n[1] = {(int)p->N};
    if (hipfftPlanMany(&p->r2c, 1, n, nullptr, 1, (int)p->N, nullptr, 1, (int)(p->N / 2 + 1), HIPFFT_R2C, (int)K) != HIPFFT_SUCCESS) { delete p; return 1; }
    if (hipfftPlanMany(&p->c2r, 1, n, nullptr, 1, (int)(p->N / 2 + 1), nullptr, 1, (int)p->N, HIPFFT_C2R, (int)K) != HIPFFT_SUCCESS) { hipfftDestroy(p->r2c); delete p; return 1; }
    if (hipMalloc(&p->xr, sizeof(float) * p->N * K) != hipSuccess || hipMalloc(&p->hr, sizeof(float) * p->N * K) != hipSuccess ||
        hipMalloc(&p->half, sizeof(float2) * (p->N / 2 + 1) * K) != hipSuccess) {
        hipfftDestroy(p->r2c); hipfftDestroy(p->c2r); if (p->xr) (void)hipFree(p->xr); if (p->hr) (void)hipFree(p->hr); delete p; return 2;
    }
    p->have = true;
    *out = p;
    return 0;
}

void pre_destroy(PrePlan *p) {
    if (!p) return;
    if (p->lds) { (void)hipFree(p->tw); delete p; return; }
    if (p->have) { hipfftDestroy(p->r2c); hipfftDestroy(p->c2r); (void)hipFree(p->xr); (void)hipFree(p->hr); (void)hipFree(p->half); }
    delete p;
}

bool pre_one_pass(const PrePlan *p) { return p && p->lds; }

int pre_execute(PrePlan *p, const void *x, void *y, hipStream_t s) {
    if (!p->have) return 0;
    if (p->lds) {
        HilbertArgs A{x, (float2 *)y, p->tw, (uint32_t)p->T, (uint32_t)p->N, p->K, p->st, p->fd, p->t0, p->fs};
        const unsigned nb = (unsigned)((p->K + 1) / 2);
        const size_t lds_bytes = sizeof(float2) * fft_lds_points(p->N);
        const unsigned th = p->threads & 0xffffu;
        const bool big = (p->threads >> 16) != 0;
        if (const FixedList *f = fixed_list(p->st, big)) {
            (p->in_type == 1 ? f->i16 : f->f32)<<<nb, th, lds_bytes, s>>>(A);
            return hipGetLastError() == hipSuccess ? 0 : 3;
        }
        if (p->in_type == 1) { if (big) hilbert_lds_kernel<int16_t, true><<<nb, th, lds_bytes, s>>>(A); else hilbert_lds_kernel<int16_t, false><<<nb, th, lds_bytes, s>>>(A); }
        else { if (big) hilbert_lds_kernel<float, true><<<nb, th, lds_bytes, s>>>(A); else hilbert_lds_kernel<float, false><<<nb, th, lds_bytes, s>>>(A); }
        return hipGetLastError() == hipSuccess ? 0 : 3;
    }
    const uint64_t NK = p->N * p->K;
    const unsigned g = (unsigned)((NK + 255) / 256);
    if (p->in_type == 1) pre_pad_kernel<int16_t><<<g, 256, 0, s>>>((const int16_t *)x, p->xr, p->T, p->N, p->K);
    else pre_pad_kernel<float><<<g, 256, 0, s>>>((const float *)x, p->xr, p->T, p->N, p->K);
    if (hipfftSetStream(p->r2c, s) != HIPFFT_SUCCESS || hipfftSetStream(p->c2r, s) != HIPFFT_SUCCESS) return 1;
    if (hipfftExecR2C(p->r2c, p->xr, (hipfftComplex *)p->half) != HIPFFT_SUCCESS) return 1;
    const uint64_t HK = (p->N / 2 + 1) * p->K;
    pre_spectrum_kernel<<<(unsigned)((HK + 255) / 256), 256, 0, s>>>(p->half, p->N, p->K, 1.0f / (float)p->N);
    if (hipfftExecC2R(p->c2r, (hipfftComplex *)p->half, p->hr) != HIPFFT_SUCCESS) return 1;
    pre_finish_kernel<<<g, 256, 0, s>>>(p->xr, p->hr, (float2 *)y, p->N, p->K, p->fd, p->t0, p->fs);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}


// ---------------------------------------------------------------------------------------------------------------- FFT convolution (convd, long filters)
// convd of complex64 traces with ONE filter (ChannelData.filter's band-pass: reference kern/convd.m + src/convd.cu:95-146 form every product, M x N per
// trace) through the same LDS-resident transform: a trace is read once, zero-padded to a length Nf >= M + N - 1 that the stage list above takes,
// transformed, multiplied by the filter's spectrum, transformed back (ifft(Z) = conj(fft(conj(Z))) / Nf) and the outputs [off, off + L) of the linear
// convolution are written -- O(Nf log Nf) per trace instead of M x N products: from about a hundred taps on the direct kernel (conv.hip, bound by
// packed-FMA issue) is the slower one.  One trace per workgroup.  The spectrum H (times 1 / Nf) and the twiddle table are made on the stream by two
// tiny kernels in double precision; nothing is synchronised.  Rounding: a few 1e-7 of the largest output, like the direct sum of fp32 products.
struct FftConvArgs {
    const float2 *x; float2 *z; const float2 *H; const float2 *tw;
    uint32_t M, N, off, L; uint64_t K;
    FftStages st;
};

// exp(-2 pi i k / N), k < N (declared in fft_lds.h: migration.hip and refocus.hip launch it)
__global__ void __launch_bounds__(256) fft_twiddles_kernel(float2 *tw, uint32_t N) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    tw[k] = fft_twiddle(k, N);
}

__global__ void __launch_bounds__(256) fftconv_tables_kernel(const void *taps, int taps_real, uint32_t ntaps, uint32_t N, float2 *H, float2 *tw) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    tw[k] = fft_twiddle(k, N);
    double re = 0.0, im = 0.0;
    for (uint32_t n = 0; n < ntaps; ++n) {
        const double yr = taps_real ? (double)((const float *)taps)[n] : (double)((const float2 *)taps)[n].x;
        const double yi = taps_real ? 0.0 : (double)((const float2 *)taps)[n].y;
        double sn, cs;
        sincospi(-2.0 * (double)(((uint64_t)k * n) % N) / (double)N, &sn, &cs);
        re += yr * cs - yi * sn; im += yr * sn + yi * cs;
    }
    H[k] = make_float2((float)(re / (double)N), (float)(im / (double)N));
}

// What the convolution's transform does at its ends (fft_lds.h fused_stage): one workgroup's trace x of M points, its outputs z[0, L)
struct FftConvOps {
    const float2 *x, *H; float2 *z;
    uint32_t M, off, L;
    __device__ __forceinline__ FftConvOps(const FftConvArgs &A, uint64_t k1) : x(A.x + (uint64_t)A.M * k1), H(A.H), z(A.z + (uint64_t)A.L * k1), M(A.M), off(A.off), L(A.L) {}
    // the trace, zero beyond M
    __device__ __forceinline__ float2 load(uint32_t idx) const { return idx < M ? x[idx] : make_float2(0.f, 0.f); }
    // times the filter's spectrum, conjugated
    __device__ __forceinline__ float2 weight(uint32_t idx, float2 v) const { const float2 p = cmulf(v, H[idx]); return make_float2(p.x, -p.y); }
    // conjugate back, outputs [off, off + L) of the linear convolution
    __device__ __forceinline__ void store(uint32_t i, float2 v) const { if (i >= off && i - off < L) z[i - off] = make_float2(v.x, -v.y); }
};

template <bool BIG>
__global__ void __launch_bounds__(BIG ? 512 : 256) fftconv_lds_kernel(const FftConvArgs A) {
    extern __shared__ float2 pre_lds[];
    const FftConvOps ops(A, blockIdx.x);
    fused_forward<BIG>(pre_lds, A.tw, A.st, A.N, ops);
    fused_inverse<BIG>(pre_lds, A.tw, A.st, A.N, ops);
}

// 0: done (asynchronously on `s`), 1: not this path (no transform length up to 8192 takes M + ntaps - 1 points), 2: HIP error
int fftconv_launch(const void *x, const void *taps, int taps_real, void *z, uint64_t M, uint64_t ntaps, uint64_t K, uint64_t off, uint64_t L, hipStream_t s) {
    const uint64_t need = M + ntaps - 1;
    if (need > 8192 || K == 0 || K >= (1ull << 31)) return 1;
    FftStages st{};
    unsigned threads = 0;
    uint64_t N = 0;
    // the transform length: among the lengths up to a quarter beyond M + ntaps - 1 that the stage list takes, the one with the least points x stages
    // (every stage is a pass over the trace in LDS between two barriers: 2944 points needed -> 3328 = 13 x 16 x 16 beats 2970 = 11 x 5 x 9 x 3 x 2)
    double best = 0.0;
    for (uint64_t n = need; n <= 8192 && n <= need + need / 4 + 64; ++n) {
        FftStages c{};
        unsigned th = 0;
        if (!fft_factor(n, c, th)) continue;
        const double cost = (double)n * ((double)c.n + ((th >> 16) ? 0.5 : 0.0));
        if (!N || cost < best) { N = n; st = c; threads = th; best = cost; }
    }
    if (!N) return 1;
    const bool big = (threads >> 16) != 0;
    const unsigned th = threads & 0xffffu;
    const size_t lds_bytes = sizeof(float2) * fft_lds_points(N);
    if (lds_bytes > 65536) {
        const void *fn = big ? (const void *)fftconv_lds_kernel<true> : (const void *)fftconv_lds_kernel<false>;
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 1; }
    }
    Scratch scratch(s);
    float2 *tab = (float2 *)scratch.get(sizeof(float2) * 2 * N);         // [H | tw]
    if (!tab) return 1;
    fftconv_tables_kernel<<<(unsigned)((N + 255) / 256), 256, 0, s>>>(taps, taps_real, (uint32_t)ntaps, (uint32_t)N, tab, tab + N);
    FftConvArgs A{(const float2 *)x, (float2 *)z, tab, tab + N, (uint32_t)M, (uint32_t)N, (uint32_t)off, (uint32_t)L, K, st};
    if (big) fftconv_lds_kernel<true><<<(unsigned)K, th, lds_bytes, s>>>(A); else fftconv_lds_kernel<false><<<(unsigned)K, th, lds_bytes, s>>>(A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : 2;
}

}  // namespace qdas

using namespace qdas;

struct qdas_pre_plan { qdas::PrePlan *p; int device; };

extern "C" int qdas_pre_plan_create(qdas_pre_plan **out, const qdas_pre_desc *d) {
    if (!out || !d) return fail(QDAS_EINVAL, "null argument");
    *out = nullptr;
    if (d->in_type != QDAS_PRE_F32 && d->in_type != QDAS_PRE_I16) return fail(QDAS_EINVAL, "pre: input type must be fp32 or int16");
    const uint64_t N = d->Nfft ? d->Nfft : d->T;
    if (N >= (1ull << 31) || d->K >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "pre: transform length / trace count too large");
    if (d->fdown != 0.0 && !(d->fs > 0)) return fail(QDAS_EINVAL, "Undefined sampling rate.");
    DeviceGuard guard(d->device);
    HIPCHK(guard.err);
    qdas_pre_plan *pl = new qdas_pre_plan();
    { hipError_t e = hipGetDevice(&pl->device); if (e != hipSuccess) { delete pl; return fail(QDAS_EHIP, "hipGetDevice: %s", hipGetErrorString(e)); } }
    const int rc = qdas::pre_create(&pl->p, d->T, d->K, d->Nfft, d->in_type, d->fs, d->t0, d->fdown);
    if (rc) { delete pl; return fail(rc == 2 ? QDAS_ENOMEM : QDAS_EHIP, "pre: hipFFT plan / workspace creation failed"); }
    *out = pl;
    return QDAS_OK;
}

extern "C" int qdas_pre_execute(qdas_pre_plan *pl, const void *x, void *y, void *stream) {
    if (!pl || !y) return fail(QDAS_EINVAL, "null argument");
    DeviceGuard guard(pl->device);
    HIPCHK(guard.err);
    const int rc = qdas::pre_execute(pl->p, x, y, (hipStream_t)stream);
    if (rc) return fail(QDAS_EHIP, "pre: hipFFT execution failed (%d)", rc);
    return QDAS_OK;
}

extern "C" int qdas_pre_plan_one_pass(const qdas_pre_plan *pl) { return pl && qdas::pre_one_pass(pl->p) ? 1 : 0; }

extern "C" void qdas_pre_plan_destroy(qdas_pre_plan *pl) {
    if (!pl) return;
    DeviceGuard guard(pl->device);
    qdas::pre_destroy(pl->p);
    delete pl;
}
