// migration.hip -- plane-wave Stolt f-k migration: qdas_migration (include/qdas.h has the formulas; reference src/UltrasoundSystem.m:4675-4887).
//
// The reference runs, per block of transmits, fft / fftshift / phase / fft / fftshift / wsinterpd / phase / ifftshift / ifft / phase / ifftshift / ifft
// as twelve array operations, each a pass over the F x K x M block.  Here the block is written and read three times, in four kernels (complex64):
//
//   A  mig_time     one workgroup per trace (n, m): load (zero-pad / truncate to F), remodulate, forward FFT in LDS, times exp(-2 pi i f (t0 + tau[n, m])),
//                   store at the SHIFTED frequency index into W[f + F (n + K m)].  Columns n >= N are never written: pass B reads them as zero.
//   B  mig_lateral  one workgroup per 16 consecutive f x all K lateral points of one transmit: 128-byte runs along f in HBM, 16 transforms of length K
//                   along the strided dimension in LDS (out of place between two tiles: a thread owns several butterflies), in place in W.
//   C  mig_stolt    one workgroup per kx column and slice of the block's transmits.  Per transmit: the F-point spectrum is staged in LDS, every output
//                   frequency gathers its taps at kkz (the weights and the support rule of wsinterpd: all taps in [0, F) and kkz >= 0, else 0), times the
//                   Jacobian and exp(+2 pi i f t0), inverse FFT in a second LDS tile, times exp(2 pi i kx gamma_m z), and the first min(T, F) depth
//                   samples are ACCUMULATED IN REGISTERS over the slice's transmits (keep_tx: written per transmit).  The Stolt index, the Jacobian
//                   and the phases are recomputed per transmit in fp64 (a square root and a few products per 16 bytes staged: far below the LDS work).
//   D  mig_lateral  (inverse) sums the slices' partial images while it loads, inverse transform along kx, crops to min(N, K), writes b (time fastest).
//
// Step 8 of the reference (the lateral inverse transform) is linear and transmit-independent, so the sum over transmits sits in front of it: D runs once
// per frame, not once per transmit.  Transmits are taken in blocks whose W fits QDAS_MIGRATION_BLOCK_BYTES (default 64 MiB: a block stays in the
// last-level cache between A, B and C); a slice's partial image carries over the blocks (read-modify-write by the one workgroup that owns it).  No atomics.
//
// The Stolt index is evaluated as  j0 = j - floor(F/2),  a = kx cs F / fs,  kkz = sign(j0) sqrt(a^2 + j0^2) + floor(F/2)  in fp64 -- algebraically the
// reference's (fkz - f(1)) F / fs, but exact on the kx = 0 column and the f = 0 row -- and split into an integer part and an fp32 fraction.
// Phases are formed in fp64 turns, reduced to [-1/2, 1/2], then sincospif in fp32 (f (t0 + tau) reaches hundreds of turns).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

#include "../../include/qdas.h"
#include "api_util.h"
#include "qdas_kernels.h"
#include "qdas_device.h"
#include "fft_lds.h"

namespace qdas {
namespace mig {

constexpr int TF = 16;              // consecutive frequencies per workgroup of the lateral passes: 128-byte runs
constexpr int QMAX = 16;            // points per thread of a time-axis transform: F / threads <= the largest radix
constexpr uint32_t LAT_LDS_MAX = 160u * 1024u;

struct Args {
    const float2 *x; float2 *W, *P, *b;
    const float2 *twF, *twK;
    const double *tau, *gamma;
    uint32_t T, N, M, F, K, Fk, Nn;         // Fk = min(T, F), Nn = min(N, K)
    uint32_t m0, mb, mper, nslice, RS;      // transmit block, transmits per slice of pass C, slices pass D sums, LDS row stride of the lateral tiles
    uint64_t frame, slice_stride;
    FftStages stF, stK;
    double fs, fmod, t0, c0, pitch;
    int32_t keep_tx, jacobian, accumulate;
};

// ---- pass A
template <bool BIG>
__global__ void __launch_bounds__(BIG ? 512 : 256) mig_time(const Args a) {
    extern __shared__ float2 mig_lds[];
    const uint32_t n = blockIdx.x, ml = blockIdx.y, m = a.m0 + ml, F = a.F;
    const float2 *x = a.x + (uint64_t)a.T * (n + (uint64_t)a.N * (m + (uint64_t)a.M * a.frame));
    for (uint32_t i = threadIdx.x; i < F; i += blockDim.x) {
        float2 v = make_float2(0.f, 0.f);
        if (i < a.Fk) {
            v = x[i];
            if (a.fmod != 0.0) v = cmulf(v, phasor(a.fmod * (a.t0 + (double)i / a.fs)));
        }
        mig_lds[lds_pad(i)] = v;
    }
    __syncthreads();
    lds_fft<BIG>(mig_lds, a.twF, a.stF, F, FftBlock{});
    const double td = a.t0 + a.tau[n + (uint64_t)a.N * m];
    const uint32_t hF = F / 2;
    float2 *W = a.W + (uint64_t)F * (n + (uint64_t)a.K * ml);
    for (uint32_t u = threadIdx.x; u < F; u += blockDim.x) {
        uint32_t j = u + hF;                                             // fftshift: bin u lands on (u + floor(F/2)) mod F
        if (j >= F) j -= F;
        const double f = (double)((int)j - (int)hF) / (double)F * a.fs;
        W[j] = cmulf(mig_lds[lds_pad(u)], phasor(-(f * td)));
    }
}

// ---- passes B and D: TF transforms of length K along the strided dimension, out of place between two LDS tiles (row stride RS, odd)
template <int R>
__device__ __forceinline__ void lat_stage(const float2 *in, float2 *out, const float2 *__restrict__ tw, const uint32_t K, const uint32_t Ns, const uint32_t RS) {
    const uint32_t NR = K / R, total = TF * NR;
    for (uint32_t b = threadIdx.x; b < total; b += blockDim.x) {
        const uint32_t row = b % TF, j = b / TF, k = j % Ns;
        const float2 *ri = in + row * RS;
        float2 v[R];
#pragma unroll
        for (int t = 0; t < R; ++t) v[t] = ri[lds_pad(j + t * NR)];
        QDAS_FFT_BUTTERFLY(R, v, tw, k, NR, Ns);
        float2 *ro = out + row * RS;
        const uint32_t j0 = (j - k) * R + k;
#pragma unroll
        for (int t = 0; t < R; ++t) ro[lds_pad(j0 + t * Ns)] = v[t];
    }
    __syncthreads();
}

// INV = false (pass B): W[f, n, m] (n < Nn, zero beyond) -> fftshift_k FFT_n, in place.
// INV = true  (pass D): sum of the slices of P[f, k, img] -> IFFT over ifftshift_k, cropped to n < Nn, to b[f, n, img]
template <bool INV>
__global__ void __launch_bounds__(256) mig_lateral(const Args a) {
    extern __shared__ float2 mig_lds[];
    const uint32_t K = a.K, RS = a.RS, hK = K / 2, Fx = INV ? a.Fk : a.F, f0 = blockIdx.x * TF, img = blockIdx.y;
    float2 *A = mig_lds, *B = mig_lds + TF * RS;
    const float2 *src = (INV ? a.P : a.W) + (uint64_t)Fx * K * img;
    for (uint32_t idx = threadIdx.x; idx < TF * K; idx += blockDim.x) {
        const uint32_t fl = idx % TF, q = idx / TF, f = f0 + fl;
        float2 v = make_float2(0.f, 0.f);
        uint32_t u = q;
        if (INV) {                                                       // q is the shifted index: ifftshift puts it at (q - floor(K/2)) mod K
            u = q >= hK ? q - hK : q + K - hK;
            if (f < Fx) {
                for (uint32_t s = 0; s < a.nslice; ++s) v = caddf(v, src[a.slice_stride * s + f + (uint64_t)Fx * q]);
                v = conjf2(v);
            }
        } else if (q < a.Nn && f < Fx) v = src[f + (uint64_t)Fx * q];
        A[fl * RS + lds_pad(u)] = v;
    }
    __syncthreads();
    uint32_t Ns = 1;
    for (int s = 0; s < a.stK.n; ++s) {
        fft_radix(a.stK.r[s], [&](auto r) QDAS_FFT_INLINE { lat_stage<decltype(r)::value>(A, B, a.twK, K, Ns, RS); });
        Ns *= a.stK.r[s];
        float2 *t = A; A = B; B = t;
    }
    if (INV) {
        const float sc = 1.0f / (float)K;
        float2 *dst = a.b + (uint64_t)Fx * a.Nn * img;
        for (uint32_t idx = threadIdx.x; idx < TF * a.Nn; idx += blockDim.x) {
            const uint32_t fl = idx % TF, n = idx / TF, f = f0 + fl;
            if (f < Fx) { const float2 v = A[fl * RS + lds_pad(n)]; dst[f + (uint64_t)Fx * n] = make_float2(v.x * sc, -v.y * sc); }
        }
    } else {
        float2 *dst = a.W + (uint64_t)Fx * K * img;
        for (uint32_t idx = threadIdx.x; idx < TF * K; idx += blockDim.x) {
            const uint32_t fl = idx % TF, u = idx / TF, f = f0 + fl;
            uint32_t k = u + hK;
            if (k >= K) k -= K;
            if (f < Fx) dst[f + (uint64_t)Fx * k] = A[fl * RS + lds_pad(u)];
        }
    }
}

// ---- pass C
// the spectrum column `sp` (shifted index, padded) sampled at the Stolt index of shifted output frequency j
template <int INTERP>
__device__ __forceinline__ float2 stolt_gather(const float2 *sp, const uint32_t F, const int j0, const double aa) {
    const double r = sqrt(aa * aa + (double)j0 * (double)j0);
    const double kkz = (j0 > 0 ? r : (j0 < 0 ? -r : 0.0)) + (double)(F / 2);
    float2 out = make_float2(0.f, 0.f);
    if (!(kkz >= 0.0)) return out;
    if constexpr (INTERP == 0) {
        const double rr = floor(kkz + 0.5);
        if (rr < (double)F) out = sp[lds_pad((uint32_t)rr)];
    } else {
        constexpr int NT = interp_taps(INTERP), OFF = (NT == 2) ? 0 : -1;
        const double fl = floor(kkz);
        if (!(fl + (double)(NT - 1 + OFF) < (double)F) || fl + (double)OFF < 0.0) return out;
        const uint32_t first = (uint32_t)((int)fl + OFF);
        float w[4];
        interp_weights<INTERP>((float)(kkz - fl), w);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float2 v = sp[lds_pad(first + k)];
            out.x += w[k] * v.x; out.y += w[k] * v.y;
        }
    }
    return out;
}

template <int INTERP, bool BIG>
__global__ void __launch_bounds__(BIG ? 512 : 256) mig_stolt(const Args a) {
    extern __shared__ float2 mig_lds[];
    const uint32_t k = blockIdx.x, slice = blockIdx.y, F = a.F, hF = F / 2, nth = blockDim.x, tid = threadIdx.x;
    const double kx = (double)((int)k - (int)(a.K / 2)) / (double)a.K / a.pitch;
    const double cs = a.c0 / sqrt(2.0);
    const double aa = kx * cs * (double)F / a.fs;
    float2 *ybuf = mig_lds + fft_lds_points(F);                             // second tile: the resampled spectrum, then its inverse transform
    float2 acc[QMAX];
#pragma unroll
    for (int q = 0; q < QMAX; ++q) acc[q] = make_float2(0.f, 0.f);
    const uint32_t ml0 = slice * a.mper, ml1 = min(a.mb, ml0 + a.mper);
    for (uint32_t ml = ml0; ml < ml1; ++ml) {
        const float2 *Wc = a.W + (uint64_t)F * (k + (uint64_t)a.K * ml);
        for (uint32_t i = tid; i < F; i += nth) mig_lds[lds_pad(i)] = Wc[i];
        __syncthreads();
        for (uint32_t j = tid; j < F; j += nth) {                        // gather from the spectrum tile into the transform's tile, at the ifftshift'ed place
            const int j0 = (int)j - (int)hF;
            float2 v = stolt_gather<INTERP>(mig_lds, F, j0, aa);
            const double f = (double)j0 / (double)F * a.fs;
            if (a.jacobian) {                                            // (y kz) / (fkz + eps), kz = f / cs
                const double rt = cs * sqrt(kx * kx + f * f / (cs * cs));
                const double fkz = f > 0.0 ? rt : (f < 0.0 ? -rt : 0.0);
                const float jac = (float)((f / cs) / (fkz + 2.220446049250313e-16));
                v.x *= jac; v.y *= jac;
            }
            ybuf[lds_pad(j >= hF ? j - hF : j + F - hF)] = conjf2(cmulf(v, phasor(f * a.t0)));     // conjugate: ifft(Y) = conj(fft(conj(Y))) / F
        }
        __syncthreads();
        lds_fft<BIG>(ybuf, a.twF, a.stF, F, FftBlock{});
        const double gz = kx * a.gamma[a.m0 + ml] * (a.c0 / 2.0), gz0 = gz * a.t0, gdz = gz / a.fs;     // turns of step 7 at depth sample i: gz0 + i gdz
        const float sc = 1.0f / (float)F;
        float2 *Y = a.P + (uint64_t)a.Fk * (k + (uint64_t)a.K * ml);
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            const uint32_t i = tid + q * nth;
            if (i < a.Fk) {
                const float2 t = ybuf[lds_pad(i)];
                const float2 v = cmulf(make_float2(t.x * sc, -t.y * sc), phasor(gz0 + (double)i * gdz));
                if (a.keep_tx) Y[i] = v; else acc[q] = caddf(acc[q], v);
            }
            __builtin_amdgcn_sched_barrier(0);                           // one point at a time: interleaving the sixteen phase evaluations costs their registers
        }
    }
    if (!a.keep_tx) {
        float2 *P = a.P + a.slice_stride * slice + (uint64_t)a.Fk * k;
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            const uint32_t i = tid + q * nth;
            if (i < a.Fk) P[i] = a.accumulate ? caddf(P[i], acc[q]) : acc[q];
        }
    }
}

typedef void (*MigFn)(const Args);
template <bool BIG> MigFn stolt_fn(int flag) {
    switch (flag) {
        case 0: return mig_stolt<0, BIG>;
        case 1: return mig_stolt<1, BIG>;
        case 2: return mig_stolt<2, BIG>;
        case 3: return mig_stolt<3, BIG>;
        default: return mig_stolt<5, BIG>;
    }
}

}  // namespace mig
}  // namespace qdas

namespace {
// bytes of the F x K x (transmits) work buffer of one block (QDAS_MIGRATION_BLOCK_BYTES, read per call: the tests make it small to see several blocks)
size_t mig_block_bytes() { const char *e = getenv("QDAS_MIGRATION_BLOCK_BYTES"); return e && atoll(e) > 0 ? (size_t)atoll(e) : (size_t)64 << 20; }
// workgroups pass C wants before the block's transmits stop being split into slices (QDAS_MIGRATION_FILL, read per call)
uint32_t mig_fill() { const char *e = getenv("QDAS_MIGRATION_FILL"); return e && atoll(e) > 0 ? (uint32_t)std::min<long long>(atoll(e), 1 << 20) : 512u; }
bool finite_pos(double v) { return v > 0.0 && v < INFINITY; }
}  // namespace

extern "C" int qdas_migration(const qdas_migration_desc *d, const void *x, void *b, void *stream) {
    using namespace qdas;
    using namespace qdas::mig;
    if (!d) return fail(QDAS_EINVAL, "migration: null descriptor");
    if (d->flag != 0 && d->flag != 1 && d->flag != 2 && d->flag != 3 && d->flag != 5) return fail(QDAS_EINVAL, "migration: unknown interpolator flag (0 nearest, 1 linear, 2 cubic, 3 lanczos3, 5 cubic_dev)");
    if ((d->keep_tx != 0 && d->keep_tx != 1) || (d->jacobian != 0 && d->jacobian != 1)) return fail(QDAS_EINVAL, "migration: keep_tx and jacobian are 0 or 1");
    const uint64_t LIM = 0x7fffff00ull;
    if (d->T > LIM || d->N > LIM || d->M > LIM || d->frames > LIM || d->F > LIM || d->K > LIM) return fail(QDAS_EUNSUPPORTED, "migration: every extent is at most 2^31 - 256");
    if (d->T == 0 || d->N == 0 || d->M == 0 || d->frames == 0) return QDAS_OK;               // b has no elements: nothing is launched
    if (d->F == 0 || d->K == 0) return fail(QDAS_EINVAL, "migration: the transform lengths F and K are positive");
    if (!finite_pos(d->fs) || !finite_pos(d->c0) || !finite_pos(d->pitch)) return fail(QDAS_EINVAL, "migration: fs, c0 and pitch are positive and finite");
    if (!(fabs(d->t0) < INFINITY) || !(fabs(d->fmod) < INFINITY)) return fail(QDAS_EINVAL, "migration: t0 and fmod are finite");
    Args a{};
    unsigned thF = 0, thK = 0;
    if (!fft_factor(d->F, a.stF, thF) || !fft_factor(d->K, a.stK, thK))
        return fail(QDAS_ENOTLDS, "migration: a transform length outside the in-LDS path (products of 2, 3, 5, 7, 11, 13 from 2 to 8192 whose stages fit a workgroup)");
    const uint32_t F = (uint32_t)d->F, K = (uint32_t)d->K;
    const uint32_t RS = fft_lds_points(K) | 1u;
    const size_t ldsK = sizeof(float2) * 2 * TF * RS, ldsF = sizeof(float2) * fft_lds_points(F), ldsC = 2 * ldsF;
    if (ldsK > LAT_LDS_MAX) return fail(QDAS_ENOTLDS, "migration: K outside the in-LDS path (two tiles of 16 x K points exceed the 160 KiB of LDS)");
    if (!x || !b || !d->tau || !d->gamma) return fail(QDAS_EINVAL, "migration: null data pointer");
    DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;

    const uint32_t M = (uint32_t)d->M, Fk = (uint32_t)std::min<uint64_t>(d->T, F), Nn = (uint32_t)std::min<uint64_t>(d->N, K);
    const size_t per = (size_t)F * K * sizeof(float2);
    const uint32_t Mb = (uint32_t)std::min<size_t>(std::min<uint32_t>(M, 65535u), std::max<size_t>(1, mig_block_bytes() / per));
    uint32_t nslice = 1, mper = Mb;
    if (!d->keep_tx) {
        const uint32_t want = std::min<uint32_t>(std::min<uint32_t>(Mb, 8u), std::max<uint32_t>(1u, (mig_fill() + K - 1) / K));
        mper = (Mb + want - 1) / want;
        nslice = (Mb + mper - 1) / mper;
    }
    const size_t slice = (size_t)Fk * K;
    Scratch scratch(s);
    float2 *tw = (float2 *)scratch.get(sizeof(float2) * ((size_t)F + K));
    float2 *W = (float2 *)scratch.get(per * Mb);
    float2 *P = (float2 *)scratch.get(slice * sizeof(float2) * (d->keep_tx ? Mb : nslice));
    if (!tw || !W || !P) return fail(QDAS_ENOMEM, "migration: no memory for the work space");
    auto hip_fail = [&](hipError_t e) { (void)hipStreamSynchronize(s); return fail(QDAS_EHIP, "%s", hipGetErrorString(e)); };

    const bool big = (thF >> 16) != 0;
    const unsigned nthF = thF & 0xffffu;
    const MigFn fnA = big ? (MigFn)mig_time<true> : (MigFn)mig_time<false>;
    const MigFn fnC = big ? stolt_fn<true>(d->flag) : stolt_fn<false>(d->flag);
    hipError_t e = hipSuccess;
    if (ldsF > 65536 && (e = hipFuncSetAttribute((const void *)fnA, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsF)) != hipSuccess) return hip_fail(e);
    if (ldsC > 65536 && (e = hipFuncSetAttribute((const void *)fnC, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsC)) != hipSuccess) return hip_fail(e);
    if (ldsK > 65536) {
        if ((e = hipFuncSetAttribute((const void *)mig_lateral<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsK)) != hipSuccess) return hip_fail(e);
        if ((e = hipFuncSetAttribute((const void *)mig_lateral<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsK)) != hipSuccess) return hip_fail(e);
    }

    a.x = (const float2 *)x; a.W = W; a.P = P; a.twF = tw; a.twK = tw + F; a.tau = d->tau; a.gamma = d->gamma;
    a.T = (uint32_t)d->T; a.N = (uint32_t)d->N; a.M = M; a.F = F; a.K = K; a.Fk = Fk; a.Nn = Nn; a.RS = RS; a.mper = mper;
    a.slice_stride = slice;
    a.fs = d->fs; a.fmod = d->fmod; a.t0 = d->t0; a.c0 = d->c0; a.pitch = d->pitch; a.keep_tx = d->keep_tx; a.jacobian = d->jacobian;
    fft_twiddles_kernel<<<(F + 255) / 256, 256, 0, s>>>(tw, F);
    fft_twiddles_kernel<<<(K + 255) / 256, 256, 0, s>>>(tw + F, K);
    const unsigned ftF = (F + TF - 1) / TF, ftD = (Fk + TF - 1) / TF;
    for (uint64_t fr = 0; fr < d->frames; ++fr) {
        a.frame = fr;
        for (uint32_t m0 = 0; m0 < M; m0 += Mb) {
            a.m0 = m0; a.mb = std::min(Mb, M - m0); a.accumulate = m0 > 0; a.nslice = nslice;
            fnA<<<dim3(Nn, a.mb), nthF, ldsF, s>>>(a);
            mig_lateral<false><<<dim3(ftF, a.mb), 256, ldsK, s>>>(a);
            fnC<<<dim3(K, (a.mb + mper - 1) / mper), nthF, ldsC, s>>>(a);
            if (d->keep_tx) {
                a.nslice = 1;
                a.b = (float2 *)b + (size_t)Fk * Nn * (m0 + (size_t)M * fr);
                mig_lateral<true><<<dim3(ftD, a.mb), 256, ldsK, s>>>(a);
            }
        }
        if (!d->keep_tx) {
            a.b = (float2 *)b + (size_t)Fk * Nn * fr;
            mig_lateral<true><<<dim3(ftD, 1), 256, ldsK, s>>>(a);
        }
    }
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
    return QDAS_OK;
}
