// refocus.hip -- REFoCUS recovery of full-synthetic-aperture channel data: qdas_refocus (include/qdas.h has the formulas; reference
// src/UltrasoundSystem.m:3505-3768).
//
// The reference transforms the whole record, multiplies by a phase, loops over the transmit elements with a broadcast product and a sum per element,
// multiplies by a second phase and transforms back: array operations over T x N x V x frames each.  Here the decoder pages Hi_k (M x V, built once per
// sequence on the host: qups_amd/refocus.py) are APPLIED in three passes of complex64, with C = N * frames columns (c = n + N * frame):
//
//   1  rf_fft     one workgroup per NT neighbouring columns of one pulse v: each trace x[:, n, v, frame] is loaded into its own LDS tile and transformed
//                 there (in place; the workgroup is two groups of threads, each on a trace of its own, where 512 threads hold two -- the second
//                 trace's loads and twiddles hide behind the first's), then all NT spectra are written together, times exp(-2 pi i f_k t0[v])
//                 (skipped when t0 is one value: it cancels against step 3's phase), so that a frequency's NT values are one run of 8 NT bytes.
//   2  rf_decode  per frequency k, Y_k (M x C) = Hi_k (M x V) X_k (V x C) on v_mfma_f32_32x32x2_f32: a workgroup of four waves owns a 64 x 64 tile of
//                 Y_k (a wave one 32 x 32 quarter), walks V in chunks of 32 staged through LDS as separate real and imaginary planes (rows past M, V
//                 and C are zeros), a complex product being four real MFMAs; the accumulators are multiplied by exp(+2 pi i f_k min t0) and stored.
//   3  rf_ifft    the mirror image of pass 1 for one element m: NT columns of Y are gathered per frequency, each is inverse-transformed in LDS
//                 (conjugate, forward transform, conjugate, times 1 / T) and written as the trace y[:, n, m, frame].
//
// No atomics and a fixed summation order: results are bit-reproducible.  f_k = k fs / T is NOT wrapped to negative frequencies (ChannelData.fftaxis,
// src/ChannelData.m:1491); the turns f_k t0 are formed in fp64 and reduced with rint before sincospif, as adjoint.hip and migration.hip do.
//
// Work buffer (the CALLER's: this file constructs no arena and allocates nothing), float2 units, after a 256-byte aligned table of T twiddles:
//   X[(k V + v) C + c]    T x V x C   written by pass 1, read by pass 2
//   Y[(k M + m) C + c]    T x M x C   written by pass 2, read by pass 3
// Column fastest, frequency slowest: pass 2 reads one contiguous V x C (and writes one M x C) page per frequency; passes 1 and 3 touch 8 NT bytes
// per (frequency, row).  NT = 16 (full 128-byte lines) up to T = 1024; the LDS tiles of NT traces (8 fft_lds_points(T) bytes each, at most 144 KiB
// together) halve it per doubling of T beyond: 8 at 2048, 4 at 4096, 2 at 8192 -- the neighbouring workgroup writes the other part of the line.
// Every element of X and Y that is read was written by the same call: the work buffer's previous content never matters.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <mutex>

#include "../../include/qdas.h"
#include "api_util.h"
#include "fft_lds.h"

namespace qdas {
namespace rf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT = 64, CT = 64;     // pass 2: rows (elements) and columns of Y_k per workgroup, 2 x 2 waves of 32 x 32
constexpr int VC = 32;              // pass 2: pulses per staged chunk
constexpr int LDT = 96;             // pass 2: LDS row stride of a staged plane (64 + 32: the two pulse rows a step reads sit 32 banks apart)
constexpr uint32_t TILES_LDS_MAX = 144u * 1024u;

struct Args {
    const float2 *x, *Hi;
    float2 *X, *Y, *y, *tw;
    const double *t0;
    uint32_t T, N, V, M, C, NT, TS, nth;                                 // C = N frames; NT traces per workgroup, TS their LDS tile stride, nth threads per trace
    FftStages st;
    double fs, t0_out;
    int32_t one_t0;
};

// ---- pass 1: x[t, n, v, frame] -> X[k, v, c]
template <bool BIG>
__global__ void __launch_bounds__(512) rf_fft(const Args a) {
    extern __shared__ float2 rf_lds[];
    const uint32_t T = a.T, NT = a.NT, c0 = blockIdx.x * NT, v = blockIdx.y, nc = min(NT, a.C - c0);
    const uint32_t nth = a.nth, grp = threadIdx.x / nth, tid = threadIdx.x - grp * nth, G = blockDim.x / nth;      // groups of whole waves, a trace each
    for (uint32_t jb = 0; jb < nc; jb += G) {
        const uint32_t j = jb + grp;
        const bool active = j < nc;
        float2 *tile = rf_lds + (active ? j : 0) * a.TS;
        if (active) {
            const uint32_t c = c0 + j, n = c % a.N, fr = c / a.N;
            const float2 *x = a.x + (uint64_t)T * (n + (uint64_t)a.N * (v + (uint64_t)a.V * fr));
            for (uint32_t i = tid; i < T; i += nth) tile[lds_pad(i)] = x[i];
        }
        __syncthreads();
        uint32_t Tj = T;
        asm volatile("" : "+s"(Tj));                                    // opaque per trace: the stage indices of every radix are not hoisted out of this loop (registers)
        lds_fft<BIG>(tile, a.tw, a.st, Tj, FftGroup{tid, nth, active});
    }
    const double dt = a.one_t0 ? 0.0 : a.t0[v] * (a.fs / (double)T);        // turns per frequency bin
    for (uint32_t idx = threadIdx.x; idx < NT * T; idx += blockDim.x) {
        const uint32_t j = idx % NT, k = idx / NT;
        if (j >= nc) continue;
        float2 val = rf_lds[j * a.TS + lds_pad(k)];
        if (!a.one_t0) val = cmulf(val, phasor(-((double)k * dt)));
        a.X[((uint64_t)k * a.V + v) * a.C + c0 + j] = val;
    }
}

// ---- pass 2: Y_k = Hi_k X_k, times exp(+2 pi i f_k min t0)
__global__ void __launch_bounds__(256) rf_decode(const Args a) {
    __shared__ float Ar[VC * LDT], Ai[VC * LDT], Br[VC * LDT], Bi[VC * LDT];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const uint32_t c0 = blockIdx.x * CT, m0 = blockIdx.y * MT, k = blockIdx.z, M = a.M, V = a.V, C = a.C;
    const uint32_t mw = (wave >> 1) * 32, cw = (wave & 1) * 32;          // this wave's quarter of the tile
    const float2 *Hk = a.Hi + (uint64_t)k * V * M, *Xk = a.X + (uint64_t)k * V * C;
    f32x16 yr = 0.f, yi = 0.f;
    for (uint32_t v0 = 0; v0 < V; v0 += VC) {
        __syncthreads();                                                // the previous chunk is consumed
#pragma unroll
        for (int r = 0; r < VC * MT / 256; ++r) {
            const uint32_t idx = tid + 256 * r, q = idx & 63, vl = idx >> 6, v = v0 + vl;
            float2 h = make_float2(0.f, 0.f), g = make_float2(0.f, 0.f);
            if (v < V && m0 + q < M) h = Hk[(uint64_t)v * M + m0 + q];
            if (v < V && c0 + q < C) g = Xk[(uint64_t)v * C + c0 + q];
            Ar[vl * LDT + q] = h.x; Ai[vl * LDT + q] = h.y;
            Br[vl * LDT + q] = g.x; Bi[vl * LDT + q] = g.y;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < VC / 2; ++s) {
            const uint32_t vl = 2 * s + half;
            const float ar = Ar[vl * LDT + mw + col], ai = Ai[vl * LDT + mw + col];
            const float br = Br[vl * LDT + cw + col], bi = Bi[vl * LDT + cw + col];
            yr = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, yr, 0, 0, 0);
            yr = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, bi, yr, 0, 0, 0);
            yi = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi, yi, 0, 0, 0);
            yi = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, yi, 0, 0, 0);
        }
    }
    float2 ph = make_float2(1.f, 0.f);
    if (!a.one_t0) ph = phasor((double)k * (a.t0_out * (a.fs / (double)a.T)));
    const uint32_t c = c0 + cw + col;
    float2 *Yk = a.Y + (uint64_t)k * M * C;
#pragma unroll
    for (int e = 0; e < 16; ++e) {                                      // lane l holds column l & 31 of rows 8 (e >> 2) + 4 (l >> 5) + (e & 3)
        const uint32_t m = m0 + mw + 8 * (e >> 2) + 4 * half + (e & 3);
        if (m < M && c < C) Yk[(uint64_t)m * C + c] = cmulf(make_float2(yr[e], yi[e]), ph);
    }
}

// ---- pass 3: Y[k, m, c] -> y[t, n, m, frame]
template <bool BIG>
__global__ void __launch_bounds__(512) rf_ifft(const Args a) {
    extern __shared__ float2 rf_lds[];
    const uint32_t T = a.T, NT = a.NT, c0 = blockIdx.x * NT, m = blockIdx.y, nc = min(NT, a.C - c0);
    for (uint32_t idx = threadIdx.x; idx < NT * T; idx += blockDim.x) {
        const uint32_t j = idx % NT, k = idx / NT;
        if (j >= nc) continue;
        const float2 val = a.Y[((uint64_t)k * a.M + m) * a.C + c0 + j];
        rf_lds[j * a.TS + lds_pad(k)] = make_float2(val.x, -val.y);      // ifft(Y) = conj(fft(conj(Y))) / T
    }
    __syncthreads();
    const float sc = 1.0f / (float)T;
    const uint32_t nth = a.nth, grp = threadIdx.x / nth, tid = threadIdx.x - grp * nth, G = blockDim.x / nth;
    for (uint32_t jb = 0; jb < nc; jb += G) {
        const uint32_t j = jb + grp;
        const bool active = j < nc;
        float2 *tile = rf_lds + (active ? j : 0) * a.TS;
        uint32_t Tj = T;
        asm volatile("" : "+s"(Tj));                                    // (as in pass 1)
        lds_fft<BIG>(tile, a.tw, a.st, Tj, FftGroup{tid, nth, active});
        if (active) {
            const uint32_t c = c0 + j, n = c % a.N, fr = c / a.N;
            float2 *y = a.y + (uint64_t)T * (n + (uint64_t)a.N * (m + (uint64_t)a.M * fr));
            for (uint32_t i = tid; i < T; i += nth) { const float2 t = tile[lds_pad(i)]; y[i] = make_float2(t.x * sc, -t.y * sc); }
        }
    }
}

// what the host side derives from the descriptor: 0, or the code `fail` returned
struct Plan { FftStages st; unsigned threads; uint32_t NT, TS; size_t off_X, off_Y, bytes; };

static int plan(const qdas_refocus_desc *d, Plan &p) {
    const uint64_t LIM = 0x7fffff00ull;
    if (d->T > LIM || d->N > LIM || d->V > LIM || d->M > LIM || d->frames > LIM) return fail(QDAS_EUNSUPPORTED, "refocus: every extent is at most 2^31 - 256");
    if (!fft_factor(d->T, p.st, p.threads))
        return fail(QDAS_ENOTLDS, "refocus: a record length outside the in-LDS path (products of 2, 3, 5, 7, 11, 13 from 2 to 8192 whose stages fit a workgroup)");
    if (d->N * d->frames > LIM) return fail(QDAS_EUNSUPPORTED, "refocus: N * frames is at most 2^31 - 256");
    if (d->V > 65535 || d->M > 65535) return fail(QDAS_EUNSUPPORTED, "refocus: at most 65535 pulses and 65535 elements");
    const uint32_t T = (uint32_t)d->T;
    p.TS = fft_lds_points(T) | 1u;
    p.NT = 16;
    while (p.NT > 1 && (size_t)p.NT * p.TS * sizeof(float2) > TILES_LDS_MAX) p.NT /= 2;
    const size_t C = (size_t)(d->N * d->frames);
    p.off_X = ((size_t)T * sizeof(float2) + 255) & ~(size_t)255;
    p.off_Y = p.off_X + (size_t)T * d->V * C * sizeof(float2);
    p.bytes = p.off_Y + (size_t)T * d->M * C * sizeof(float2);
    return QDAS_OK;
}

}  // namespace rf
}  // namespace qdas

using qdas::fail;

extern "C" int qdas_refocus_work_bytes(const qdas_refocus_desc *d, uint64_t *bytes) {
    if (!d || !bytes) return fail(QDAS_EINVAL, "refocus: null descriptor or result pointer");
    *bytes = 0;
    if (d->T == 0 || d->N == 0 || d->V == 0 || d->M == 0 || d->frames == 0) return QDAS_OK;
    qdas::rf::Plan p;
    if (const int rc = qdas::rf::plan(d, p)) return rc;
    *bytes = p.bytes;
    return QDAS_OK;
}

extern "C" int qdas_refocus(const qdas_refocus_desc *d, const void *x, const void *Hi, void *y, void *work, uint64_t work_bytes) {
    using namespace qdas::rf;
    if (!d) return fail(QDAS_EINVAL, "refocus: null descriptor");
    if (d->one_t0 != 0 && d->one_t0 != 1) return fail(QDAS_EINVAL, "refocus: one_t0 is 0 or 1");
    if (d->T == 0 || d->N == 0 || d->V == 0 || d->M == 0 || d->frames == 0) return QDAS_OK;     // y has no elements, or the sum over pulses none: nothing is launched
    Plan p;
    if (const int rc = plan(d, p)) return rc;
    if (!(d->fs > 0.0 && d->fs < INFINITY) || !(fabs(d->t0_out) < INFINITY)) return fail(QDAS_EINVAL, "refocus: fs is positive and finite, t0_out finite");
    if (!x || !Hi || !y || !work || (!d->one_t0 && !d->t0)) return fail(QDAS_EINVAL, "refocus: null data pointer");
    if (work_bytes < p.bytes) return fail(QDAS_EINVAL, "refocus: the work space holds %llu bytes, %llu are needed (qdas_refocus_work_bytes)", (unsigned long long)work_bytes, (unsigned long long)p.bytes);
    if (((uintptr_t)work & 7u) != 0) return fail(QDAS_EINVAL, "refocus: the work space must be aligned to 8 bytes");
    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)d->queue;

    Args a{};
    a.x = (const float2 *)x; a.Hi = (const float2 *)Hi; a.y = (float2 *)y; a.t0 = d->t0;
    a.tw = (float2 *)work; a.X = (float2 *)((char *)work + p.off_X); a.Y = (float2 *)((char *)work + p.off_Y);
    a.T = (uint32_t)d->T; a.N = (uint32_t)d->N; a.V = (uint32_t)d->V; a.M = (uint32_t)d->M; a.C = (uint32_t)(d->N * d->frames);
    a.NT = p.NT; a.TS = p.TS; a.st = p.st; a.fs = d->fs; a.t0_out = d->t0_out; a.one_t0 = d->one_t0;

    const bool big = (p.threads >> 16) != 0;
    const unsigned nth = p.threads & 0xffffu, ngrp = (2 * nth <= 512 && a.NT > 1 && a.C > 1) ? 2 : 1;       // two traces at a time where 512 threads hold them
    a.nth = nth;
    typedef void (*Fn)(const Args);
    const Fn f1 = big ? (Fn)rf_fft<true> : (Fn)rf_fft<false>, f3 = big ? (Fn)rf_ifft<true> : (Fn)rf_ifft<false>;
    const size_t lds = (size_t)std::min<uint32_t>(a.NT, a.C) * a.TS * sizeof(float2);
    auto hip_fail = [&](hipError_t e) { return fail(QDAS_EHIP, "%s", hipGetErrorString(e)); };
    hipError_t e = hipSuccess;
    if (lds > 65536) {                                                  // once per (device, variant): the limit is raised to the most any call asks for
        static std::mutex mu;
        static uint64_t raised[2] = {0, 0};                             // bit = device ordinal, per variant
        int dev = 0;
        if ((e = hipGetDevice(&dev)) != hipSuccess) return hip_fail(e);
        std::lock_guard<std::mutex> lock(mu);
        if (dev < 0 || dev > 63 || !(raised[big] >> dev & 1)) {
            if ((e = hipFuncSetAttribute((const void *)f1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TILES_LDS_MAX)) != hipSuccess) return hip_fail(e);
            if ((e = hipFuncSetAttribute((const void *)f3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TILES_LDS_MAX)) != hipSuccess) return hip_fail(e);
            if (dev >= 0 && dev <= 63) raised[big] |= 1ull << dev;
        }
    }
    const unsigned gc = (a.C + a.NT - 1) / a.NT;
    qdas::fft_twiddles_kernel<<<(a.T + 255) / 256, 256, 0, s>>>(a.tw, a.T);
    f1<<<dim3(gc, a.V), nth * ngrp, lds, s>>>(a);
    rf_decode<<<dim3((a.C + CT - 1) / CT, (a.M + MT - 1) / MT, a.T), 256, 0, s>>>(a);
    f3<<<dim3(gc, a.M), nth * ngrp, lds, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
    return QDAS_OK;
}
