// adjoint.hip -- the frequency-domain adjoint beamformer: qdas_adjoint (include/qdas.h has the formulas).
//
// What the reference's bfAdjoint does in a parfor over frequency blocks of pagemtimes on materialised I x N x F phasor arrays
// (src/UltrasoundSystem.m:3997-4037): per frequency two dense complex contractions, pixels x aperture against aperture x transmits.  Here the left
// operand never exists in memory: it is the Green's phasor exp(-+2 pi i f tau(i, n)), and each lane generates the element of the MFMA A operand it owns.
//
// adj_mfma (keep_rx = 0).  A workgroup of 4 waves owns 128 pixels (32 per wave: the M side of v_mfma_f32_32x32x2_f32) and a contiguous chunk of the
// selected frequencies.  Per frequency and per group of NVT x 32 transmits the aperture is walked in chunks of 32 elements: the chunk of X[k] (receive)
// or S[k] (transmit; S is written once per call by adj_steer) is staged through LDS for all of the tile's pixels -- rows padded with zeros past N / M / V --,
// then 16 MFMA steps of K = 2 each consume it: lane l supplies the phasor of pixel l & 31 and element 2 s + (l >> 5), and a complex product is four real
// MFMAs (re += ar br, re += (-ai) bi, im += ar bi, im += ai br).  The epilogue is VALU work on the accumulators (lane l holds transmit l & 31 of
// rows 8 (e >> 2) + 4 (l >> 5) + (e & 3)): |A|^2 summed over the transmits with shuffles, a_m R conj(A) / ||A||, and the sum over k in registers.
// Frequencies are split across workgroups only to fill the device at small I; the partial images are then added in frequency order by adj_reduce:
// no floating-point atomics anywhere, b is written once.
//
// Phase.  f tau reaches hundreds of cycles, so it is formed in fp64 -- |P - Pi| from the fp32 coordinates, times cinv, times f_k -- and reduced to
// [-1/2, 1/2] cycles (minus rint) BEFORE the conversion to fp32 and sincospif: the error of the fractional cycle is that of one fp64 product, whatever k.
// The product is formed anew per (pixel, element, k) rather than carried: carrying df tau in fp64 for N + M = 256 elements is 512 VGPRs per lane, the
// whole file; forming it costs ~20 fp64 operations that issue beside the MFMAs.
//
// keep_tx runs the same kernel twice: MODE_NORM (transmit half only) writes ||A[i,:,k]||^2, MODE_KEEPTX takes one transmit group per workgroup over all
// frequencies.  keep_rx is plain VALU code (adj_ahat, adj_keeprx) in the role das_generic.hip plays for DAS: correctness, no performance claim.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

#include "../../include/qdas.h"
#include "api_util.h"
#include "qdas_kernels.h"

namespace qdas {
namespace adj {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PT = 128;             // pixels per workgroup: 4 waves x 32 rows
constexpr int EC = 32;              // aperture elements per staged chunk
constexpr int LDB = 33;             // LDS row stride of a staged tile (32 transmits + 1: the staging writes walk the rows)
constexpr int MODE_SUM = 0, MODE_NORM = 1, MODE_KEEPTX = 2;

struct Args {
    const float *Pi, *Pr, *Pt, *cinv;
    const double *freq;             // device copy
    const float2 *X, *S;            // Ksel x V x N, Ksel x V x M
    const float *a_n, *a_m;
    float2 *out;                    // MODE_SUM: b, or kchunks x I partial images; MODE_KEEPTX: b
    float *nrm2;                    // Ksel x icount: MODE_NORM writes, MODE_KEEPTX reads
    uint32_t I, i0, icount, N, M, V, Ksel, kchunk;
    int cinv_one;
};

__device__ __forceinline__ void phasor(double px, double py, double pz, const float *e, double cinv, double f, float &c, float &s) {
    const double dx = px - (double)e[0], dy = py - (double)e[1], dz = pz - (double)e[2];
    double cyc = f * (sqrt(dx * dx + dy * dy + dz * dz) * cinv);
    cyc -= rint(cyc);
    sincospif(2.0f * (float)cyc, &s, &c);
}

// one side of the contraction for NVT tiles of 32 transmits from v0: C += phasor(pixel, element) x G[k] over all Ne elements
template <bool TX, int NVT>
__device__ __forceinline__ void contract(f32x16 (&cr)[NVT], f32x16 (&ci)[NVT], const float2 *__restrict__ G, const float *__restrict__ Epos, uint32_t Ne,
                                         uint32_t V, uint32_t v0, const float *__restrict__ an, uint32_t I, double f, double px, double py, double pz,
                                         double cinv, float *Br, float *Bi, float *Es) {
    const uint32_t tid = threadIdx.x, col = tid & 31, half = (tid & 63) >> 5;
    for (uint32_t e0 = 0; e0 < Ne; e0 += EC) {
        __syncthreads();                                  // the previous chunk is consumed
#pragma unroll
        for (int t = 0; t < NVT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t el = tid & 31, vl = (tid >> 5) + 8 * r, e = e0 + el, v = v0 + 32 * t + vl;
                float2 g = make_float2(0.f, 0.f);
                if (e < Ne && v < V) g = G[(size_t)v * Ne + e];
                Br[t * EC * LDB + el * LDB + vl] = g.x;
                Bi[t * EC * LDB + el * LDB + vl] = g.y;
            }
        if (tid < 3 * EC) { const uint32_t e = e0 + tid / 3; Es[tid] = e < Ne ? Epos[3 * (size_t)e + tid % 3] : 0.f; }
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < EC / 2; ++s) {
            const uint32_t el = 2 * s + half, e = e0 + el;
            float pr, pi;
            phasor(px, py, pz, Es + 3 * el, cinv, f, pr, pi);
            if (TX) pi = -pi;
            if (!TX && an) { const float w = e < Ne ? an[(size_t)e * I] : 0.f; pr *= w; pi *= w; }
            if (e >= Ne) pr = pi = 0.f;
#pragma unroll
            for (int t = 0; t < NVT; ++t) {
                const float br = Br[t * EC * LDB + el * LDB + col], bi = Bi[t * EC * LDB + el * LDB + col];
                cr[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(pr, br, cr[t], 0, 0, 0);
                cr[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(-pi, bi, cr[t], 0, 0, 0);
                ci[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(pr, bi, ci[t], 0, 0, 0);
                ci[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(pi, br, ci[t], 0, 0, 0);
            }
        }
    }
}

__device__ __forceinline__ float sum32(float v) {         // over the 32 lanes that share lane >> 5
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

template <int MODE, int NVT>
__global__ __launch_bounds__(256) void adj_mfma(const Args a) {
    __shared__ float Br[NVT * EC * LDB], Bi[NVT * EC * LDB], Es[3 * EC];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    // the pixel whose phasors this lane generates (rows past the block repeat its last pixel and are never written)
    const uint32_t pbase = blockIdx.x * PT + wave * 32;
    const uint32_t p = a.i0 + min(pbase + col, a.icount - 1);
    const double px = a.Pi[3 * (size_t)p], py = a.Pi[3 * (size_t)p + 1], pz = a.Pi[3 * (size_t)p + 2];
    const double cinv = a.cinv_one ? a.cinv[0] : a.cinv[p];
    const float *an = a.a_n ? a.a_n + p : nullptr;
    const uint32_t VG = NVT * 32, nvg = (a.V + VG - 1) / VG;
    uint32_t k0 = 0, k1 = a.Ksel;
    if (MODE != MODE_KEEPTX) { k0 = blockIdx.y * a.kchunk; k1 = min(a.Ksel, k0 + a.kchunk); }
    auto row = [&](int e) { return pbase + 8 * (e >> 2) + 4 * half + (e & 3); };      // block-local pixel of accumulator element e

    f32x16 br[MODE == MODE_KEEPTX ? NVT : 1], bi[MODE == MODE_KEEPTX ? NVT : 1];      // the image, summed over k
#pragma unroll
    for (int t = 0; t < (MODE == MODE_KEEPTX ? NVT : 1); ++t) { br[t] = 0.f; bi[t] = 0.f; }

    for (uint32_t k = k0; k < k1; ++k) {
        const double f = a.freq[k];
        const float2 *Xk = a.X + (size_t)k * a.V * a.N, *Sk = a.S + (size_t)k * a.V * a.M;
        f32x16 nr = 0.f, ni = 0.f, nn = 0.f;             // this frequency: sum_v a_m R conj(A), sum_v |A|^2, per lane
        float inv[16];
        if (MODE == MODE_KEEPTX) {
#pragma unroll
            for (int e = 0; e < 16; ++e) inv[e] = 1.0f / sqrtf(a.nrm2[(size_t)k * a.icount + min(row(e), a.icount - 1)]);
        }
        for (uint32_t vg = (MODE == MODE_KEEPTX ? blockIdx.y : 0); vg < (MODE == MODE_KEEPTX ? blockIdx.y + 1 : nvg); ++vg) {
            const uint32_t v0 = vg * VG;
            f32x16 Ar[NVT], Ai[NVT], Rr[NVT], Ri[NVT];
#pragma unroll
            for (int t = 0; t < NVT; ++t) { Ar[t] = 0.f; Ai[t] = 0.f; Rr[t] = 0.f; Ri[t] = 0.f; }
            contract<true, NVT>(Ar, Ai, Sk, a.Pt, a.M, a.V, v0, nullptr, a.I, f, px, py, pz, cinv, Br, Bi, Es);
            if (MODE != MODE_NORM) contract<false, NVT>(Rr, Ri, Xk, a.Pr, a.N, a.V, v0, an, a.I, f, px, py, pz, cinv, Br, Bi, Es);
#pragma unroll
            for (int t = 0; t < NVT; ++t) {
                const uint32_t v = v0 + 32 * t + col;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (MODE == MODE_NORM) { nn[e] += Ar[t][e] * Ar[t][e] + Ai[t][e] * Ai[t][e]; continue; }
                    float am = 1.f;
                    if (a.a_m) am = v < a.V ? a.a_m[(size_t)v * a.I + a.i0 + min(row(e), a.icount - 1)] : 0.f;
                    const float yr = am * (Rr[t][e] * Ar[t][e] + Ri[t][e] * Ai[t][e]), yi = am * (Ri[t][e] * Ar[t][e] - Rr[t][e] * Ai[t][e]);
                    if (MODE == MODE_KEEPTX) { br[t][e] += yr * inv[e]; bi[t][e] += yi * inv[e]; }
                    else { nr[e] += yr; ni[e] += yi; nn[e] += Ar[t][e] * Ar[t][e] + Ai[t][e] * Ai[t][e]; }
                }
            }
        }
        if (MODE == MODE_NORM) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float n2 = sum32(nn[e]);
                if (col == 0 && row(e) < a.icount) a.nrm2[(size_t)k * a.icount + row(e)] = n2;
            }
        }
        if (MODE == MODE_SUM) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float w = 1.0f / sqrtf(sum32(nn[e]));
                br[0][e] += nr[e] * w; bi[0][e] += ni[e] * w;
            }
        }
    }
    if (MODE == MODE_SUM) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float yr = sum32(br[0][e]), yi = sum32(bi[0][e]);
            if (col == 0 && row(e) < a.icount) a.out[(size_t)blockIdx.y * a.icount + row(e)] = make_float2(yr, yi);
        }
    }
    if (MODE == MODE_KEEPTX) {
#pragma unroll
        for (int t = 0; t < NVT; ++t) {
            const uint32_t v = blockIdx.y * VG + 32 * t + col;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (v < a.V && row(e) < a.icount) a.out[(size_t)v * a.I + a.i0 + row(e)] = make_float2(br[t][e], bi[t][e]);
        }
    }
}

// b[i] = sum over the frequency chunks, in order
__global__ void adj_reduce(const float2 *__restrict__ part, float2 *__restrict__ b, uint32_t I, uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    float yr = 0.f, yi = 0.f;
    for (uint32_t c = 0; c < nchunks; ++c) { const float2 v = part[(size_t)c * I + i]; yr += v.x; yi += v.y; }
    b[i] = make_float2(yr, yi);
}

// S[k][v][m] = apod_tx[m, v] exp(-2 pi i f_k del_tx[m, v])
__global__ void adj_steer(const double *__restrict__ freq, const double *__restrict__ del, const float *__restrict__ apod, float2 *__restrict__ S, size_t MV, size_t total) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x) {
        const size_t k = j / MV, mv = j - k * MV;
        double cyc = freq[k] * del[mv];
        cyc -= rint(cyc);
        float s, c;
        sincospif(2.0f * (float)cyc, &s, &c);
        const float w = apod[mv];
        S[j] = make_float2(w * c, -w * s);
    }
}

// ---- keep_rx: plain vector code.  Ah[k][v][pl] = A / ||A|| for the pixels of one block
__global__ void adj_ahat(const Args a, float2 *__restrict__ Ah) {
    const size_t total = (size_t)a.icount * a.Ksel;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = (uint32_t)(j / a.icount), pl = (uint32_t)(j - (size_t)k * a.icount), p = a.i0 + pl;
        const double px = a.Pi[3 * (size_t)p], py = a.Pi[3 * (size_t)p + 1], pz = a.Pi[3 * (size_t)p + 2];
        const double cinv = a.cinv_one ? a.cinv[0] : a.cinv[p], f = a.freq[k];
        float n2 = 0.f;
        for (uint32_t v = 0; v < a.V; ++v) {
            const float2 *Sv = a.S + ((size_t)k * a.V + v) * a.M;
            float yr = 0.f, yi = 0.f;
            for (uint32_t m = 0; m < a.M; ++m) {
                float c, s;
                phasor(px, py, pz, a.Pt + 3 * (size_t)m, cinv, f, c, s);
                const float2 g = Sv[m];
                yr += c * g.x + s * g.y;                   // (c - i s)(g.x + i g.y)
                yi += c * g.y - s * g.x;
            }
            Ah[((size_t)k * a.V + v) * a.icount + pl] = make_float2(yr, yi);
            n2 += yr * yr + yi * yi;
        }
        const float w = 1.0f / sqrtf(n2);
        for (uint32_t v = 0; v < a.V; ++v) {
            float2 &y = Ah[((size_t)k * a.V + v) * a.icount + pl];
            y = make_float2(y.x * w, y.y * w);
        }
    }
}

// b[i, n (, v)] = sum_k sum_v a_m a_n exp(+2 pi i f_k tau_rx) X[k, v, n] conj(Ah[k, v, i])
__global__ void adj_keeprx(const Args a, const float2 *__restrict__ Ah, int keep_tx) {
    const uint32_t Vo = keep_tx ? a.V : 1;
    const size_t total = (size_t)a.icount * a.N * Vo;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x) {
        const uint32_t pl = (uint32_t)(j % a.icount), n = (uint32_t)((j / a.icount) % a.N), vo = (uint32_t)(j / ((size_t)a.icount * a.N)), p = a.i0 + pl;
        const double px = a.Pi[3 * (size_t)p], py = a.Pi[3 * (size_t)p + 1], pz = a.Pi[3 * (size_t)p + 2];
        const double cinv = a.cinv_one ? a.cinv[0] : a.cinv[p];
        const float an = a.a_n ? a.a_n[(size_t)n * a.I + p] : 1.f;
        const uint32_t va = keep_tx ? vo : 0, vb = keep_tx ? vo + 1 : a.V;
        float yr = 0.f, yi = 0.f;
        for (uint32_t k = 0; k < a.Ksel; ++k) {
            float c, s;
            phasor(px, py, pz, a.Pr + 3 * (size_t)n, cinv, a.freq[k], c, s);
            float zr = 0.f, zi = 0.f;                    // sum_v a_m X conj(Ah)
            for (uint32_t v = va; v < vb; ++v) {
                const float2 x = a.X[((size_t)k * a.V + v) * a.N + n], h = Ah[((size_t)k * a.V + v) * a.icount + pl];
                const float am = a.a_m ? a.a_m[(size_t)v * a.I + p] : 1.f;
                zr += am * (x.x * h.x + x.y * h.y);
                zi += am * (x.y * h.x - x.x * h.y);
            }
            yr += an * (c * zr - s * zi);
            yi += an * (c * zi + s * zr);
        }
        a.out[p + (size_t)a.I * (n + (size_t)a.N * vo)] = make_float2(yr, yi);
    }
}

}  // namespace adj
}  // namespace qdas

using qdas::fail;
using qdas::DeviceGuard;

namespace {
// work space of one pixel block of the keep_tx / keep_rx forms: 256 MiB (QDAS_ADJOINT_BLOCK_BYTES, read per call: the tests make it small to see several blocks)
size_t adj_block_bytes() { const char *e = getenv("QDAS_ADJOINT_BLOCK_BYTES"); return e && atoll(e) > 0 ? (size_t)atoll(e) : (size_t)256 << 20; }
// workgroups wanted before the frequencies stop being split: 512 (QDAS_ADJOINT_FILL, read per call: the tests set it to see one chunk, or many)
uint32_t adj_fill() { const char *e = getenv("QDAS_ADJOINT_FILL"); return e && atoll(e) > 0 ? (uint32_t)std::min<long long>(atoll(e), 1 << 20) : 512u; }

template <int MODE>
void adj_launch(const qdas::adj::Args &a, dim3 grid, hipStream_t s) {
    using namespace qdas::adj;
    if (a.V <= 32) adj_mfma<MODE, 1><<<grid, 256, 0, s>>>(a);
    else adj_mfma<MODE, 2><<<grid, 256, 0, s>>>(a);
}
unsigned adj_blocks(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, 1u << 20); }
}  // namespace

extern "C" int qdas_adjoint(const qdas_adjoint_desc *d, const void *X, void *b, void *stream) {
    using namespace qdas::adj;
    if (!d) return fail(QDAS_EINVAL, "adjoint: null descriptor");
    if (d->dtype == QDAS_F16 || d->dtype == QDAS_F64) return fail(QDAS_EUNSUPPORTED, "adjoint: complex64 data only (half precision is insufficient for frequency-domain beamforming; there is no fp64 path)");
    if (d->dtype != QDAS_F32) return fail(QDAS_EINVAL, "adjoint: unknown dtype");
    if ((d->keep_rx != 0 && d->keep_rx != 1) || (d->keep_tx != 0 && d->keep_tx != 1)) return fail(QDAS_EINVAL, "adjoint: keep_rx and keep_tx are 0 or 1");
    const uint64_t LIM = 0x7fffff00ull;
    if (d->I > LIM || d->N > LIM || d->M > LIM || d->V > LIM || d->Ksel > LIM) return fail(QDAS_EUNSUPPORTED, "adjoint: every extent is at most 2^31 - 256");
    if (d->cinv_count != 1 && d->cinv_count != d->I) return fail(QDAS_EINVAL, "adjoint: cinv holds 1 or I values");
    if (d->I == 0 || (d->keep_rx && d->N == 0) || (d->keep_tx && d->V == 0)) return QDAS_OK;          // b has no elements: nothing is launched
    if (!b) return fail(QDAS_EINVAL, "adjoint: null output pointer");
    DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const size_t nout = (size_t)d->I * (d->keep_rx ? d->N : 1) * (d->keep_tx ? d->V : 1);
    if (d->N == 0 || d->V == 0 || d->Ksel == 0) {           // an empty sum: zeros, no kernel
        const hipError_t e = hipMemsetAsync(b, 0, nout * sizeof(float2), s);
        return e == hipSuccess ? QDAS_OK : fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    }
    if (d->M == 0) return fail(QDAS_EINVAL, "adjoint: no transmit elements (M = 0): the transmit field has no norm");
    if (!X || !d->Pi || !d->Pr || !d->Pt || !d->cinv || !d->freq || !d->del_tx || !d->apod_tx) return fail(QDAS_EINVAL, "adjoint: null data pointer");
    const uint32_t I = (uint32_t)d->I, N = (uint32_t)d->N, M = (uint32_t)d->M, V = (uint32_t)d->V, K = (uint32_t)d->Ksel;
    const uint32_t VG = V <= 32 ? 32 : 64, nvg = (V + VG - 1) / VG;
    if (nvg > 65535) return fail(QDAS_EUNSUPPORTED, "adjoint: at most 65535 x 64 transmits");

    // the pixels of one launch: all of them for the summed image; blocks under the work-space budget for the kept forms
    const size_t per_pixel = d->keep_rx ? (size_t)K * V * sizeof(float2) : (d->keep_tx ? (size_t)K * sizeof(float) : 0);
    uint32_t IB = I;
    if (per_pixel) {
        const size_t fit = std::max<size_t>(1, adj_block_bytes() / per_pixel);
        if (fit < I) IB = (uint32_t)(fit >= PT ? fit / PT * PT : fit);
    }
    const uint32_t ptiles = (IB + PT - 1) / PT;
    uint32_t kchunks = std::min<uint32_t>(std::min<uint32_t>(K, 65535), std::max<uint32_t>(1, adj_fill() / ptiles));
    const uint32_t kchunk = (K + kchunks - 1) / kchunks;
    kchunks = (K + kchunk - 1) / kchunk;

    const size_t nS = (size_t)K * V * M;
    const size_t off_S = ((size_t)K * sizeof(double) + 255) & ~(size_t)255;
    qdas::Scratch scratch(s);
    char *w0 = (char *)scratch.get(off_S + nS * sizeof(float2));
    const bool partial = !d->keep_rx && !d->keep_tx && kchunks > 1;
    void *w1 = per_pixel ? scratch.get(per_pixel * IB) : (partial ? scratch.get((size_t)kchunks * I * sizeof(float2)) : nullptr);
    if (!w0 || ((per_pixel || partial) && !w1)) return fail(QDAS_ENOMEM, "adjoint: no memory for the work space");
    auto hip_fail = [&](hipError_t e) { (void)hipStreamSynchronize(s); return fail(QDAS_EHIP, "%s", hipGetErrorString(e)); };
    hipError_t e = hipMemcpyAsync(w0, d->freq, (size_t)K * sizeof(double), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e);

    Args a{};
    a.Pi = d->Pi; a.Pr = d->Pr; a.Pt = d->Pt; a.cinv = d->cinv; a.cinv_one = d->cinv_count == 1;
    a.freq = (const double *)w0; a.X = (const float2 *)X; a.S = (const float2 *)(w0 + off_S);
    a.a_n = d->a_n; a.a_m = d->a_m;
    a.I = I; a.N = N; a.M = M; a.V = V; a.Ksel = K; a.kchunk = kchunk;
    adj_steer<<<adj_blocks(nS), 256, 0, s>>>(a.freq, d->del_tx, d->apod_tx, (float2 *)a.S, (size_t)M * V, nS);

    if (!d->keep_rx && !d->keep_tx) {
        a.i0 = 0; a.icount = I;
        a.out = partial ? (float2 *)w1 : (float2 *)b;
        adj_launch<MODE_SUM>(a, dim3(ptiles, kchunks), s);
        if (partial) adj_reduce<<<(I + 255) / 256, 256, 0, s>>>((const float2 *)w1, (float2 *)b, I, kchunks);
    } else {
        a.out = (float2 *)b;
        for (uint32_t i0 = 0; i0 < I; i0 += IB) {
            a.i0 = i0; a.icount = std::min(IB, I - i0);
            const uint32_t pt = (a.icount + PT - 1) / PT;
            if (d->keep_rx) {
                adj_ahat<<<adj_blocks((size_t)a.icount * K), 256, 0, s>>>(a, (float2 *)w1);
                adj_keeprx<<<adj_blocks((size_t)a.icount * N * (d->keep_tx ? V : 1)), 256, 0, s>>>(a, (const float2 *)w1, d->keep_tx);
            } else {
                a.nrm2 = (float *)w1;
                adj_launch<MODE_NORM>(a, dim3(pt, kchunks), s);
                adj_launch<MODE_KEEPTX>(a, dim3(pt, nvg), s);
            }
        }
    }
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
    return QDAS_OK;
}
