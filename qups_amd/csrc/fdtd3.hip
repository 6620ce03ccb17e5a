// fdtd3.hip -- qdas_fdtd3: the solver of fdtd.hip with a third axis: linear, lossless, first order, of order 2R on a 3-D staggered grid, V pulses stepped
// together, from the medium maps and a source table to a sensor record without leaving the device (include/qdas.h states the scheme; the arithmetic is
// fdtd3_core.h, shared with a host test).
//
// MI355X mapping.  Two launches per time step, Nt steps enqueued as plain launches by a host loop (no graph):
//   * velocity_kernel (steps 1-2): a workgroup of 256 lanes owns a brick of 64 (z, along lanes) x TX (x) x TY (y) nodes of one pulse and marches along y.
//     Per plane it stages p with a halo of R in z and x in LDS -- the 2-D kernel's block -- and takes the y derivative from a window of 2R values of each of
//     its own columns held in registers, which slides by one plane per step of the march (one load per column and plane).  After the march, behind a barrier,
//     it adds the source samples of the sources inside its brick.  (Staging plane k + 1 in a second block while plane k is used -- one barrier per plane --
//     was measured and gained nothing: 1.753 against 1.746 ms per step on 148^3 nodes and 16 pulses.)
//   * density_kernel (steps 3-5): stages uz (halo in z) and ux (halo in x) per plane, slides a window of uy, updates rz, rx, ry, writes p, and -- behind a
//     barrier, after the march -- records the sensors inside its brick.
//   The pulse is the slowest grid dimension (blockIdx.y).  A wave is one row of 64 consecutive z: every global access is a contiguous 256-byte (fp32) run,
//   every LDS access is stride 1 along lanes.
//   * BYTES per node, step and pulse (fp32): velocity reads p, uz, ux, uy and writes uz, ux, uy (28), density reads the three u and the three r and writes
//     the three r and p (40); the five medium maps add 20 / V.  The z / x halo of a plane and the 2R - 1 planes beyond a brick's ends are read twice; they
//     are assumed to come from L2 and are not counted.
//   * LDS: 4.5 KiB (velocity) and 6.3 KiB (density) at R = 4 in fp32, twice that in fp64; none for y.
//   * No atomics: every node has one owner, sources and sensors sit on distinct nodes and belong to the brick that holds them.  Pulse, plane and row strides
//     are 64-bit; node indices are int32 (Nz Nx Ny < 2^31).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"
#include "fdtd3_core.h"

namespace qdas {
namespace fd3 {

template <int R, typename T>
__global__ void __launch_bounds__(LANES) velocity_kernel(const Params<T> P, const int64_t n, const int inj) {
    __shared__ T lds[lds_words_vel(R)];
    const int t = threadIdx.x, brick = blockIdx.x, v = blockIdx.y;
    const int i0 = (brick % P.nbz) * TZ, j0 = (brick / P.nbz % P.nbx) * TX, k0 = (brick / P.nbz / P.nbx) * TY;
    const int64_t off = (int64_t)v * P.vs;
    Window<R, T> win;
    window_fill<R, T>(P, P.p + off, win, i0, j0, k0 - R, t);
    for (int k = k0; k < k0 + TY && k < P.Ny; ++k) {                 // (uniform)
        window_slide<R, T>(P, P.p + off, win, i0, j0, k + R, t);
        stage(lds, P.p + off + (int64_t)k * P.ps, i0, j0, R, R, P.Nz, P.Nx, P.ld, t);
        __syncthreads();
        velocity_cells<R, T>(P, lds, win, P.uz + off, P.ux + off, P.uy + off, i0, j0, k, t);
        __syncthreads();
    }
    if (inj && P.src_start[brick + 1] > P.src_start[brick])         // (uniform; the barrier that ended the march is the one the injection needs)
        inject(P, P.uz + off, P.ux + off, P.uy + off, brick, n, v, t);
}

template <int R, typename T>
__global__ void __launch_bounds__(LANES) density_kernel(const Params<T> P, const int64_t n) {
    __shared__ T lds[lds_words_den(R)];
    T *lz = lds, *lx = lds + (TZ + 2 * R) * TX;
    const int t = threadIdx.x, brick = blockIdx.x, v = blockIdx.y;
    const int i0 = (brick % P.nbz) * TZ, j0 = (brick / P.nbz % P.nbx) * TX, k0 = (brick / P.nbz / P.nbx) * TY;
    const int64_t off = (int64_t)v * P.vs;
    Window<R, T> win;
    window_fill<R, T>(P, P.uy + off, win, i0, j0, k0 - R - 1, t);
    for (int k = k0; k < k0 + TY && k < P.Ny; ++k) {                 // (uniform)
        window_slide<R, T>(P, P.uy + off, win, i0, j0, k + R - 1, t);
        stage(lz, P.uz + off + (int64_t)k * P.ps, i0, j0, R, 0, P.Nz, P.Nx, P.ld, t);
        stage(lx, P.ux + off + (int64_t)k * P.ps, i0, j0, 0, R, P.Nz, P.Nx, P.ld, t);
        __syncthreads();
        density_cells<R, T>(P, lz, lx, win, P.rz + off, P.rx + off, P.ry + off, P.p + off, i0, j0, k, t);
        __syncthreads();
    }
    if (P.N > 0 && P.sen_start[brick + 1] > P.sen_start[brick])     // (uniform; behind the march's last barrier)
        record(P, P.p + off, brick, n, v, t);
}

template <int R, typename T>
static void run(const Params<T> &P, hipStream_t s, uint64_t Nt, uint64_t Ts) {
    const dim3 grid((uint32_t)((int64_t)P.nbz * P.nbx * P.nby), (uint32_t)P.V), block(LANES);
    const bool src = P.M > 0;
    for (uint64_t n = 0; n < Nt; ++n) {
        velocity_kernel<R, T><<<grid, block, 0, s>>>(P, (int64_t)n, src && n < Ts ? 1 : 0);
        density_kernel<R, T><<<grid, block, 0, s>>>(P, (int64_t)n);
    }
}

template <typename T>
static void run_order(const qdas_fdtd3_desc *d, const qdas_fdtd3_args *a, hipStream_t s) {
    Params<T> P;
    memset(&P, 0, sizeof P);
    P.p = (T *)a->p; P.uz = (T *)a->uz; P.ux = (T *)a->ux; P.uy = (T *)a->uy; P.rz = (T *)a->rz; P.rx = (T *)a->rx; P.ry = (T *)a->ry;
    P.c2 = (const T *)a->c2; P.rho = (const T *)a->rho; P.dtrz = (const T *)a->dtrz; P.dtrx = (const T *)a->dtrx; P.dtry = (const T *)a->dtry;
    P.az = (const T *)a->az; P.azs = (const T *)a->azs; P.ax = (const T *)a->ax; P.axs = (const T *)a->axs; P.ay = (const T *)a->ay; P.ays = (const T *)a->ays;
    P.s = (const T *)a->s; P.src_wz = (const T *)a->src_wz; P.src_wx = (const T *)a->src_wx; P.src_wy = (const T *)a->src_wy;
    P.src_node = a->src_node; P.src_start = a->src_start; P.src_list = a->src_list;
    P.sen_node = a->sen_node; P.sen_start = a->sen_start; P.sen_list = a->sen_list;
    P.rec = (T *)a->rec;
    P.vs = (int64_t)d->vstride; P.ps = (int64_t)d->pstride; P.ld = (int64_t)d->ld;
    P.rec_st = (int64_t)d->rec_st; P.rec_sn = (int64_t)d->rec_sn; P.rec_sv = (int64_t)d->rec_sv;
    P.Nz = (int32_t)d->Nz; P.Nx = (int32_t)d->Nx; P.Ny = (int32_t)d->Ny;
    P.nbz = (int32_t)bricks_z((int64_t)d->Nz); P.nbx = (int32_t)bricks_x((int64_t)d->Nx); P.nby = (int32_t)bricks_y((int64_t)d->Ny);
    P.M = (d->Ts > 0) ? (int32_t)d->M : 0; P.V = (int32_t)d->V; P.N = (int32_t)d->N;
    P.inv_h = (T)d->inv_h; P.dt_h = (T)d->dt_h;
    switch (d->order) {
        case 2:  run<1, T>(P, s, d->Nt, d->Ts); break;
        case 4:  run<2, T>(P, s, d->Nt, d->Ts); break;
        default: run<4, T>(P, s, d->Nt, d->Ts); break;
    }
}

static bool fits(uint64_t Nz, uint64_t Nx, uint64_t Ny) {           // Nz Nx Ny < 2^31, without a product that leaves 64 bits
    const uint64_t lim = 1ull << 31;
    return Nz < lim && Nx < lim && Ny < lim && Nz * Nx < lim && Nz * Nx * Ny < lim;
}

}  // namespace fd3
}  // namespace qdas

using qdas::fail;

extern "C" uint64_t qdas_fdtd3_bricks(uint64_t Nz, uint64_t Nx, uint64_t Ny) {
    using namespace qdas::fd3;
    return (uint64_t)(bricks_z((int64_t)Nz) * bricks_x((int64_t)Nx) * bricks_y((int64_t)Ny));
}

extern "C" int qdas_fdtd3_brick_lists(uint64_t Nz, uint64_t Nx, uint64_t Ny, uint64_t n, const int32_t *node, int32_t *start, int32_t *list) {
    typedef unsigned long long ull;
    if (Nz == 0 || Nx == 0 || Ny == 0 || !qdas::fd3::fits(Nz, Nx, Ny))
        return fail(QDAS_EINVAL, "fdtd3: a grid of %llu x %llu x %llu nodes has no bricks to list", (ull)Nz, (ull)Nx, (ull)Ny);
    if (!start || (n && (!node || !list))) return fail(QDAS_EINVAL, "fdtd3: null pointer (brick lists)");
    if (n >= (1ull << 31)) return fail(QDAS_EINVAL, "fdtd3: %llu points", (ull)n);
    const int64_t rc = qdas::fd3::brick_lists((int64_t)Nz, (int64_t)Nx, (int64_t)Ny, (int64_t)n, node, start, list);
    if (rc < 0)
        return fail(QDAS_EINVAL, "fdtd3: point %lld sits at node %d, outside the grid of %llu x %llu x %llu nodes", (long long)(-1 - rc), node[-1 - rc], (ull)Nz,
                    (ull)Nx, (ull)Ny);
    return QDAS_OK;
}

extern "C" int qdas_fdtd3(const qdas_fdtd3_desc *d, const qdas_fdtd3_args *a) {
    using namespace qdas::fd3;
    typedef unsigned long long ull;
    static_assert(QDAS_FDTD3_TZ == TZ && QDAS_FDTD3_TX == TX && QDAS_FDTD3_TY == TY, "brick of include/qdas.h");
    static_assert(lds_words_den(4) * sizeof(double) <= 64 * 1024 && lds_words_vel(4) * sizeof(double) <= 64 * 1024, "LDS per workgroup");
    if (!d) return fail(QDAS_EINVAL, "fdtd3: null descriptor");
    if (d->dtype != QDAS_F32 && d->dtype != QDAS_F64) return fail(QDAS_EINVAL, "fdtd3: dtype is QDAS_F32 or QDAS_F64, got %d", d->dtype);
    if (d->Nz == 0 || d->Nx == 0 || d->Ny == 0)
        return fail(QDAS_EINVAL, "fdtd3: the grid needs at least one node each way, got %llu x %llu x %llu", (ull)d->Nz, (ull)d->Nx, (ull)d->Ny);
    if (d->ld < d->Nz) return fail(QDAS_EINVAL, "fdtd3: ld = %llu is less than Nz = %llu", (ull)d->ld, (ull)d->Nz);
    if (d->pstride / d->ld < d->Nx)                     // pstride < Nx ld, without the product (it may not fit 64 bits)
        return fail(QDAS_EINVAL, "fdtd3: pstride = %llu is less than Nx ld = %llu x %llu", (ull)d->pstride, (ull)d->Nx, (ull)d->ld);
    if (d->vstride / d->pstride < d->Ny)
        return fail(QDAS_EINVAL, "fdtd3: vstride = %llu is less than Ny pstride = %llu x %llu", (ull)d->vstride, (ull)d->Ny, (ull)d->pstride);
    if (d->flags & ~QDAS_FDTD3_ZERO) return fail(QDAS_EINVAL, "fdtd3: unknown flags 0x%x", (unsigned)d->flags);
    if (!(d->dt_h > 0.0) || !(d->inv_h > 0.0) || !isfinite(d->dt_h) || !isfinite(d->inv_h))
        return fail(QDAS_EINVAL, "fdtd3: dt / h = %g and 1 / h = %g must be finite and positive", d->dt_h, d->inv_h);
    if (d->order != 2 && d->order != 4 && d->order != 8) return fail(QDAS_EUNSUPPORTED, "fdtd3: order %d: built are 2, 4 and 8", d->order);
    if (d->Nz >= (1ull << 31) || d->Nx >= (1ull << 31) || d->Ny >= (1ull << 31) || d->ld >= (1ull << 40) || d->pstride >= (1ull << 44))
        return fail(QDAS_EUNSUPPORTED, "fdtd3: Nz = %llu, Nx = %llu or Ny = %llu reaches 2^31, ld = %llu reaches 2^40 or pstride = %llu reaches 2^44", (ull)d->Nz,
                    (ull)d->Nx, (ull)d->Ny, (ull)d->ld, (ull)d->pstride);
    if (!fits(d->Nz, d->Nx, d->Ny)) return fail(QDAS_EUNSUPPORTED, "fdtd3: %llu x %llu x %llu nodes reach 2^31", (ull)d->Nz, (ull)d->Nx, (ull)d->Ny);
    if (d->V > 65535) return fail(QDAS_EUNSUPPORTED, "fdtd3: V = %llu pulses in one call, at most 65535", (ull)d->V);
    if (d->M >= (1ull << 31) || d->N >= (1ull << 31) || d->Nt >= (1ull << 40) || d->Ts >= (1ull << 40) || d->vstride >= (1ull << 46) ||
        d->rec_st >= (1ull << 40) || d->rec_sn >= (1ull << 40) || d->rec_sv >= (1ull << 40))
        return fail(QDAS_EUNSUPPORTED, "fdtd3: M, N reach 2^31, Nt, Ts or a record stride reach 2^40, or vstride reaches 2^46");
    if (d->Nt == 0 || d->V == 0) return QDAS_OK;
    if (!a) return fail(QDAS_EINVAL, "fdtd3: null argument block");
    if (!a->p || !a->uz || !a->ux || !a->uy || !a->rz || !a->rx || !a->ry) return fail(QDAS_EINVAL, "fdtd3: null pointer (a state array)");
    if (!a->c2 || !a->rho || !a->dtrz || !a->dtrx || !a->dtry) return fail(QDAS_EINVAL, "fdtd3: null pointer (a medium map)");
    if (!a->az || !a->azs || !a->ax || !a->axs || !a->ay || !a->ays) return fail(QDAS_EINVAL, "fdtd3: null pointer (a PML vector)");
    if (d->M > 0 && d->Ts > 0 && (!a->s || !a->src_wz || !a->src_wx || !a->src_wy || !a->src_node || !a->src_start || !a->src_list))
        return fail(QDAS_EINVAL, "fdtd3: null pointer (the sources)");
    if (d->N > 0 && (!a->rec || !a->sen_node || !a->sen_start || !a->sen_list)) return fail(QDAS_EINVAL, "fdtd3: null pointer (the sensors)");

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    if (d->flags & QDAS_FDTD3_ZERO) {                   // Nz elements of each of the V Ny Nx rows, the padding left alone
        const size_t es = d->dtype == QDAS_F32 ? 4 : 8;
        void *st[7] = {a->p, a->uz, a->ux, a->uy, a->rz, a->rx, a->ry};
        const bool rows = d->pstride == d->Nx * d->ld, dense = rows && d->ld == d->Nz && d->vstride == d->Ny * d->pstride;
        for (void *p : st) {
            if (dense) { HIPCHK(hipMemsetAsync(p, 0, d->V * d->vstride * es, s)); continue; }
            for (uint64_t v = 0; v < d->V; ++v) {
                char *pv = (char *)p + v * d->vstride * es;
                if (rows) { HIPCHK(hipMemset2DAsync(pv, d->ld * es, 0, d->Nz * es, d->Nx * d->Ny, s)); continue; }
                for (uint64_t k = 0; k < d->Ny; ++k) HIPCHK(hipMemset2DAsync(pv + k * d->pstride * es, d->ld * es, 0, d->Nz * es, d->Nx, s));
            }
        }
    }
    if (d->dtype == QDAS_F32) run_order<float>(d, a, s);
    else run_order<double>(d, a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
