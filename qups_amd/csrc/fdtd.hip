// fdtd.hip -- qdas_fdtd: a linear, lossless, first-order acoustic FDTD solver of order 2R on a 2-D staggered grid, V pulses stepped together, from the
// medium maps and a source table to a sensor record without leaving the device (include/qdas.h states the scheme; the arithmetic is fdtd_core.h, shared
// with a host test).  qdas_fdtd_lossy is the same solver with power-law absorption: relaxation mechanisms (memory variables) or the Stokes term in the
// density pass, density_lossy_kernel below; the velocity pass and the host loop are shared.
//
// MI355X mapping.  Two launches per time step, Nt steps enqueued as plain launches by a host loop (no graph):
//   * velocity_kernel (steps 1-2): a workgroup of 256 lanes owns 64 (z, along lanes) x 16 (x) nodes of one pulse, stages p with a halo of R in LDS, updates
//     uz and ux, and -- behind a barrier -- adds the source samples of the sources inside its tile.
//   * density_kernel (steps 3-5): stages uz (halo in z) and ux (halo in x), updates rz and rx, writes p, and -- behind a barrier -- records the sensors
//     inside its tile.
//   The pulse is the slowest grid dimension (blockIdx.y): all tiles of pulse v are dispatched before pulse v + 1, so the medium maps are re-read once per
//   pulse, from L2 or the Infinity Cache where they fit (not measured).
//   A wave is one row of 64 consecutive z: every global access is a contiguous 256-byte (fp32) run, every LDS access is stride 1 along lanes (conflict-free).
//   * BYTES per node, step and pulse (fp32): velocity reads p, uz, ux and writes uz, ux (20), density reads uz, ux, rz, rx and writes rz, rx, p (28); the
//     four medium maps add 16 / V.  The halo re-reads (a factor (TZ + 2R)(TX + 2R) / (TZ TX) = 1.69 on p at R = 4) are served by L2.
//   * LDS: 6.9 KiB (velocity) and 10.8 KiB (density) at R = 4 in fp32, twice that in fp64.
//   * No atomics: every node has one owner, sources and sensors sit on distinct nodes and belong to the tile that holds them.  The pulse stride is 64-bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/qdas.h"
#include "api_util.h"
#include "fdtd_core.h"

namespace qdas {
namespace fd {

template <int R, typename T>
__global__ void __launch_bounds__(LANES) velocity_kernel(const Params<T> P, const int64_t n, const int inj) {
    __shared__ T lds[lds_words_vel(R)];
    const int t = threadIdx.x, tile = blockIdx.x, v = blockIdx.y;
    const int i0 = (tile % P.ntz) * TZ, j0 = (tile / P.ntz) * TX;
    const int64_t off = (int64_t)v * P.vs;
    stage(lds, P.p + off, i0, j0, R, R, P.Nz, P.Nx, P.ld, t);
    __syncthreads();
    velocity_cells<R, T>(P, lds, P.uz + off, P.ux + off, i0, j0, t);
    if (inj && P.src_start[tile + 1] > P.src_start[tile]) {          // (uniform)
        __syncthreads();
        inject(P, P.uz + off, P.ux + off, tile, n, v, t);
    }
}

template <int R, typename T>
__global__ void __launch_bounds__(LANES) density_kernel(const Params<T> P, const int64_t n) {
    __shared__ T lds[lds_words_den(R)];
    T *lz = lds, *lx = lds + (TZ + 2 * R) * TX;
    const int t = threadIdx.x, tile = blockIdx.x, v = blockIdx.y;
    const int i0 = (tile % P.ntz) * TZ, j0 = (tile / P.ntz) * TX;
    const int64_t off = (int64_t)v * P.vs;
    stage(lz, P.uz + off, i0, j0, R, 0, P.Nz, P.Nx, P.ld, t);
    stage(lx, P.ux + off, i0, j0, 0, R, P.Nz, P.Nx, P.ld, t);
    __syncthreads();
    density_cells<R, T>(P, lz, lx, P.rz + off, P.rx + off, P.p + off, i0, j0, t);
    if (P.N > 0 && P.sen_start[tile + 1] > P.sen_start[tile]) {      // (uniform)
        __syncthreads();
        record(P, P.p + off, tile, n, v, t);
    }
}

// the density pass with absorption: density_kernel with density_cells_lossy in place of density_cells (L = 0: Stokes, L = 1 .. 4: relaxation).  The memory
// variables of pulse v start at e + v L vs; they add 2 L words of traffic per node (read and write) and the map one.
template <int R, typename T, int L>
__global__ void __launch_bounds__(LANES) density_lossy_kernel(const Params<T> P, const int64_t n, const Loss<T> Q) {
    __shared__ T lds[lds_words_den(R)];
    T *lz = lds, *lx = lds + (TZ + 2 * R) * TX;
    const int t = threadIdx.x, tile = blockIdx.x, v = blockIdx.y;
    const int i0 = (tile % P.ntz) * TZ, j0 = (tile / P.ntz) * TX;
    const int64_t off = (int64_t)v * P.vs;
    stage(lz, P.uz + off, i0, j0, R, 0, P.Nz, P.Nx, P.ld, t);
    stage(lx, P.ux + off, i0, j0, 0, R, P.Nz, P.Nx, P.ld, t);
    __syncthreads();
    density_cells_lossy<R, T, L>(P, Q, lz, lx, P.rz + off, P.rx + off, P.p + off, L > 0 ? Q.e + off * L : nullptr, i0, j0, t);
    if (P.N > 0 && P.sen_start[tile + 1] > P.sen_start[tile]) {      // (uniform)
        __syncthreads();
        record(P, P.p + off, tile, n, v, t);
    }
}

// the nonlinear density pass (qdas_fdtd_nonlinear): density_kernel with density_cells_nl.  L = 0 serves no absorption (Q.kap null) and Stokes alike -- ro is
// needed by the convective term anyway -- and L = 1 .. 4 relaxation.  The map bq adds one word of traffic per node.
template <int R, typename T, int L>
__global__ void __launch_bounds__(LANES) density_nl_kernel(const Params<T> P, const int64_t n, const Loss<T> Q, const Nl<T> N) {
    __shared__ T lds[lds_words_den(R)];
    T *lz = lds, *lx = lds + (TZ + 2 * R) * TX;
    const int t = threadIdx.x, tile = blockIdx.x, v = blockIdx.y;
    const int i0 = (tile % P.ntz) * TZ, j0 = (tile / P.ntz) * TX;
    const int64_t off = (int64_t)v * P.vs;
    stage(lz, P.uz + off, i0, j0, R, 0, P.Nz, P.Nx, P.ld, t);
    stage(lx, P.ux + off, i0, j0, 0, R, P.Nz, P.Nx, P.ld, t);
    __syncthreads();
    density_cells_nl<R, T, L>(P, Q, N, lz, lx, P.rz + off, P.rx + off, P.p + off, L > 0 ? Q.e + off * L : nullptr, i0, j0, t);
    if (P.N > 0 && P.sen_start[tile + 1] > P.sen_start[tile]) {      // (uniform)
        __syncthreads();
        record(P, P.p + off, tile, n, v, t);
    }
}

// the host loop of every variant: `den` is the density kernel of the call, `x` what it takes after (P, n)
template <int R, typename T, typename Den, typename... X>
static void run(const Params<T> &P, hipStream_t s, uint64_t Nt, uint64_t Ts, Den den, X... x) {
    const dim3 grid((uint32_t)(P.ntz * P.ntx), (uint32_t)P.V), block(LANES);
    const bool src = P.M > 0;
    for (uint64_t n = 0; n < Nt; ++n) {
        velocity_kernel<R, T><<<grid, block, 0, s>>>(P, (int64_t)n, src && n < Ts ? 1 : 0);
        den<<<grid, block, 0, s>>>(P, (int64_t)n, x...);
    }
}

template <typename T>
static Params<T> params(const qdas_fdtd_desc *d, const qdas_fdtd_args *a) {
    Params<T> P;
    memset(&P, 0, sizeof P);
    P.p = (T *)a->p; P.uz = (T *)a->uz; P.ux = (T *)a->ux; P.rz = (T *)a->rz; P.rx = (T *)a->rx;
    P.c2 = (const T *)a->c2; P.rho = (const T *)a->rho; P.dtrz = (const T *)a->dtrz; P.dtrx = (const T *)a->dtrx;
    P.az = (const T *)a->az; P.azs = (const T *)a->azs; P.ax = (const T *)a->ax; P.axs = (const T *)a->axs;
    P.s = (const T *)a->s; P.src_wz = (const T *)a->src_wz; P.src_wx = (const T *)a->src_wx;
    P.src_node = a->src_node; P.src_start = a->src_start; P.src_list = a->src_list;
    P.sen_node = a->sen_node; P.sen_start = a->sen_start; P.sen_list = a->sen_list;
    P.rec = (T *)a->rec;
    P.vs = (int64_t)d->vstride; P.ld = (int64_t)d->ld;
    P.rec_st = (int64_t)d->rec_st; P.rec_sn = (int64_t)d->rec_sn; P.rec_sv = (int64_t)d->rec_sv;
    P.Nz = (int32_t)d->Nz; P.Nx = (int32_t)d->Nx; P.ntz = (int32_t)tiles_z((int64_t)d->Nz); P.ntx = (int32_t)tiles_x((int64_t)d->Nx);
    P.M = (d->Ts > 0) ? (int32_t)d->M : 0; P.V = (int32_t)d->V; P.N = (int32_t)d->N;
    P.inv_h = (T)d->inv_h; P.dt_h = (T)d->dt_h;
    return P;
}

template <typename T>
static void run_order(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, hipStream_t s) {
    const Params<T> P = params<T>(d, a);
    switch (d->order) {
        case 2:  run<1, T>(P, s, d->Nt, d->Ts, density_kernel<1, T>); break;
        case 4:  run<2, T>(P, s, d->Nt, d->Ts, density_kernel<2, T>); break;
        default: run<4, T>(P, s, d->Nt, d->Ts, density_kernel<4, T>); break;
    }
}

template <int R, typename T>
static void run_mechanisms(const Params<T> &P, const Loss<T> &Q, int L, hipStream_t s, uint64_t Nt, uint64_t Ts) {
    switch (L) {
        case 0:  run<R, T>(P, s, Nt, Ts, density_lossy_kernel<R, T, 0>, Q); break;
        case 1:  run<R, T>(P, s, Nt, Ts, density_lossy_kernel<R, T, 1>, Q); break;
        case 2:  run<R, T>(P, s, Nt, Ts, density_lossy_kernel<R, T, 2>, Q); break;
        case 3:  run<R, T>(P, s, Nt, Ts, density_lossy_kernel<R, T, 3>, Q); break;
        default: run<R, T>(P, s, Nt, Ts, density_lossy_kernel<R, T, 4>, Q); break;
    }
}

template <typename T>
static Loss<T> loss_block(const qdas_fdtd_loss *l) {
    Loss<T> Q;
    memset(&Q, 0, sizeof Q);
    if (!l) return Q;
    Q.kap = (const T *)l->kap; Q.e = (T *)l->e;
    for (int k = 0; k < l->L; ++k) { Q.g[k] = (T)l->g[k]; Q.E[k] = (T)l->E[k]; }
    return Q;
}

template <typename T>
static void run_order_lossy(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l, hipStream_t s) {
    const Params<T> P = params<T>(d, a);
    const Loss<T> Q = loss_block<T>(l);
    switch (d->order) {
        case 2:  run_mechanisms<1, T>(P, Q, l->L, s, d->Nt, d->Ts); break;
        case 4:  run_mechanisms<2, T>(P, Q, l->L, s, d->Nt, d->Ts); break;
        default: run_mechanisms<4, T>(P, Q, l->L, s, d->Nt, d->Ts); break;
    }
}

template <int R, typename T>
static void run_mechanisms_nl(const Params<T> &P, const Loss<T> &Q, const Nl<T> &N, int L, hipStream_t s, uint64_t Nt, uint64_t Ts) {
    switch (L) {
        case 0:  run<R, T>(P, s, Nt, Ts, density_nl_kernel<R, T, 0>, Q, N); break;
        case 1:  run<R, T>(P, s, Nt, Ts, density_nl_kernel<R, T, 1>, Q, N); break;
        case 2:  run<R, T>(P, s, Nt, Ts, density_nl_kernel<R, T, 2>, Q, N); break;
        case 3:  run<R, T>(P, s, Nt, Ts, density_nl_kernel<R, T, 3>, Q, N); break;
        default: run<R, T>(P, s, Nt, Ts, density_nl_kernel<R, T, 4>, Q, N); break;
    }
}

template <typename T>
static void run_order_nl(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l, const qdas_fdtd_nl *q, hipStream_t s) {
    const Params<T> P = params<T>(d, a);
    const Loss<T> Q = loss_block<T>(l);
    Nl<T> N;
    N.bq = (const T *)q->bq;
    N.K = (q->flags & QDAS_FDTD_NL_NO_CONVECTIVE) ? T(0) : T(2);
    const int L = l ? l->L : 0;
    switch (d->order) {
        case 2:  run_mechanisms_nl<1, T>(P, Q, N, L, s, d->Nt, d->Ts); break;
        case 4:  run_mechanisms_nl<2, T>(P, Q, N, L, s, d->Nt, d->Ts); break;
        default: run_mechanisms_nl<4, T>(P, Q, N, L, s, d->Nt, d->Ts); break;
    }
}

}  // namespace fd
}  // namespace qdas

using qdas::fail;

extern "C" uint64_t qdas_fdtd_tiles(uint64_t Nz, uint64_t Nx) { return (uint64_t)(qdas::fd::tiles_z((int64_t)Nz) * qdas::fd::tiles_x((int64_t)Nx)); }

extern "C" int qdas_fdtd_tile_lists(uint64_t Nz, uint64_t Nx, uint64_t n, const int32_t *node, int32_t *start, int32_t *list) {
    typedef unsigned long long ull;
    if (Nz == 0 || Nx == 0 || Nz * Nx >= (1ull << 31) || Nz >= (1ull << 31) || Nx >= (1ull << 31))
        return fail(QDAS_EINVAL, "fdtd: a grid of %llu x %llu nodes has no tiles to list", (ull)Nz, (ull)Nx);
    if (!start || (n && (!node || !list))) return fail(QDAS_EINVAL, "fdtd: null pointer (tile lists)");
    if (n >= (1ull << 31)) return fail(QDAS_EINVAL, "fdtd: %llu points", (ull)n);
    const int64_t rc = qdas::fd::tile_lists((int64_t)Nz, (int64_t)Nx, (int64_t)n, node, start, list);
    if (rc < 0) return fail(QDAS_EINVAL, "fdtd: point %lld sits at node %d, outside the grid of %llu x %llu nodes", (long long)(-1 - rc), node[-1 - rc], (ull)Nz, (ull)Nx);
    return QDAS_OK;
}

// the descriptor's rows of both entries, in the order include/qdas.h lists them; *work: the call has steps and pulses
static int check_desc(const qdas_fdtd_desc *d, bool *work) {
    using namespace qdas::fd;
    typedef unsigned long long ull;
    static_assert(QDAS_FDTD_TZ == TZ && QDAS_FDTD_TX == TX, "tile of include/qdas.h");
    *work = false;
    if (!d) return fail(QDAS_EINVAL, "fdtd: null descriptor");
    if (d->dtype != QDAS_F32 && d->dtype != QDAS_F64) return fail(QDAS_EINVAL, "fdtd: dtype is QDAS_F32 or QDAS_F64, got %d", d->dtype);
    if (d->Nz == 0 || d->Nx == 0) return fail(QDAS_EINVAL, "fdtd: the grid needs at least one node each way, got %llu x %llu", (ull)d->Nz, (ull)d->Nx);
    if (d->ld < d->Nz) return fail(QDAS_EINVAL, "fdtd: ld = %llu is less than Nz = %llu", (ull)d->ld, (ull)d->Nz);
    if (d->vstride / d->ld < d->Nx)                     // vstride < Nx ld, without the product (it may not fit 64 bits)
        return fail(QDAS_EINVAL, "fdtd: vstride = %llu is less than Nx ld = %llu x %llu", (ull)d->vstride, (ull)d->Nx, (ull)d->ld);
    if (d->flags & ~QDAS_FDTD_ZERO) return fail(QDAS_EINVAL, "fdtd: unknown flags 0x%x", (unsigned)d->flags);
    if (!(d->dt_h > 0.0) || !(d->inv_h > 0.0) || !isfinite(d->dt_h) || !isfinite(d->inv_h))
        return fail(QDAS_EINVAL, "fdtd: dt / h = %g and 1 / h = %g must be finite and positive", d->dt_h, d->inv_h);
    if (d->order != 2 && d->order != 4 && d->order != 8) return fail(QDAS_EUNSUPPORTED, "fdtd: order %d: built are 2, 4 and 8", d->order);
    if (d->Nz >= (1ull << 31) || d->Nx >= (1ull << 31) || d->ld >= (1ull << 40))
        return fail(QDAS_EUNSUPPORTED, "fdtd: Nz = %llu or Nx = %llu reaches 2^31, or ld = %llu reaches 2^40", (ull)d->Nz, (ull)d->Nx, (ull)d->ld);
    if (d->Nz * d->Nx >= (1ull << 31)) return fail(QDAS_EUNSUPPORTED, "fdtd: %llu x %llu nodes reach 2^31", (ull)d->Nz, (ull)d->Nx);
    if (d->V > 65535) return fail(QDAS_EUNSUPPORTED, "fdtd: V = %llu pulses in one call, at most 65535", (ull)d->V);
    if (d->M >= (1ull << 31) || d->N >= (1ull << 31) || d->Nt >= (1ull << 40) || d->Ts >= (1ull << 40) || d->vstride >= (1ull << 40) ||
        d->rec_st >= (1ull << 40) || d->rec_sn >= (1ull << 40) || d->rec_sv >= (1ull << 40))
        return fail(QDAS_EUNSUPPORTED, "fdtd: M, N reach 2^31 or Nt, Ts, a stride reach 2^40");
    *work = d->Nt != 0 && d->V != 0;
    return QDAS_OK;
}

// the argument block's rows, for a call that has work
static int check_args(const qdas_fdtd_desc *d, const qdas_fdtd_args *a) {
    if (!a) return fail(QDAS_EINVAL, "fdtd: null argument block");
    if (!a->p || !a->uz || !a->ux || !a->rz || !a->rx) return fail(QDAS_EINVAL, "fdtd: null pointer (a state array)");
    if (!a->c2 || !a->rho || !a->dtrz || !a->dtrx) return fail(QDAS_EINVAL, "fdtd: null pointer (a medium map)");
    if (!a->az || !a->azs || !a->ax || !a->axs) return fail(QDAS_EINVAL, "fdtd: null pointer (a PML vector)");
    if (d->M > 0 && d->Ts > 0 && (!a->s || !a->src_wz || !a->src_wx || !a->src_node || !a->src_start || !a->src_list))
        return fail(QDAS_EINVAL, "fdtd: null pointer (the sources)");
    if (d->N > 0 && (!a->rec || !a->sen_node || !a->sen_start || !a->sen_list)) return fail(QDAS_EINVAL, "fdtd: null pointer (the sensors)");
    return QDAS_OK;
}

// QDAS_FDTD_ZERO for `count` arrays of `pulses` pulses each: Nz elements of each of the Nx rows of a pulse, the padding left alone
static int clear_states(const qdas_fdtd_desc *d, void *const *st, int count, uint64_t pulses, hipStream_t s) {
    const size_t es = d->dtype == QDAS_F32 ? 4 : 8;
    const bool dense = d->ld == d->Nz && d->vstride == d->Nx * d->Nz;
    for (int k = 0; k < count; ++k) {
        if (dense) { HIPCHK(hipMemsetAsync(st[k], 0, pulses * d->vstride * es, s)); continue; }
        for (uint64_t v = 0; v < pulses; ++v)
            HIPCHK(hipMemset2DAsync((char *)st[k] + v * d->vstride * es, d->ld * es, 0, d->Nz * es, d->Nx, s));
    }
    return QDAS_OK;
}

extern "C" int qdas_fdtd(const qdas_fdtd_desc *d, const qdas_fdtd_args *a) {
    bool work;
    int rc = check_desc(d, &work);
    if (rc != QDAS_OK || !work) return rc;
    if ((rc = check_args(d, a)) != QDAS_OK) return rc;

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    if (d->flags & QDAS_FDTD_ZERO) {
        void *st[5] = {a->p, a->uz, a->ux, a->rz, a->rx};
        if ((rc = clear_states(d, st, 5, d->V, s)) != QDAS_OK) return rc;
    }
    if (d->dtype == QDAS_F32) qdas::fd::run_order<float>(d, a, s);
    else qdas::fd::run_order<double>(d, a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}

// the loss block's rows, before the pointers are looked at
static int check_loss(const qdas_fdtd_loss *l) {
    if (!l) return fail(QDAS_EINVAL, "fdtd: null loss block");
    if (l->mode != QDAS_FDTD_LOSS_STOKES && l->mode != QDAS_FDTD_LOSS_RELAX) return fail(QDAS_EINVAL, "fdtd: unknown loss mode %d", l->mode);
    if (l->L < 0 || l->L > QDAS_FDTD_MAX_L) return fail(QDAS_EINVAL, "fdtd: L = %d mechanisms, at most %d", l->L, QDAS_FDTD_MAX_L);
    if ((l->mode == QDAS_FDTD_LOSS_RELAX) != (l->L > 0))
        return fail(QDAS_EINVAL, "fdtd: L = %d with mode %d: relaxation has 1 .. %d mechanisms, Stokes none", l->L, l->mode, QDAS_FDTD_MAX_L);
    for (int k = 0; k < l->L; ++k) {
        if (!isfinite(l->g[k]) || l->g[k] < 0.0) return fail(QDAS_EINVAL, "fdtd: g[%d] = %g must be finite and not negative", k, l->g[k]);
        if (!(l->E[k] > 0.0 && l->E[k] <= 1.0)) return fail(QDAS_EINVAL, "fdtd: E[%d] = %g lies outside (0, 1]", k, l->E[k]);
    }
    return QDAS_OK;
}

// the loss block's pointers, for a call that has work
static int check_loss_work(const qdas_fdtd_desc *d, const qdas_fdtd_loss *l) {
    if (!l->kap || (l->L > 0 && !l->e)) return fail(QDAS_EINVAL, "fdtd: null pointer (the loss map or the memory variables)");
    if (d->V * (uint64_t)(l->L > 0 ? l->L : 1) * d->vstride >= (1ull << 62)) return fail(QDAS_EUNSUPPORTED, "fdtd: the memory variables pass 2^62 elements");
    return QDAS_OK;
}

// QDAS_FDTD_ZERO with an optional loss block: the memory variables are V L arrays of the states' layout
static int clear_all(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l, hipStream_t s) {
    void *st[6] = {a->p, a->uz, a->ux, a->rz, a->rx, l ? l->e : nullptr};
    int rc;
    if ((rc = clear_states(d, st, 5, d->V, s)) != QDAS_OK) return rc;
    if (l && l->L > 0 && (rc = clear_states(d, st + 5, 1, d->V * (uint64_t)l->L, s)) != QDAS_OK) return rc;
    return QDAS_OK;
}

extern "C" int qdas_fdtd_lossy(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l) {
    bool work;
    int rc = check_desc(d, &work);
    if (rc != QDAS_OK) return rc;
    if ((rc = check_loss(l)) != QDAS_OK) return rc;
    if (!work) return QDAS_OK;
    if ((rc = check_args(d, a)) != QDAS_OK) return rc;
    if ((rc = check_loss_work(d, l)) != QDAS_OK) return rc;

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    if ((d->flags & QDAS_FDTD_ZERO) && (rc = clear_all(d, a, l, s)) != QDAS_OK) return rc;
    if (d->dtype == QDAS_F32) qdas::fd::run_order_lossy<float>(d, a, l, s);
    else qdas::fd::run_order_lossy<double>(d, a, l, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}

extern "C" int qdas_fdtd_nonlinear(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l, const qdas_fdtd_nl *q) {
    bool work;
    int rc = check_desc(d, &work);
    if (rc != QDAS_OK) return rc;
    if (l && (rc = check_loss(l)) != QDAS_OK) return rc;
    if (!q) return fail(QDAS_EINVAL, "fdtd: null nonlinear block");
    if (q->flags & ~QDAS_FDTD_NL_NO_CONVECTIVE) return fail(QDAS_EINVAL, "fdtd: unknown flags 0x%x (the nonlinear block)", (unsigned)q->flags);
    if (!work) return QDAS_OK;
    if ((rc = check_args(d, a)) != QDAS_OK) return rc;
    if (l && (rc = check_loss_work(d, l)) != QDAS_OK) return rc;
    if (!q->bq) return fail(QDAS_EINVAL, "fdtd: null pointer (the nonlinearity map)");

    qdas::DeviceGuard guard(d->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice failed: %s", hipGetErrorString(guard.err));
    const hipStream_t s = (hipStream_t)d->queue;
    if ((d->flags & QDAS_FDTD_ZERO) && (rc = clear_all(d, a, l, s)) != QDAS_OK) return rc;
    if (d->dtype == QDAS_F32) qdas::fd::run_order_nl<float>(d, a, l, q, s);
    else qdas::fd::run_order_nl<double>(d, a, l, q, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QDAS_EHIP, "%s", hipGetErrorString(e));
    return QDAS_OK;
}
