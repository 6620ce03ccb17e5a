// fdtd3_core.h -- the per-cell arithmetic and the per-lane loops of fdtd3.hip, the 3-D twin of fdtd_core.h: the staging of one plane of a brick with its z / x
// halo, the sliding window of a lane's own column along y, the two cell updates, the source injection, the sensor record and the per-brick point lists.
// Plain C++ with no HIP in it: the same text compiles for the host, where tests/fdtd3_core_host.cpp walks the bricks lane by lane on the CPU under the
// sanitizers (every LDS block and every lane's window a heap block of exactly its size).  coef, dplus, dminus and pml_update are those of fdtd_core.h.
//
// THE SCHEME (include/qdas.h states it in full).  Nz x Nx x Ny nodes, z fastest, then x, then y; p, rz, rx, ry at (i, j, k), uz at (i + 1/2, j, k), ux at
// (i, j + 1/2, k), uy at (i, j, k + 1/2).  One step n:
//   1. u_a <- A+_a (A+_a u_a - dtr_a D+_a p)                    a = z, x, y
//   2. u_a[src] += w_a s[n, m, v]                               w_a = n_a 2 c dt / h
//   3. r_a <- A_a (A_a r_a - dt rho D-_a u_a)
//   4. p = c2 ((rz + rx) + ry)
//   5. rec[n, j, v] = p[sensor j]
// Steps 1-2 are the velocity pass, 3-5 the density pass.
//
// THE BRICK.  A workgroup of LANES = 256 lanes owns TZ x TX x TY nodes of one pulse and marches along y, plane by plane.  Lane t has z offset t mod 64 (a wave
// is one contiguous row of 64) and the columns (t div 64) + 4 r, r = 0 .. PER_LANE - 1, of every plane.  Per plane the velocity pass stages p with a halo of R
// in z and x ((TZ + 2R) x (TX + 2R) words), the density pass uz with a halo in z and ux with a halo in x, exactly as the 2-D tile does.  The y derivative
// needs no LDS: each lane keeps the 2R values of ITS OWN columns it needs -- p[k - R + 1 .. k + R] for D+y at k + 1/2, uy[k - R .. k + R - 1] for D-y at k --
// in a window (registers on the device) that slides by one plane per step of the march: one new value per column and plane.  Only the 2R - 1 planes beyond a
// brick's two ends are read by two bricks.  Anything outside the grid reads as 0 and is never loaded.  Every node is updated by exactly one lane; the sources
// and sensors of a brick are listed per brick (brick_lists), and the lanes of the brick that updated them inject and record them behind a barrier, after the
// march: no atomics, no flags.
#pragma once
#include "fdtd_core.h"

namespace qdas {
namespace fd3 {

using fd::coef;
using fd::dminus;
using fd::dplus;
using fd::pml_update;

constexpr int TZ = 64, TX = 8, TY = 8, LANES = 256, ROWS = LANES / TZ, PER_LANE = TX / ROWS;
static_assert(TX % ROWS == 0 && PER_LANE >= 1, "a lane owns whole columns");

template <typename T>
struct Params {
    T *p, *uz, *ux, *uy, *rz, *rx, *ry;         // the seven state arrays: element (i, j, k) of pulse v at v vs + k ps + j ld + i
    const T *c2, *rho, *dtrz, *dtrx, *dtry;     // the medium, Ny x Nx x Nz dense, shared by the pulses
    const T *az, *azs, *ax, *axs, *ay, *ays;    // the PML factors: Nz, Nz, Nx, Nx, Ny, Ny
    const T *s;                                 // the source table: s[(n M + m) V + v], n < Ts
    const T *src_wz, *src_wx, *src_wy;          // per source: n_a 2 c dt / h
    const int32_t *src_node, *src_start, *src_list;   // node (k Nx + j) Nz + i of source m; brick b owns src_list[src_start[b] .. src_start[b + 1])
    const int32_t *sen_node, *sen_start, *sen_list;
    T *rec;                                     // rec[n rec_st + j rec_sn + v rec_sv]
    int64_t vs, ps, ld;
    int64_t rec_st, rec_sn, rec_sv;
    int32_t Nz, Nx, Ny, nbz, nbx, nby, M, V, N;
    T inv_h, dt_h;                              // 1 / h, dt / h
};

constexpr int lds_words_vel(int R) { return (TZ + 2 * R) * (TX + 2 * R); }
constexpr int lds_words_den(int R) { return (TZ + 2 * R) * TX + TZ * (TX + 2 * R); }

// one lane's share of staging one plane (`src` points at its node (0, 0)) of the brick at (i0, j0) with halos (hz, hx): element (a, b) of the block is node
// (i0 - hz + a, j0 - hx + b), 0 outside the grid.  The addressing of fd::stage: a wave per row, 64 consecutive z, then the 2 hz that remain.
template <typename T>
QDAS_FD_HD void stage(T *lds, const T *src, int i0, int j0, int hz, int hx, int Nz, int Nx, int64_t ld, int t) {
    const int W = TZ + 2 * hz, H = TX + 2 * hx, l = t % TZ;
    for (int b = t / TZ; b < H; b += ROWS) {
        const int j = j0 - hx + b;
        const bool row = j >= 0 && j < Nx;
        const int i = i0 - hz + l;
        lds[b * W + l] = (row && i >= 0 && i < Nz) ? src[(int64_t)j * ld + i] : T(0);
        if (l < 2 * hz) {
            const int i2 = i + TZ;
            lds[b * W + TZ + l] = (row && i2 >= 0 && i2 < Nz) ? src[(int64_t)j * ld + i2] : T(0);
        }
    }
}

// the window of lane t: w[r][q], q = 0 .. 2R - 1, consecutive planes of the lane's column r
template <int R, typename T>
struct Window {
    T w[PER_LANE][2 * R];
};

// f (a pulse's array) at the lane's column r in plane k, 0 outside the grid
template <typename T>
QDAS_FD_HD T column_at(const Params<T> &P, const T *f, int i, int j, int k) {
    return (i < P.Nz && j < P.Nx && k >= 0 && k < P.Ny) ? f[(int64_t)k * P.ps + (int64_t)j * P.ld + i] : T(0);
}

// before the march: slots 1 .. 2R - 1 take the planes k1 + 1 .. k1 + 2R - 1 (slot 0 leaves with the first slide)
template <int R, typename T>
QDAS_FD_HD void window_fill(const Params<T> &P, const T *f, Window<R, T> &win, int i0, int j0, int k1, int t) {
    const int i = i0 + t % TZ;
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int j = j0 + t / TZ + r * ROWS;
        win.w[r][0] = T(0);
QDAS_FD_UNROLL
        for (int q = 1; q < 2 * R; ++q) win.w[r][q] = column_at(P, f, i, j, k1 + q);
    }
}

// one plane on: every slot moves down by one, the last takes plane k_new
template <int R, typename T>
QDAS_FD_HD void window_slide(const Params<T> &P, const T *f, Window<R, T> &win, int i0, int j0, int k_new, int t) {
    const int i = i0 + t % TZ;
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int j = j0 + t / TZ + r * ROWS;
QDAS_FD_UNROLL
        for (int q = 0; q + 1 < 2 * R; ++q) win.w[r][q] = win.w[r][q + 1];
        win.w[r][2 * R - 1] = column_at(P, f, i, j, k_new);
    }
}

// step 1 for the nodes of lane t in plane k (lds: p of the plane with a halo of R in z and x; win: p[k - R + 1 .. k + R] of the lane's columns)
template <int R, typename T>
QDAS_FD_HD void velocity_cells(const Params<T> &P, const T *lds, const Window<R, T> &win, T *uz, T *ux, T *uy, int i0, int j0, int k, int t) {
    constexpr int W = TZ + 2 * R;
    const int tz = t % TZ, i = i0 + tz;
    if (i >= P.Nz) return;
    const T a = P.azs[i], cy = P.ays[k];
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int jl = t / TZ + r * ROWS, j = j0 + jl;
        if (j < P.Nx) {
            const T *pc = lds + (jl + R) * W + (tz + R);
            const int64_t o = (int64_t)k * P.ps + (int64_t)j * P.ld + i, m = ((int64_t)k * P.Nx + j) * P.Nz + i;
            const T b = P.axs[j];
            uz[o] = pml_update(uz[o], a, P.dtrz[m] * P.inv_h, dplus<R, T>(pc, 1));
            ux[o] = pml_update(ux[o], b, P.dtrx[m] * P.inv_h, dplus<R, T>(pc, W));
            uy[o] = pml_update(uy[o], cy, P.dtry[m] * P.inv_h, dplus<R, T>(&win.w[r][R - 1], 1));
        }
    }
}

// node -> element offset of a pulse's array
template <typename T>
QDAS_FD_HD int64_t node_offset(const Params<T> &P, int node) {
    const int i = node % P.Nz, jk = node / P.Nz;
    return (int64_t)(jk / P.Nx) * P.ps + (int64_t)(jk % P.Nx) * P.ld + i;
}

// step 2 for the sources of `brick` (behind a barrier: the lanes that updated these nodes belong to this workgroup)
template <typename T>
QDAS_FD_HD void inject(const Params<T> &P, T *uz, T *ux, T *uy, int brick, int64_t n, int v, int t) {
    const int e = P.src_start[brick + 1];
    for (int q = P.src_start[brick] + t; q < e; q += LANES) {
        const int m = P.src_list[q];
        const int64_t o = node_offset(P, P.src_node[m]);
        const T sv = P.s[((int64_t)n * P.M + m) * P.V + v];
        uz[o] += P.src_wz[m] * sv;
        ux[o] += P.src_wx[m] * sv;
        uy[o] += P.src_wy[m] * sv;
    }
}

// steps 3 and 4 for the nodes of lane t in plane k (lz: uz with a halo in z, lx: ux with a halo in x; win: uy[k - R .. k + R - 1] of the lane's columns)
template <int R, typename T>
QDAS_FD_HD void density_cells(const Params<T> &P, const T *lz, const T *lx, const Window<R, T> &win, T *rz, T *rx, T *ry, T *p, int i0, int j0, int k, int t) {
    constexpr int W = TZ + 2 * R;
    const int tz = t % TZ, i = i0 + tz;
    if (i >= P.Nz) return;
    const T a = P.az[i], cy = P.ay[k];
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int jl = t / TZ + r * ROWS, j = j0 + jl;
        if (j < P.Nx) {
            const int64_t o = (int64_t)k * P.ps + (int64_t)j * P.ld + i, m = ((int64_t)k * P.Nx + j) * P.Nz + i;
            const T b = P.ax[j], w = P.dt_h * P.rho[m];
            const T vz = pml_update(rz[o], a, w, dminus<R, T>(lz + jl * W + (tz + R), 1));
            const T vx = pml_update(rx[o], b, w, dminus<R, T>(lx + (jl + R) * TZ + tz, TZ));
            const T vy = pml_update(ry[o], cy, w, dminus<R, T>(&win.w[r][R], 1));
            rz[o] = vz;
            rx[o] = vx;
            ry[o] = vy;
            p[o] = P.c2[m] * ((vz + vx) + vy);
        }
    }
}

// step 5 for the sensors of `brick` (behind a barrier)
template <typename T>
QDAS_FD_HD void record(const Params<T> &P, const T *p, int brick, int64_t n, int v, int t) {
    const int e = P.sen_start[brick + 1];
    for (int q = P.sen_start[brick] + t; q < e; q += LANES) {
        const int j = P.sen_list[q];
        P.rec[n * P.rec_st + (int64_t)j * P.rec_sn + (int64_t)v * P.rec_sv] = p[node_offset(P, P.sen_node[j])];
    }
}

inline int64_t bricks_z(int64_t Nz) { return (Nz + TZ - 1) / TZ; }
inline int64_t bricks_x(int64_t Nx) { return (Nx + TX - 1) / TX; }
inline int64_t bricks_y(int64_t Ny) { return (Ny + TY - 1) / TY; }

// the per-brick lists of n points at `node` ((k Nx + j) Nz + i): start[0 .. bricks] and list[0 .. n), points of a brick in ascending index (a counting
// sort).  Returns -1 - q when node q lies outside the grid, else 0.  Brick (bz, bx, by) has the number (by nbx + bx) nbz + bz.
inline int64_t brick_lists(int64_t Nz, int64_t Nx, int64_t Ny, int64_t n, const int32_t *node, int32_t *start, int32_t *list) {
    const int64_t nbz = bricks_z(Nz), nbx = bricks_x(Nx), nb = nbz * nbx * bricks_y(Ny);
    for (int64_t q = 0; q < n; ++q)
        if (node[q] < 0 || (int64_t)node[q] >= Nz * Nx * Ny) return -1 - q;
    for (int64_t b = 0; b <= nb; ++b) start[b] = 0;
    auto brick_of = [&](int64_t q) {
        const int64_t i = (int64_t)node[q] % Nz, jk = (int64_t)node[q] / Nz;
        return ((jk / Nx / TY) * nbx + (jk % Nx) / TX) * nbz + i / TZ;
    };
    for (int64_t q = 0; q < n; ++q) ++start[brick_of(q) + 1];
    for (int64_t b = 0; b < nb; ++b) start[b + 1] += start[b];
    std::vector<int32_t> cur(start, start + nb);
    for (int64_t q = 0; q < n; ++q) list[cur[brick_of(q)]++] = (int32_t)q;
    return 0;
}

}  // namespace fd3
}  // namespace qdas
