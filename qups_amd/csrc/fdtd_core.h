// fdtd_core.h -- the per-cell arithmetic and the per-lane loops of fdtd.hip: the staggered derivative sums of order 2R, the two PML updates, the staging of
// a tile with its halo, the source injection, the sensor record and the per-tile point lists.  Plain C++ with no HIP in it: the same text compiles for the
// host, where tests/fdtd_core_host.cpp walks the tiles lane by lane on the CPU under the sanitizers (every LDS block a heap block of exactly its size).
//
// THE SCHEME (include/qdas.h states it in full).  Nz x Nx nodes, z fastest; p, rz, rx at (i, j), uz at (i + 1/2, j), ux at (i, j + 1/2):
//   D+f[i] = (1/h) sum_{k=1..R} a_k (f[i+k] - f[i-k+1])       valued at i + 1/2
//   D-g[i] = (1/h) sum_{k=1..R} a_k (g[i+k-1] - g[i-k])       valued at i
// with anything outside the array read as 0.  One step n:
//   1. uz <- azs (azs uz - dtrz D+z p),  ux <- axs (axs ux - dtrx D+x p)            (dtrz = dt / rho_sgz, the PML factors per row / column)
//   2. uz[src] += wz s[n, m, v],  ux[src] += wx s[n, m, v]                            (wz = nz 2 c dt / h)
//   3. rz <- az (az rz - dt rho D-z uz),  rx <- ax (ax rx - dt rho D-x ux)
//   4. p = c2 (rz + rx)
//   5. rec[n, j, v] = p[sensor j]
// Steps 1-2 are the velocity pass, 3-5 the density pass.  With absorption (qdas_fdtd_lossy) step 4 is density_cells_lossy's; every other step is the same
// text (tests/fdtd_loss_core_host.cpp walks it).  With nonlinear propagation (qdas_fdtd_nonlinear) steps 3 and 4 are density_cells_nl's
// (tests/fdtd_nl_core_host.cpp).
//
// THE TILE.  A workgroup of LANES = 256 lanes owns TZ x TX = 64 x 16 nodes of one pulse: lane t has z offset t mod 64 (a wave is one contiguous row of 64) and
// the rows (t div 64) + 4 r, r = 0 .. 3.  The velocity pass stages p with a halo of R on every side ((TZ + 2R) x (TX + 2R) words); the density pass stages uz
// with a halo in z ((TZ + 2R) x TX) and ux with a halo in x (TZ x (TX + 2R)).  A staged element outside the grid is 0 and is never loaded.  Every node is
// updated by exactly one lane; the sources and sensors of a tile are listed per tile (tile_lists), and the lanes of the tile that updated them inject and
// record them behind a barrier: no atomics, no flags.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define QDAS_FD_HD __host__ __device__ inline
#define QDAS_FD_UNROLL _Pragma("unroll")
#else
#define QDAS_FD_HD inline
#define QDAS_FD_UNROLL
#endif
// QDAS_FD_ROUNDED(x): x is a rounded value of its own from here on -- the device compiler may not fold the product that made it into a later sum as an FMA
// (an empty statement that claims to modify x; nothing on the host, which is built without contraction).  density_cells_lossy needs it: see there.
#if defined(__HIP_DEVICE_COMPILE__)
#define QDAS_FD_ROUNDED(x) asm volatile("" : "+v"(x))
#else
#define QDAS_FD_ROUNDED(x) ((void)0)
#endif

namespace qdas {
namespace fd {

constexpr int TZ = 64, TX = 16, LANES = 256, ROWS = LANES / TZ, PER_LANE = TX / ROWS;
constexpr int MAX_R = 4;

// the staggered-grid coefficients a_k, k = 1 .. R
template <int R, typename T>
QDAS_FD_HD T coef(int k) {
    if (R == 1) return T(1);
    if (R == 2) return k == 1 ? T(9.0 / 8.0) : T(-1.0 / 24.0);
    return k == 1 ? T(1225.0 / 1024.0) : k == 2 ? T(-245.0 / 3072.0) : k == 3 ? T(49.0 / 5120.0) : T(-5.0 / 7168.0);
}

// h D+f at i + 1/2: f points at element i, `st` is the stride of the direction
template <int R, typename T>
QDAS_FD_HD T dplus(const T *f, int st) {
    T d = T(0);
QDAS_FD_UNROLL
    for (int k = 1; k <= R; ++k) d += coef<R, T>(k) * (f[k * st] - f[(1 - k) * st]);
    return d;
}

// h D-g at i: g points at element i
template <int R, typename T>
QDAS_FD_HD T dminus(const T *g, int st) {
    T d = T(0);
QDAS_FD_UNROLL
    for (int k = 1; k <= R; ++k) d += coef<R, T>(k) * (g[(k - 1) * st] - g[-k * st]);
    return d;
}

// u <- a (a u - w d): both PML updates (w = dtr / h for a velocity, dt rho / h for a density)
template <typename T>
QDAS_FD_HD T pml_update(T u, T a, T w, T d) { return a * (a * u - w * d); }

template <typename T>
struct Params {
    T *p, *uz, *ux, *rz, *rx;                   // the five state arrays: element (i, j) of pulse v at v vs + j ld + i
    const T *c2, *rho, *dtrz, *dtrx;            // the medium, Nx x Nz dense (row stride Nz), shared by the pulses
    const T *az, *azs, *ax, *axs;               // the PML factors: Nz, Nz, Nx, Nx
    const T *s;                                 // the source table: s[(n M + m) V + v], n < Ts
    const T *src_wz, *src_wx;                   // per source: nz 2 c dt / h, nx 2 c dt / h
    const int32_t *src_node, *src_start, *src_list;   // node j Nz + i of source m; tile t owns src_list[src_start[t] .. src_start[t + 1])
    const int32_t *sen_node, *sen_start, *sen_list;
    T *rec;                                     // rec[n rec_st + j rec_sn + v rec_sv]
    int64_t vs, ld;
    int64_t rec_st, rec_sn, rec_sv;
    int32_t Nz, Nx, ntz, ntx, M, V, N;
    T inv_h, dt_h;                              // 1 / h, dt / h
};

constexpr int lds_words_vel(int R) { return (TZ + 2 * R) * (TX + 2 * R); }
constexpr int lds_words_den(int R) { return (TZ + 2 * R) * TX + TZ * (TX + 2 * R); }

// one lane's share of staging the tile at (i0, j0) with halos (hz, hx): element (a, b) of the block is node (i0 - hz + a, j0 - hx + b), 0 outside the grid
template <typename T>
QDAS_FD_HD void stage(T *lds, const T *src, int i0, int j0, int hz, int hx, int Nz, int Nx, int64_t ld, int t) {
    const int W = TZ + 2 * hz, H = TX + 2 * hx, l = t % TZ;
    for (int b = t / TZ; b < H; b += ROWS) {            // a wave per row: 64 consecutive z, then the 2 hz that remain (no division by W)
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

// step 1 for the nodes of lane t (lds: p with a halo of R on every side); uz, ux: the pulse's arrays
template <int R, typename T>
QDAS_FD_HD void velocity_cells(const Params<T> &P, const T *lds, T *uz, T *ux, int i0, int j0, int t) {
    constexpr int W = TZ + 2 * R;
    const int tz = t % TZ, i = i0 + tz;
    if (i >= P.Nz) return;
    const T a = P.azs[i];
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int jl = t / TZ + r * ROWS, j = j0 + jl;
        if (j >= P.Nx) break;
        const T *pc = lds + (jl + R) * W + (tz + R);
        const int64_t o = (int64_t)j * P.ld + i, m = (int64_t)j * P.Nz + i;
        const T b = P.axs[j];
        uz[o] = pml_update(uz[o], a, P.dtrz[m] * P.inv_h, dplus<R, T>(pc, 1));
        ux[o] = pml_update(ux[o], b, P.dtrx[m] * P.inv_h, dplus<R, T>(pc, W));
    }
}

// step 2 for the sources of `tile` (behind a barrier: the lanes that updated these nodes belong to this workgroup)
template <typename T>
QDAS_FD_HD void inject(const Params<T> &P, T *uz, T *ux, int tile, int64_t n, int v, int t) {
    const int e = P.src_start[tile + 1];
    for (int k = P.src_start[tile] + t; k < e; k += LANES) {
        const int m = P.src_list[k];
        const int node = P.src_node[m];
        const int64_t o = (int64_t)(node / P.Nz) * P.ld + node % P.Nz;
        const T sv = P.s[((int64_t)n * P.M + m) * P.V + v];
        uz[o] += P.src_wz[m] * sv;
        ux[o] += P.src_wx[m] * sv;
    }
}

// steps 3 and 4 for the nodes of lane t (lz: uz with a halo in z, lx: ux with a halo in x)
template <int R, typename T>
QDAS_FD_HD void density_cells(const Params<T> &P, const T *lz, const T *lx, T *rz, T *rx, T *p, int i0, int j0, int t) {
    constexpr int W = TZ + 2 * R;
    const int tz = t % TZ, i = i0 + tz;
    if (i >= P.Nz) return;
    const T a = P.az[i];
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int jl = t / TZ + r * ROWS, j = j0 + jl;
        if (j >= P.Nx) break;
        const int64_t o = (int64_t)j * P.ld + i, m = (int64_t)j * P.Nz + i;
        const T b = P.ax[j], w = P.dt_h * P.rho[m];
        const T vz = pml_update(rz[o], a, w, dminus<R, T>(lz + jl * W + (tz + R), 1));
        const T vx = pml_update(rx[o], b, w, dminus<R, T>(lx + (jl + R) * TZ + tz, TZ));
        rz[o] = vz;
        rx[o] = vx;
        p[o] = P.c2[m] * (vz + vx);
    }
}

// the loss block of qdas_fdtd_lossy: `kap` is Nx x Nz dense like the medium maps (2 c a under relaxation, mud = 2 c a / dt under Stokes); mechanism l of
// pulse v keeps its memory variable at e + (v L + l) vs, laid out like a state array
template <typename T>
struct Loss {
    const T *kap;
    T *e;
    T g[4], E[4];
};

// THE ROUNDINGS OF THE LOSSY PASS are written out, not left to the compiler.  Built with contraction, the lossless density kernels round steps 3 and 4 in
// one definite way (read from their code objects):
//   d  = fma(a_R, g_R, ... fma(a_1, g_1, 0))                     the derivative sum, every product fused into it
//   v  = A * fma(A, r, -(w * d))                                  w d and A (...) are products of their own
//   rz + rx = vz + vx in float, fma(az, fma(az, rz, -(w dz)), vx) in double
// and a second kernel with more arithmetic behind the same text is free to fuse differently (it did).  With a zero loss map the lossy pass must give the BITS
// of the lossless one (tests/test_gpu_fdtd_loss.py), so it states these roundings with explicit fused operations and QDAS_FD_ROUNDED, and the compiler has
// no choice left.  On the host the same text gives the same values.
// (a host build with QDAS_FD_UNFUSED and without contraction rounds every product: the arithmetic of the numpy restatements, operation for operation;
// tests/fdtd_nl_core_host.cpp compares bits with it)
#if defined(QDAS_FD_UNFUSED) && !defined(__HIPCC__)
QDAS_FD_HD float fused(float a, float b, float c) { return a * b + c; }
QDAS_FD_HD double fused(double a, double b, double c) { return a * b + c; }
#else
QDAS_FD_HD float fused(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
QDAS_FD_HD double fused(double a, double b, double c) { return __builtin_fma(a, b, c); }
#endif

template <int R, typename T>
QDAS_FD_HD T dminus_fused(const T *g, int st) {
    T d = T(0);
QDAS_FD_UNROLL
    for (int k = 1; k <= R; ++k) d = fused(coef<R, T>(k), g[(k - 1) * st] - g[-k * st], d);
    return d;
}

// steps 3 and 4 with absorption for the nodes of lane t; e: the pulse's first memory variable (unused for L = 0).  rn = rz + rx (the new ones), then
//   L = 0 (Stokes):      p = c2 (rn + mud (rn - ro)),                      ro = rz + rx before the update
//   L > 0 (relaxation):  e_l <- e_l + E_l (rn - e_l),  p = c2 (rn + kap sum_l g_l (rn - e_l))
// and p = c2 rn where the map is 0.  The memory variables are updated at every node, lossy or not.
template <int R, typename T, int L>
QDAS_FD_HD void density_cells_lossy(const Params<T> &P, const Loss<T> &Q, const T *lz, const T *lx, T *rz, T *rx, T *p, T *e, int i0, int j0, int t) {
    constexpr int W = TZ + 2 * R;
    const int tz = t % TZ, i = i0 + tz;
    if (i >= P.Nz) return;
    const T a = P.az[i];
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int jl = t / TZ + r * ROWS, j = j0 + jl;
        if (j >= P.Nx) break;
        const int64_t o = (int64_t)j * P.ld + i, m = (int64_t)j * P.Nz + i;
        const T b = P.ax[j], w = P.dt_h * P.rho[m];
        const T oz = rz[o], ox = rx[o];
        T wdz = w * dminus_fused<R, T>(lz + jl * W + (tz + R), 1), wdx = w * dminus_fused<R, T>(lx + (jl + R) * TZ + tz, TZ);
        QDAS_FD_ROUNDED(wdz);
        QDAS_FD_ROUNDED(wdx);
        const T iz = fused(a, oz, -wdz), ix = fused(b, ox, -wdx);
        T vz = a * iz, vx = b * ix;
        QDAS_FD_ROUNDED(vz);
        QDAS_FD_ROUNDED(vx);
        rz[o] = vz;
        rx[o] = vx;
        T rn = sizeof(T) == 4 ? vz + vx : fused(a, iz, vx);
        QDAS_FD_ROUNDED(rn);
        T acc;
        if (L == 0) {
            acc = rn - (oz + ox);
        } else {
            acc = T(0);
QDAS_FD_UNROLL
            for (int l = 0; l < L; ++l) {
                T *el = e + (int64_t)l * P.vs + o;
                const T en = *el + Q.E[l] * (rn - *el);
                *el = en;
                acc += Q.g[l] * (rn - en);
            }
        }
        const T k = Q.kap[m];
        p[o] = P.c2[m] * (k != T(0) ? rn + k * acc : rn);      // a node without loss is step 4 itself, the sign of a zero included
    }
}

// the nonlinear block of qdas_fdtd_nonlinear: `bq` = BoA / (2 rho) is Nx x Nz dense like the medium maps, K the weight of the convective term (2, or 0 when
// it is switched off)
template <typename T>
struct Nl {
    const T *bq;
    T K;
};

// steps 3' and 4' (nonlinear propagation, with or without absorption) for the nodes of lane t.  ro = rz + rx before the update, rn after it:
//   3'. r_a <- A_a (A_a r_a - (dt / h) (rho + K ro) h D-_a u_a)
//   4'. p = c2 (rn + [the absorption term of density_cells_lossy] + bq rn^2)
// Q.kap == nullptr: no absorption (L = 0).  THE ROUNDINGS are density_cells_lossy's, stated again, so that K = 0 with a zero bq map gives the bits of
// density_cells (no loss block) and of density_cells_lossy (with one):
//   * rho + K ro is ONE rounding, fused(K, ro, rho): rho itself for K = 0 (rho + 0 ro);
//   * the absorption term is written with the fused operations the contracting compiler chose for density_cells_lossy (read from its code objects):
//     e_l + E_l (rn - e_l) = fused(E_l, rn - e_l, e_l); the sum over l from acc = 0 is fused(g_l, rn - e_l, acc) in double and for l = 0, but in float the
//     products g_l (rn - e_l), l >= 1, are rounded on their own (that compiler packs them in pairs); rn + kap acc = fused(kap, acc, rn);
//   * rn^2 is a product of its own, then fused(bq, rn^2, .); a node with bq = 0 takes the linear value itself, as a node with kap = 0 takes rn.
template <int R, typename T, int L>
QDAS_FD_HD void density_cells_nl(const Params<T> &P, const Loss<T> &Q, const Nl<T> &N, const T *lz, const T *lx, T *rz, T *rx, T *p, T *e, int i0, int j0,
                                 int t) {
    constexpr int W = TZ + 2 * R;
    const int tz = t % TZ, i = i0 + tz;
    if (i >= P.Nz) return;
    const T a = P.az[i];
QDAS_FD_UNROLL
    for (int r = 0; r < PER_LANE; ++r) {
        const int jl = t / TZ + r * ROWS, j = j0 + jl;
        if (j >= P.Nx) break;
        const int64_t o = (int64_t)j * P.ld + i, m = (int64_t)j * P.Nz + i;
        const T oz = rz[o], ox = rx[o];
        T ro = oz + ox;
        QDAS_FD_ROUNDED(ro);
        T re = fused(N.K, ro, P.rho[m]);
        QDAS_FD_ROUNDED(re);
        const T b = P.ax[j], w = P.dt_h * re;
        T wdz = w * dminus_fused<R, T>(lz + jl * W + (tz + R), 1), wdx = w * dminus_fused<R, T>(lx + (jl + R) * TZ + tz, TZ);
        QDAS_FD_ROUNDED(wdz);
        QDAS_FD_ROUNDED(wdx);
        const T iz = fused(a, oz, -wdz), ix = fused(b, ox, -wdx);
        T vz = a * iz, vx = b * ix;
        QDAS_FD_ROUNDED(vz);
        QDAS_FD_ROUNDED(vx);
        rz[o] = vz;
        rx[o] = vx;
        T rn = sizeof(T) == 4 ? vz + vx : fused(a, iz, vx);
        QDAS_FD_ROUNDED(rn);
        T lin = rn;
        if (L > 0 || Q.kap != nullptr) {                          // (uniform)
            T acc;
            if (L == 0) {
                acc = rn - ro;
            } else {
                acc = T(0);
QDAS_FD_UNROLL
                for (int l = 0; l < L; ++l) {
                    T *el = e + (int64_t)l * P.vs + o;
                    const T eo = *el;
                    T en = fused(Q.E[l], rn - eo, eo);
                    QDAS_FD_ROUNDED(en);
                    *el = en;
                    T gd = rn - en;
                    QDAS_FD_ROUNDED(gd);
                    if (sizeof(T) == 4 && l > 0) {
                        T pr = Q.g[l] * gd;
                        QDAS_FD_ROUNDED(pr);
                        acc += pr;
                    } else {
                        acc = fused(Q.g[l], gd, acc);
                    }
                    QDAS_FD_ROUNDED(acc);
                }
            }
            const T k = Q.kap[m];
            if (k != T(0)) lin = fused(k, acc, rn);
        }
        const T q = N.bq[m];
        T r2 = rn * rn;
        QDAS_FD_ROUNDED(r2);
        p[o] = P.c2[m] * (q != T(0) ? fused(q, r2, lin) : lin);
    }
}

// step 5 for the sensors of `tile` (behind a barrier)
template <typename T>
QDAS_FD_HD void record(const Params<T> &P, const T *p, int tile, int64_t n, int v, int t) {
    const int e = P.sen_start[tile + 1];
    for (int k = P.sen_start[tile] + t; k < e; k += LANES) {
        const int j = P.sen_list[k];
        const int node = P.sen_node[j];
        P.rec[n * P.rec_st + (int64_t)j * P.rec_sn + (int64_t)v * P.rec_sv] = p[(int64_t)(node / P.Nz) * P.ld + node % P.Nz];
    }
}

inline int64_t tiles_z(int64_t Nz) { return (Nz + TZ - 1) / TZ; }
inline int64_t tiles_x(int64_t Nx) { return (Nx + TX - 1) / TX; }

// the per-tile lists of n points at `node` (j Nz + i): start[0 .. ntiles] and list[0 .. n), points of a tile in ascending index (a counting sort).
// Returns -1 - k when node k lies outside the grid, else 0.  Tile (tz, tx) has the number tx ntz + tz.
inline int64_t tile_lists(int64_t Nz, int64_t Nx, int64_t n, const int32_t *node, int32_t *start, int32_t *list) {
    const int64_t ntz = tiles_z(Nz), nt = ntz * tiles_x(Nx);
    for (int64_t k = 0; k < n; ++k)
        if (node[k] < 0 || (int64_t)node[k] >= Nz * Nx) return -1 - k;
    for (int64_t t = 0; t <= nt; ++t) start[t] = 0;
    auto tile_of = [&](int64_t k) { return ((int64_t)node[k] / Nz / TX) * ntz + ((int64_t)node[k] % Nz) / TZ; };
    for (int64_t k = 0; k < n; ++k) ++start[tile_of(k) + 1];
    for (int64_t t = 0; t < nt; ++t) start[t + 1] += start[t];
    std::vector<int32_t> cur(start, start + nt);
    for (int64_t k = 0; k < n; ++k) list[cur[tile_of(k)]++] = (int32_t)k;
    return 0;
}

}  // namespace fd
}  // namespace qdas
