// fdtd_nl_core_host.cpp -- the per-lane loops of qdas_fdtd_nonlinear (qups_amd/csrc/fdtd_core.h: the velocity pass and density_cells_nl) walked on the CPU,
// tile by tile and lane by lane in the kernels' order, by a stand-alone program that tests/test_fdtd_nl_host.py builds with -fsanitize=address,undefined.
// Every LDS block and every array -- the memory variables, the loss map and the map bq among them -- is a heap block of exactly its size, so an index the
// kernels would send outside the tile, the grid, a table, the record or the V L arrays of e is a sanitizer report here.  Built with -DQDAS_FD_UNFUSED (every
// fused operation of the core two roundings) and without contraction, the walk does the arithmetic of tests/fdtd_nl_ref.py operation for operation: the
// results must be the restatement's bits.
//
// usage: fdtd_nl_core_host in.bin out.bin.  in.bin: 12 int64 (dtype 0 = f64 | 1 = f32, R, Nz, Nx, V, Nt, ld, M, Ts, N, L, loss block given 1 | 0), 3 doubles
// (dt / h, 1 / h, K), then doubles: c2, rho, dtrz, dtrx, kap, bq (Nx Nz each; kap is read but unused without a loss block), az, azs (Nz), ax, axs (Nx), g,
// E (L), s (Ts M V), wz, wx (M), then int32: src_node (M), sen_node (N).  L = 0 is the Stokes term, or no absorption.  out.bin: doubles rec (Nt N V), then
// p, uz, ux, rz, rx (V Nx Nz each, the row padding dropped), then e (V L Nx Nz).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "fdtd_core.h"

using namespace qdas::fd;

static FILE *g_in;

static void need(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "fdtd_nl_core_host: %s\n", what); exit(2); }
}

template <typename T>
static std::unique_ptr<T[]> read_as(size_t n) {
    std::unique_ptr<T[]> out(new T[n]);          // exactly n elements
    std::vector<double> tmp(n);
    need(fread(tmp.data(), sizeof(double), n, g_in) == n, "short input");
    for (size_t k = 0; k < n; ++k) out[k] = (T)tmp[k];
    return out;
}

static std::unique_ptr<int32_t[]> read_i32(size_t n) {
    std::unique_ptr<int32_t[]> out(new int32_t[n]);
    need(fread(out.get(), sizeof(int32_t), n, g_in) == n, "short input");
    return out;
}

template <int R, typename T, int L>
static void walk(Params<T> &P, const Loss<T> &Q, const Nl<T> &NL, int64_t V, int64_t Nt, int64_t Ts) {
    const int nt = P.ntz * P.ntx;
    for (int64_t n = 0; n < Nt; ++n) {
        for (int pass = 0; pass < 2; ++pass)
            for (int v = 0; v < (int)V; ++v)
                for (int tile = 0; tile < nt; ++tile) {
                    const int i0 = (tile % P.ntz) * TZ, j0 = (tile / P.ntz) * TX;
                    const int64_t off = (int64_t)v * P.vs;
                    if (pass == 0) {
                        std::unique_ptr<T[]> lds(new T[lds_words_vel(R)]);
                        for (int t = 0; t < LANES; ++t) stage(lds.get(), P.p + off, i0, j0, R, R, P.Nz, P.Nx, P.ld, t);
                        for (int t = 0; t < LANES; ++t) velocity_cells<R, T>(P, lds.get(), P.uz + off, P.ux + off, i0, j0, t);
                        if (P.M > 0 && n < Ts && P.src_start[tile + 1] > P.src_start[tile])
                            for (int t = 0; t < LANES; ++t) inject(P, P.uz + off, P.ux + off, tile, n, v, t);
                    } else {
                        std::unique_ptr<T[]> lz(new T[(TZ + 2 * R) * TX]), lx(new T[TZ * (TX + 2 * R)]);
                        for (int t = 0; t < LANES; ++t) stage(lz.get(), P.uz + off, i0, j0, R, 0, P.Nz, P.Nx, P.ld, t);
                        for (int t = 0; t < LANES; ++t) stage(lx.get(), P.ux + off, i0, j0, 0, R, P.Nz, P.Nx, P.ld, t);
                        for (int t = 0; t < LANES; ++t)
                            density_cells_nl<R, T, L>(P, Q, NL, lz.get(), lx.get(), P.rz + off, P.rx + off, P.p + off, L > 0 ? Q.e + off * L : nullptr, i0, j0, t);
                        if (P.N > 0 && P.sen_start[tile + 1] > P.sen_start[tile])
                            for (int t = 0; t < LANES; ++t) record(P, P.p + off, tile, n, v, t);
                    }
                }
    }
}

template <int R, typename T>
static void walk_mechanisms(Params<T> &P, const Loss<T> &Q, const Nl<T> &NL, int64_t L, int64_t V, int64_t Nt, int64_t Ts) {
    if (L == 0) walk<R, T, 0>(P, Q, NL, V, Nt, Ts);
    else if (L == 1) walk<R, T, 1>(P, Q, NL, V, Nt, Ts);
    else if (L == 2) walk<R, T, 2>(P, Q, NL, V, Nt, Ts);
    else if (L == 3) walk<R, T, 3>(P, Q, NL, V, Nt, Ts);
    else walk<R, T, 4>(P, Q, NL, V, Nt, Ts);
}

template <typename T>
static int run(const int64_t *hd, double dt_h, double inv_h, double K, const char *out_path) {
    const int64_t R = hd[1], Nz = hd[2], Nx = hd[3], V = hd[4], Nt = hd[5], ld = hd[6], M = hd[7], Ts = hd[8], N = hd[9], L = hd[10], lossy = hd[11];
    need(L >= 0 && L <= 4 && (lossy || L == 0), "L is 0 .. 4, and 0 without a loss block");
    need(Nz > 0 && Nx > 0 && ld >= Nz && V >= 0 && Nt >= 0 && M >= 0 && N >= 0 && Ts >= 0, "bad header");
    const size_t cells = (size_t)(Nx * Nz);
    auto c2 = read_as<T>(cells), rho = read_as<T>(cells), dtrz = read_as<T>(cells), dtrx = read_as<T>(cells), kap = read_as<T>(cells), bq = read_as<T>(cells);
    auto az = read_as<T>(Nz), azs = read_as<T>(Nz), ax = read_as<T>(Nx), axs = read_as<T>(Nx);
    auto g = read_as<T>(L), E = read_as<T>(L);
    auto s = read_as<T>((size_t)(Ts * M * V)), wz = read_as<T>(M), wx = read_as<T>(M);
    auto src_node = read_i32(M), sen_node = read_i32(N);
    const int64_t nt = tiles_z(Nz) * tiles_x(Nx);
    std::unique_ptr<int32_t[]> src_start(new int32_t[nt + 1]), src_list(new int32_t[M]), sen_start(new int32_t[nt + 1]), sen_list(new int32_t[N]);
    need(tile_lists(Nz, Nx, M, src_node.get(), src_start.get(), src_list.get()) == 0, "a source outside the grid");
    need(tile_lists(Nz, Nx, N, sen_node.get(), sen_start.get(), sen_list.get()) == 0, "a sensor outside the grid");
    // every point in exactly one tile, and that tile holds its node: sources and sensors alike
    for (int which = 0; which < 2; ++which) {
        const int64_t n = which ? N : M;
        const int32_t *node = which ? sen_node.get() : src_node.get(), *start = which ? sen_start.get() : src_start.get(), *list = which ? sen_list.get() : src_list.get();
        std::vector<int> seen(n, 0);
        for (int64_t t = 0; t < nt; ++t)
            for (int k = start[t]; k < start[t + 1]; ++k) {
                const int m = list[k];
                need(m >= 0 && m < n, "a list entry that is no point");
                ++seen[m];
                need((node[m] % Nz) / TZ == t % tiles_z(Nz) && (node[m] / Nz) / TX == t / tiles_z(Nz), which ? "a sensor in the wrong tile" : "a source in the wrong tile");
            }
        for (int64_t m = 0; m < n; ++m) need(seen[m] == 1, which ? "a sensor not in exactly one tile" : "a source not in exactly one tile");
    }
    const int64_t vs = Nx * ld;
    const size_t span = V ? (size_t)((V - 1) * vs + (Nx - 1) * ld + Nz) : 0;      // exactly what the kernels may address
    std::unique_ptr<T[]> st[5];
    for (auto &a : st) {
        a.reset(new T[span]);
        for (size_t k = 0; k < span; ++k) a[k] = T(0);
    }
    const size_t espan = (V && L) ? (size_t)((V * L - 1) * vs + (Nx - 1) * ld + Nz) : 0;      // V L arrays of the states' layout, and not a word more
    std::unique_ptr<T[]> e(new T[espan]);
    for (size_t k = 0; k < espan; ++k) e[k] = T(0);
    std::unique_ptr<T[]> rec(new T[(size_t)(Nt * N * V)]);
    for (size_t k = 0; k < (size_t)(Nt * N * V); ++k) rec[k] = T(-777);
    Params<T> P{};
    P.p = st[0].get(); P.uz = st[1].get(); P.ux = st[2].get(); P.rz = st[3].get(); P.rx = st[4].get();
    P.c2 = c2.get(); P.rho = rho.get(); P.dtrz = dtrz.get(); P.dtrx = dtrx.get();
    P.az = az.get(); P.azs = azs.get(); P.ax = ax.get(); P.axs = axs.get();
    P.s = s.get(); P.src_wz = wz.get(); P.src_wx = wx.get();
    P.src_node = src_node.get(); P.src_start = src_start.get(); P.src_list = src_list.get();
    P.sen_node = sen_node.get(); P.sen_start = sen_start.get(); P.sen_list = sen_list.get();
    P.rec = rec.get();
    P.vs = vs; P.ld = ld; P.rec_st = N * V; P.rec_sn = V; P.rec_sv = 1;
    P.Nz = (int32_t)Nz; P.Nx = (int32_t)Nx; P.ntz = (int32_t)tiles_z(Nz); P.ntx = (int32_t)tiles_x(Nx);
    P.M = Ts > 0 ? (int32_t)M : 0; P.V = (int32_t)V; P.N = (int32_t)N;
    P.inv_h = (T)inv_h; P.dt_h = (T)dt_h;
    Loss<T> Q{};
    Q.kap = lossy ? kap.get() : nullptr; Q.e = e.get();
    for (int64_t k = 0; k < L; ++k) { Q.g[k] = g[k]; Q.E[k] = E[k]; }
    Nl<T> NL{};
    NL.bq = bq.get(); NL.K = (T)K;
    if (R == 1) walk_mechanisms<1, T>(P, Q, NL, L, V, Nt, Ts);
    else if (R == 2) walk_mechanisms<2, T>(P, Q, NL, L, V, Nt, Ts);
    else if (R == 4) walk_mechanisms<4, T>(P, Q, NL, L, V, Nt, Ts);
    else need(false, "R is 1, 2 or 4");
    FILE *f = fopen(out_path, "wb");
    need(f != nullptr, "cannot write");
    for (size_t k = 0; k < (size_t)(Nt * N * V); ++k) { const double d = (double)rec[k]; fwrite(&d, sizeof d, 1, f); }
    for (auto &a : st)
        for (int64_t v = 0; v < V; ++v)
            for (int64_t j = 0; j < Nx; ++j)
                for (int64_t i = 0; i < Nz; ++i) { const double d = (double)a[(size_t)(v * vs + j * ld + i)]; fwrite(&d, sizeof d, 1, f); }
    for (int64_t v = 0; v < V * L; ++v)
        for (int64_t j = 0; j < Nx; ++j)
            for (int64_t i = 0; i < Nz; ++i) { const double d = (double)e[(size_t)(v * vs + j * ld + i)]; fwrite(&d, sizeof d, 1, f); }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    need(argc == 3, "usage: fdtd_nl_core_host in.bin out.bin");
    g_in = fopen(argv[1], "rb");
    need(g_in != nullptr, "cannot read");
    int64_t hd[12];
    double sc[3];
    need(fread(hd, sizeof(int64_t), 12, g_in) == 12 && fread(sc, sizeof(double), 3, g_in) == 3, "short header");
    const int rc = hd[0] == 1 ? run<float>(hd, sc[0], sc[1], sc[2], argv[2]) : run<double>(hd, sc[0], sc[1], sc[2], argv[2]);
    fclose(g_in);
    return rc;
}
