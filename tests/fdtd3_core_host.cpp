// fdtd3_core_host.cpp -- the per-lane loops of qups_amd/csrc/fdtd3_core.h walked on the CPU, brick by brick, plane by plane and lane by lane in the kernels'
// order, by a stand-alone program that tests/test_fdtd3_host.py builds with -fsanitize=address,undefined.  Every LDS block, every lane's window and every
// array is a heap block of exactly its size, so an index the kernels would send outside the brick, the grid, a table or the record is a sanitizer report here.
//
// usage: fdtd3_core_host in.bin out.bin.  in.bin: 14 int64 (dtype 0 = f64 | 1 = f32, R, Nz, Nx, Ny, V, Nt, ld, pstride, M, Ts, N, pad0, pad1), 2 doubles
// (dt / h, 1 / h), then doubles: c2, rho, dtrz, dtrx, dtry (Ny Nx Nz each), az, azs (Nz), ax, axs (Nx), ay, ays (Ny), s (Ts M V), wz, wx, wy (M), then int32:
// src_node (M), sen_node (N).  out.bin: doubles rec (Nt N V), then p, uz, ux, uy, rz, rx, ry (V Ny Nx Nz each, the padding dropped).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "fdtd3_core.h"

using namespace qdas::fd3;

static FILE *g_in;

static void need(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "fdtd3_core_host: %s\n", what); exit(2); }
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

template <int R, typename T>
static void walk(Params<T> &P, int64_t V, int64_t Nt, int64_t Ts) {
    const int nb = P.nbz * P.nbx * P.nby;
    for (int64_t n = 0; n < Nt; ++n) {
        for (int pass = 0; pass < 2; ++pass)
            for (int v = 0; v < (int)V; ++v)
                for (int brick = 0; brick < nb; ++brick) {
                    const int i0 = (brick % P.nbz) * TZ, j0 = (brick / P.nbz % P.nbx) * TX, k0 = (brick / P.nbz / P.nbx) * TY;
                    const int64_t off = (int64_t)v * P.vs;
                    std::vector<std::unique_ptr<Window<R, T>>> win(LANES);          // a heap block per lane
                    for (auto &w : win) w.reset(new Window<R, T>);
                    if (pass == 0) {
                        for (int t = 0; t < LANES; ++t) window_fill<R, T>(P, P.p + off, *win[t], i0, j0, k0 - R, t);
                        for (int k = k0; k < k0 + TY && k < P.Ny; ++k) {
                            std::unique_ptr<T[]> lds(new T[lds_words_vel(R)]);
                            for (int t = 0; t < LANES; ++t) window_slide<R, T>(P, P.p + off, *win[t], i0, j0, k + R, t);
                            for (int t = 0; t < LANES; ++t) stage(lds.get(), P.p + off + (int64_t)k * P.ps, i0, j0, R, R, P.Nz, P.Nx, P.ld, t);
                            for (int t = 0; t < LANES; ++t) velocity_cells<R, T>(P, lds.get(), *win[t], P.uz + off, P.ux + off, P.uy + off, i0, j0, k, t);
                        }
                        if (P.M > 0 && n < Ts && P.src_start[brick + 1] > P.src_start[brick])
                            for (int t = 0; t < LANES; ++t) inject(P, P.uz + off, P.ux + off, P.uy + off, brick, n, v, t);
                    } else {
                        for (int t = 0; t < LANES; ++t) window_fill<R, T>(P, P.uy + off, *win[t], i0, j0, k0 - R - 1, t);
                        for (int k = k0; k < k0 + TY && k < P.Ny; ++k) {
                            std::unique_ptr<T[]> lz(new T[(TZ + 2 * R) * TX]), lx(new T[TZ * (TX + 2 * R)]);
                            for (int t = 0; t < LANES; ++t) window_slide<R, T>(P, P.uy + off, *win[t], i0, j0, k + R - 1, t);
                            for (int t = 0; t < LANES; ++t) stage(lz.get(), P.uz + off + (int64_t)k * P.ps, i0, j0, R, 0, P.Nz, P.Nx, P.ld, t);
                            for (int t = 0; t < LANES; ++t) stage(lx.get(), P.ux + off + (int64_t)k * P.ps, i0, j0, 0, R, P.Nz, P.Nx, P.ld, t);
                            for (int t = 0; t < LANES; ++t)
                                density_cells<R, T>(P, lz.get(), lx.get(), *win[t], P.rz + off, P.rx + off, P.ry + off, P.p + off, i0, j0, k, t);
                        }
                        if (P.N > 0 && P.sen_start[brick + 1] > P.sen_start[brick])
                            for (int t = 0; t < LANES; ++t) record(P, P.p + off, brick, n, v, t);
                    }
                }
    }
}

template <typename T>
static int run(const int64_t *hd, double dt_h, double inv_h, const char *out_path) {
    const int64_t R = hd[1], Nz = hd[2], Nx = hd[3], Ny = hd[4], V = hd[5], Nt = hd[6], ld = hd[7], ps = hd[8], M = hd[9], Ts = hd[10], N = hd[11];
    need(Nz > 0 && Nx > 0 && Ny > 0 && ld >= Nz && ps >= Nx * ld && V >= 0 && Nt >= 0 && M >= 0 && N >= 0 && Ts >= 0, "bad header");
    const size_t cells = (size_t)(Ny * Nx * Nz);
    auto c2 = read_as<T>(cells), rho = read_as<T>(cells), dtrz = read_as<T>(cells), dtrx = read_as<T>(cells), dtry = read_as<T>(cells);
    auto az = read_as<T>(Nz), azs = read_as<T>(Nz), ax = read_as<T>(Nx), axs = read_as<T>(Nx), ay = read_as<T>(Ny), ays = read_as<T>(Ny);
    auto s = read_as<T>((size_t)(Ts * M * V)), wz = read_as<T>(M), wx = read_as<T>(M), wy = read_as<T>(M);
    auto src_node = read_i32(M), sen_node = read_i32(N);
    const int64_t nbz = bricks_z(Nz), nbx = bricks_x(Nx), nb = nbz * nbx * bricks_y(Ny);
    std::unique_ptr<int32_t[]> src_start(new int32_t[nb + 1]), src_list(new int32_t[M]), sen_start(new int32_t[nb + 1]), sen_list(new int32_t[N]);
    need(brick_lists(Nz, Nx, Ny, M, src_node.get(), src_start.get(), src_list.get()) == 0, "a source outside the grid");
    need(brick_lists(Nz, Nx, Ny, N, sen_node.get(), sen_start.get(), sen_list.get()) == 0, "a sensor outside the grid");
    // every point in exactly one brick, and that brick holds its node: sources and sensors alike
    for (int which = 0; which < 2; ++which) {
        const int64_t n = which ? N : M;
        const int32_t *node = which ? sen_node.get() : src_node.get(), *start = which ? sen_start.get() : src_start.get(), *list = which ? sen_list.get() : src_list.get();
        std::vector<int> seen(n, 0);
        for (int64_t b = 0; b < nb; ++b)
            for (int q = start[b]; q < start[b + 1]; ++q) {
                const int m = list[q];
                need(m >= 0 && m < n, "a list entry that is no point");
                ++seen[m];
                const int64_t i = node[m] % Nz, j = node[m] / Nz % Nx, k = node[m] / Nz / Nx;
                need(i / TZ == b % nbz && j / TX == b / nbz % nbx && k / TY == b / nbz / nbx, which ? "a sensor in the wrong brick" : "a source in the wrong brick");
            }
        for (int64_t m = 0; m < n; ++m) need(seen[m] == 1, which ? "a sensor not in exactly one brick" : "a source not in exactly one brick");
    }
    const int64_t vs = Ny * ps;
    const size_t span = V ? (size_t)((V - 1) * vs + (Ny - 1) * ps + (Nx - 1) * ld + Nz) : 0;      // exactly what the kernels may address
    std::unique_ptr<T[]> st[7];
    for (auto &a : st) {
        a.reset(new T[span]);
        for (size_t k = 0; k < span; ++k) a[k] = T(0);
    }
    std::unique_ptr<T[]> rec(new T[(size_t)(Nt * N * V)]);
    for (size_t k = 0; k < (size_t)(Nt * N * V); ++k) rec[k] = T(-777);
    Params<T> P{};
    P.p = st[0].get(); P.uz = st[1].get(); P.ux = st[2].get(); P.uy = st[3].get(); P.rz = st[4].get(); P.rx = st[5].get(); P.ry = st[6].get();
    P.c2 = c2.get(); P.rho = rho.get(); P.dtrz = dtrz.get(); P.dtrx = dtrx.get(); P.dtry = dtry.get();
    P.az = az.get(); P.azs = azs.get(); P.ax = ax.get(); P.axs = axs.get(); P.ay = ay.get(); P.ays = ays.get();
    P.s = s.get(); P.src_wz = wz.get(); P.src_wx = wx.get(); P.src_wy = wy.get();
    P.src_node = src_node.get(); P.src_start = src_start.get(); P.src_list = src_list.get();
    P.sen_node = sen_node.get(); P.sen_start = sen_start.get(); P.sen_list = sen_list.get();
    P.rec = rec.get();
    P.vs = vs; P.ps = ps; P.ld = ld; P.rec_st = N * V; P.rec_sn = V; P.rec_sv = 1;
    P.Nz = (int32_t)Nz; P.Nx = (int32_t)Nx; P.Ny = (int32_t)Ny; P.nbz = (int32_t)nbz; P.nbx = (int32_t)nbx; P.nby = (int32_t)bricks_y(Ny);
    P.M = Ts > 0 ? (int32_t)M : 0; P.V = (int32_t)V; P.N = (int32_t)N;
    P.inv_h = (T)inv_h; P.dt_h = (T)dt_h;
    if (R == 1) walk<1, T>(P, V, Nt, Ts);
    else if (R == 2) walk<2, T>(P, V, Nt, Ts);
    else if (R == 4) walk<4, T>(P, V, Nt, Ts);
    else need(false, "R is 1, 2 or 4");
    FILE *f = fopen(out_path, "wb");
    need(f != nullptr, "cannot write");
    std::vector<double> buf;
    for (size_t k = 0; k < (size_t)(Nt * N * V); ++k) buf.push_back((double)rec[k]);
    for (auto &a : st)
        for (int64_t v = 0; v < V; ++v)
            for (int64_t k = 0; k < Ny; ++k)
                for (int64_t j = 0; j < Nx; ++j)
                    for (int64_t i = 0; i < Nz; ++i) buf.push_back((double)a[(size_t)(v * vs + k * ps + j * ld + i)]);
    need(fwrite(buf.data(), sizeof(double), buf.size(), f) == buf.size(), "short write");
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    need(argc == 3, "usage: fdtd3_core_host in.bin out.bin");
    g_in = fopen(argv[1], "rb");
    need(g_in != nullptr, "cannot read");
    int64_t hd[14];
    double sc[2];
    need(fread(hd, sizeof(int64_t), 14, g_in) == 14 && fread(sc, sizeof(double), 2, g_in) == 2, "short header");
    const int rc = hd[0] == 1 ? run<float>(hd, sc[0], sc[1], argv[2]) : run<double>(hd, sc[0], sc[1], argv[2]);
    fclose(g_in);
    return rc;
}
