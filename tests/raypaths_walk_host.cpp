// raypaths_walk_host.cpp -- runs the walk of qups_amd/csrc/raypaths_walk.h (the text the device kernels compile) on the CPU: TEST INFRASTRUCTURE, built by
// tests/test_raypaths_host.py with g++ (and the host sanitizers: every grid read of the walk is a read of a heap array of exactly X or Z values here).
// Input (a text file, argv[1]): "bits X Z J", the X and Z grid values, then J lines "ax az bx bz" (nan / inf are read as such).  Output: per ray one line
// "slots used-steps" followed by the X * Z dense sums W[ix][iz], %.17g.  The program itself checks what the kernels rely on: at most K slots, every index
// inside the grid, no negative or non-finite weight; with ALL = true exactly K slots.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "raypaths_walk.h"

template <typename R> static int run(FILE *f, int X, int Z, int J) {
    std::vector<double> gx(X), gz(Z);
    for (auto &v : gx) if (fscanf(f, "%lf", &v) != 1) return 2;
    for (auto &v : gz) if (fscanf(f, "%lf", &v) != 1) return 2;
    // as the kernels do: the grid in the data's precision, less its first value
    R *xs = new R[X], *zs = new R[Z];
    const R x0 = (R)gx[0], z0 = (R)gz[0];
    for (int i = 0; i < X; ++i) xs[i] = (R)gx[i] - x0;
    for (int i = 0; i < Z; ++i) zs[i] = (R)gz[i] - z0;
    const int K = X + Z + 1;
    std::vector<double> W((size_t)X * Z);
    for (int j = 0; j < J; ++j) {
        double e[4];
        for (double &v : e) if (fscanf(f, "%lf", &v) != 1) return 2;
        const R ax = (R)e[0] - x0, az = (R)e[1] - z0, bx = (R)e[2] - x0, bz = (R)e[3] - z0;
        int bad = 0, nall = 0, nsome = 0, used = 0;
        W.assign(W.size(), 0.0);
        qdas::rayp::walk<R, true>(xs, zs, X, Z, ax, az, bx, bz, [&](int s, bool emit, int cx, int cz, R w00, R w10, R w01, R w11) {
            if (s != nall || s >= K) bad |= 1;
            ++nall;
            const R w[4] = {w00, w10, w01, w11};
            for (int c = 0; c < 4; ++c) if (!(w[c] >= R(0)) || !(w[c] - w[c] == R(0))) bad |= 2;
            if (!emit) { for (int c = 0; c < 4; ++c) if (w[c] != R(0)) bad |= 4; return; }
            if (cx < 0 || cx > X - 2 || cz < 0 || cz > Z - 2) { bad |= 8; return; }
            ++used;
            for (int c = 0; c < 4; ++c) W[(size_t)(cx + (c & 1)) * Z + cz + (c >> 1)] += (double)w[c];
        });
        double sum_some = 0, sum_all = 0;
        qdas::rayp::walk<R, false>(xs, zs, X, Z, ax, az, bx, bz, [&](int s, bool emit, int, int, R w00, R w10, R w01, R w11) {
            if (s != nsome || s >= K) bad |= 16;
            ++nsome;
            if (emit) sum_some += (double)w00 + (double)w10 + (double)w01 + (double)w11;
        });
        for (double v : W) sum_all += v;
        if (nall != K) bad |= 32;
        if (!(sum_some - sum_all <= 1e-6 * sum_all + 1e-300 && sum_all - sum_some <= 1e-6 * sum_all + 1e-300)) bad |= 64;   // the two modes walk the same path
        if (bad) { fprintf(stderr, "ray %d: walk broke its contract, flags %d\n", j, bad); return 1; }
        printf("%d %d", nsome, used);
        for (double v : W) printf(" %.17g", v);
        printf("\n");
    }
    delete[] xs;
    delete[] zs;
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    int bits, X, Z, J;
    if (!f || fscanf(f, "%d %d %d %d", &bits, &X, &Z, &J) != 4 || X < 2 || Z < 2) return 2;
    const int rc = bits == 32 ? run<float>(f, X, Z, J) : run<double>(f, X, Z, J);
    fclose(f);
    return rc;
}
