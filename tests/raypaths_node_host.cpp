// raypaths_node_host.cpp -- runs the per-node weight of qups_amd/csrc/raypaths_node.h (the text the back-projection kernel compiles) on the CPU: TEST
// INFRASTRUCTURE, built by tests/test_raybackproject_host.py with g++ and the host sanitizers (every grid read is a read of a heap array of exactly X or Z
// values here).  Input (a text file, argv[1]): the format of tests/raypaths_walk_host.cpp -- "bits X Z J", the X and Z grid values, then J lines
// "ax az bx bz".  Output: per ray one line "tiles-hit" followed by the X * Z weights W[ix][iz], %.17g.  The program itself checks what the kernel relies on:
// no weight negative or non-finite, and on a sound grid (finite, increasing) a ray whose slab test misses a tile's grown box weighs no node of that tile.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "raypaths_node.h"

template <typename R> static int run(FILE *f, int X, int Z, int J) {
    using namespace qdas::rayp;
    std::vector<double> gx(X), gz(Z);
    for (auto &v : gx) if (fscanf(f, "%lf", &v) != 1) return 2;
    for (auto &v : gz) if (fscanf(f, "%lf", &v) != 1) return 2;
    std::vector<R> xv(gx.begin(), gx.end()), zv(gz.begin(), gz.end());     // as the kernel sees them: the data's precision, the first value still in
    const R *xg = xv.data(), *zg = zv.data();
    // the slab test promises nothing on a grid that breaks the caller's promise: there a weight may be dropped (never invented)
    bool sound = true;
    for (int i = 0; i < X; ++i) sound = sound && xg[i] - xg[i] == R(0) && (i == 0 || xg[i] > xg[i - 1]);
    for (int i = 0; i < Z; ++i) sound = sound && zg[i] - zg[i] == R(0) && (i == 0 || zg[i] > zg[i - 1]);
    std::vector<Node<R>> nodes((size_t)X * Z);
    for (int i = 0; i < X; ++i) for (int k = 0; k < Z; ++k) nodes[(size_t)i * Z + k] = make_node(xg, X, i, zg, Z, k);
    const int TX = (X + TILE - 1) / TILE, TZ = (Z + TILE - 1) / TILE;
    std::vector<double> W((size_t)X * Z);
    for (int j = 0; j < J; ++j) {
        double e[4];
        for (double &v : e) if (fscanf(f, "%lf", &v) != 1) return 2;
        const Ray<R> q = make_ray((R)e[0] - xg[0], (R)e[1] - zg[0], (R)e[2] - xg[0], (R)e[3] - zg[0]);
        int bad = 0, hit = 0;
        for (size_t n = 0; n < W.size(); ++n) {
            const R w = node_weight(nodes[n], q);
            if (!(w >= R(0)) || !(w - w == R(0))) bad |= 1;
            W[n] = (double)w;
        }
        for (int tx = 0; tx < TX; ++tx) for (int tz = 0; tz < TZ; ++tz) {
            R xlo, xhi, zlo, zhi;
            tile_axis(xg, X, tx, xlo, xhi);
            tile_axis(zg, Z, tz, zlo, zhi);
            if (ray_meets_box(q, xlo, xhi, zlo, zhi)) { ++hit; continue; }
            for (int i = TILE * tx; i < TILE * tx + TILE && i < X; ++i)
                for (int k = TILE * tz; k < TILE * tz + TILE && k < Z; ++k) if (sound && W[(size_t)i * Z + k] != 0.0) bad |= 2;
        }
        if (bad) { fprintf(stderr, "ray %d: the node weight broke its contract, flags %d\n", j, bad); return 1; }
        printf("%d", hit);
        for (double v : W) printf(" %.17g", v);
        printf("\n");
    }
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
