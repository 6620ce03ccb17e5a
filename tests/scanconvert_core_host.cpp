// scanconvert_core_host.cpp -- qups_amd/csrc/scanconvert_core.h on the CPU (TEST INFRASTRUCTURE): the text the device kernels compile, built for the host with
// -fsanitize=address,undefined by tests/test_scanconvert_host.py and run on the cases that test writes to a file.  The loop below is the kernel's: the pitch
// test over every node of an axis, then per pixel the coordinates, the cells, the weights rounded to the data's type and the lerps per page.  Every array is a
// heap block of exactly its size, so a cell outside its axis or a corner outside the data is a sanitizer report; the program itself fails on a cell index
// outside [0, n - 2].
//
// Input (text): kind (2 | 3)  bits (32 | 64)  cplx  pre  R A E  Z X Y  P  bisect
//               origin[3]  fill  db_floor
//               r[R]  a[A]  e[E]  x[X]  y[Y]  z[Z]            (polar: E = 0 and Y = 0, no values)
//               b: R A max(E, 1) P samples, r fastest (complex: re im pairs)
// Output: one line per output element, z fastest, then x, [y], pages: "inside re im" in hexadecimal floating point (im = 0 for real output);
//         the first line is "uniform_r uniform_a uniform_e".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scanconvert_core.h"

using namespace qdas::sc;

static double *read_axis(FILE *f, long n) {
    double *g = n ? (double *)malloc(sizeof(double) * (size_t)n) : nullptr;
    for (long i = 0; i < n; ++i) {
        char tok[64];
        if (fscanf(f, "%63s", tok) != 1) { fprintf(stderr, "short axis\n"); exit(2); }
        g[i] = strtod(tok, nullptr);                             // (strtod reads nan and inf)
    }
    return g;
}

static double axis_inv(const double *g, int n, bool bisect, int *uniform) {
    const double pitch = pitch_of(g[0], g[n - 1], n);
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = on_pitch(g[i], g[0], i, pitch) && ok;
    *uniform = ok;
    return inv_pitch(pitch, ok && !bisect);
}

template <typename R, bool CPLX, int PRE>
static int run(FILE *f, int kind, long Rn, long An, long En, long Z, long X, long Y, long P, int bisect, const double *og, double fill, double db_floor,
               const double *r, const double *a, const double *e, const double *x, const double *y, const double *z) {
    using V = typename Value<R, CPLX, PRE>::T;
    const long Ee = kind == 3 ? En : 1, Ye = kind == 3 ? Y : 1;
    const size_t ns = (size_t)(Rn * An * Ee * P);
    Cx<R> *bc = nullptr;
    R *br = nullptr;
    if (CPLX) bc = (Cx<R> *)aligned_alloc(2 * sizeof(R), sizeof(Cx<R>) * (ns ? ns : 1));
    else br = (R *)malloc(sizeof(R) * (ns ? ns : 1));
    for (size_t i = 0; i < ns; ++i) {
        char t1[64], t2[64] = "0";
        if (fscanf(f, "%63s", t1) != 1 || (CPLX && fscanf(f, "%63s", t2) != 1)) { fprintf(stderr, "short data\n"); return 2; }
        if (CPLX) { bc[i].re = (R)strtod(t1, nullptr); bc[i].im = (R)strtod(t2, nullptr); }
        else br[i] = (R)strtod(t1, nullptr);
    }
    const void *b = CPLX ? (const void *)bc : (const void *)br;
    int ur = 0, ua = 0, ue = 0;
    const double inv_r = axis_inv(r, (int)Rn, bisect, &ur), inv_a = axis_inv(a, (int)An, bisect, &ua);
    const double inv_e = kind == 3 ? axis_inv(e, (int)En, bisect, &ue) : 0.0;
    printf("%d %d %d\n", ur, ua, ue);
    const int64_t sr = 1, sa = Rn, se = Rn * An, sp = Rn * An * Ee;
    std::vector<V> out((size_t)(Z * X * Ye * P));
    std::vector<char> ins((size_t)(Z * X * Ye));
    for (long yy = 0; yy < Ye; ++yy)
        for (long j = 0; j < X; ++j)
            for (long i = 0; i < Z; ++i) {
                const double dz = z[i] - og[2], dx = x[j] - og[0];
                int k = 0, l = 0, m = 0;
                double wu = 0, wv = 0, ww = 0;
                bool in;
                if (kind == 3) {
                    double rho, alpha, eps;
                    spherical_of(dz, dx, y[yy] - og[1], rho, alpha, eps);
                    in = locate(r, (int)Rn, rho, inv_r, k, wu);
                    in = locate(a, (int)An, alpha, inv_a, l, wv) && in;
                    in = locate(e, (int)En, eps, inv_e, m, ww) && in;
                } else {
                    double rho, alpha;
                    polar_of(dz, dx, rho, alpha);
                    in = locate(r, (int)Rn, rho, inv_r, k, wu);
                    in = locate(a, (int)An, alpha, inv_a, l, wv) && in;
                }
                if (k < 0 || k > Rn - 2 || l < 0 || l > An - 2 || m < 0 || (kind == 3 && m > En - 2)) { fprintf(stderr, "cell outside its axis: %d %d %d\n", k, l, m); return 3; }
                const R u = (R)wu, v = (R)wv, w = (R)ww;
                const int64_t o = k * sr + l * sa + m * se;
                const size_t q = (size_t)(i + Z * (j + X * yy));
                ins[q] = in;
                for (long pg = 0; pg < P; ++pg) {
                    V val = filled<R, CPLX, PRE>((R)fill);
                    if (in) val = kind == 3 ? trilerp<R, CPLX, PRE>(b, o + pg * sp, sr, sa, se, u, v, w, (R)db_floor) : bilerp<R, CPLX, PRE>(b, o + pg * sp, sr, sa, u, v, (R)db_floor);
                    out[q + (size_t)pg * (size_t)(Z * X * Ye)] = val;
                }
            }
    for (long pg = 0; pg < P; ++pg)
        for (size_t q = 0; q < (size_t)(Z * X * Ye); ++q) {
            const V val = out[q + (size_t)pg * (size_t)(Z * X * Ye)];
            if constexpr (CPLX && PRE == PRE_NONE) printf("%d %a %a\n", (int)ins[q], (double)val.re, (double)val.im);
            else printf("%d %a 0\n", (int)ins[q], (double)val);
        }
    free(bc);
    free(br);
    return 0;
}

template <typename R, bool CPLX, typename... T> static int by_pre(int pre, T... t) {
    if (pre == PRE_NONE) return run<R, CPLX, PRE_NONE>(t...);
    if (pre == PRE_ABS) return run<R, CPLX, PRE_ABS>(t...);
    return run<R, CPLX, PRE_DB>(t...);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int kind, bits, cplx, pre, bisect;
    long Rn, An, En, Z, X, Y, P;
    if (fscanf(f, "%d %d %d %d %ld %ld %ld %ld %ld %ld %ld %d", &kind, &bits, &cplx, &pre, &Rn, &An, &En, &Z, &X, &Y, &P, &bisect) != 12) { fprintf(stderr, "bad header\n"); return 2; }
    if ((kind != 2 && kind != 3) || Rn < 2 || An < 2 || (kind == 3 && En < 2) || pre < 0 || pre > 2) { fprintf(stderr, "bad sizes\n"); return 2; }
    double *head = read_axis(f, 5);
    double *r = read_axis(f, Rn), *a = read_axis(f, An), *e = read_axis(f, kind == 3 ? En : 0);
    double *x = read_axis(f, X), *y = read_axis(f, kind == 3 ? Y : 0), *z = read_axis(f, Z);
    int rc;
    if (bits == 32) rc = cplx ? by_pre<float, true>(pre, f, kind, Rn, An, En, Z, X, Y, P, bisect, head, head[3], head[4], r, a, e, x, y, z)
                              : by_pre<float, false>(pre, f, kind, Rn, An, En, Z, X, Y, P, bisect, head, head[3], head[4], r, a, e, x, y, z);
    else rc = cplx ? by_pre<double, true>(pre, f, kind, Rn, An, En, Z, X, Y, P, bisect, head, head[3], head[4], r, a, e, x, y, z)
                   : by_pre<double, false>(pre, f, kind, Rn, An, En, Z, X, Y, P, bisect, head, head[3], head[4], r, a, e, x, y, z);
    free(head); free(r); free(a); free(e); free(x); free(y); free(z);
    fclose(f);
    return rc;
}
