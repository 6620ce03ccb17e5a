// resample_core_host.cpp -- qups_amd/csrc/resample_core.h on the CPU (TEST INFRASTRUCTURE): the index arithmetic the device kernel compiles, built for the host
// with -fsanitize=address,undefined by tests/test_resample_host.py and run on the cases that test writes to a file.  The loops below are the kernel's, lane by
// lane: the taps, the staging sweep with the edge rule, then per lane its outputs with the carried (n div p, n mod p) and the tap loop over
// the taps that exist.  The taps, the span and the record are heap blocks of exactly their size: an address outside its block is a sanitizer report.  The
// (For p = 1 the kernel shares one tap read among a lane's outputs: the same indices, order and accumulators.)  The
// program itself fails when a tap word or a span element is read that was not written, and counts how often each sample is loaded.
//
// Input (text): type (0 int16 | 1 float | 2 complex float | 3 double | 4 complex double)  edge  T C K p q off J
//               h[K]  x: C traces of T samples (complex: re im pairs)
// Output: first line "TJ lanes span lds_bytes loads_max", then one line per output element, j fastest, then c: "re im" in hexadecimal floating point.
// A second mode, "geom K p q elem_bytes real_bytes", prints "TJ lanes S Mmax rem span tap_bytes lds_bytes".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resample_core.h"

using namespace qdas::rs;

template <typename RT> struct Cplx { RT x, y; };

static float ldv(const int16_t *p, long i) { return (float)p[i]; }
static float ldv(const float *p, long i) { return p[i]; }
static double ldv(const double *p, long i) { return p[i]; }
template <typename RT> static Cplx<RT> ldv(const Cplx<RT> *p, long i) { return p[i]; }

template <typename RT> static RT reflect(RT a, RT v) { return (RT)2 * a - v; }
template <typename RT> static Cplx<RT> reflect(Cplx<RT> a, Cplx<RT> v) { return Cplx<RT>{(RT)2 * a.x - v.x, (RT)2 * a.y - v.y}; }
template <typename RT> static void mac(RT &a, RT x, RT h) { a = std::fma(x, h, a); }
template <typename RT> static void mac(Cplx<RT> &a, Cplx<RT> x, RT h) { a.x = std::fma(x.x, h, a.x); a.y = std::fma(x.y, h, a.y); }
static double re(float v) { return v; }
static double re(double v) { return v; }
static double im(float) { return 0; }
static double im(double) { return 0; }
template <typename RT> static double re(Cplx<RT> v) { return v.x; }
template <typename RT> static double im(Cplx<RT> v) { return v.y; }

static double rd(FILE *f) {
    char tok[64];
    if (fscanf(f, "%63s", tok) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return strtod(tok, nullptr);
}
static void rdx(FILE *f, int16_t &v) { v = (int16_t)rd(f); }
static void rdx(FILE *f, float &v) { v = (float)rd(f); }
static void rdx(FILE *f, double &v) { v = rd(f); }
template <typename RT> static void rdx(FILE *f, Cplx<RT> &v) { v.x = (RT)rd(f); v.y = (RT)rd(f); }

template <typename RT, typename TX, typename SIN>
static int run(FILE *f, int edge, long T, long C, long K, long p, long q, long off, long J) {
    RT *h = (RT *)malloc(sizeof(RT) * (size_t)K);
    for (long k = 0; k < K; ++k) h[k] = (RT)rd(f);
    const Geom g = geometry(K, p, q, (int)sizeof(TX), (int)sizeof(RT));
    if (g.TJ < 1 || g.lds_bytes > LDS_MAX) { fprintf(stderr, "does not fit\n"); return 4; }
    const int lanes = g.lanes;
    const int qd = (int)(q / p), qm = (int)(q % p), sd = (int)((long)lanes * q / p), sm = (int)((long)lanes * q % p);
    std::vector<TX> out((size_t)(J * C));
    long loads_max = 0;
    for (long c = 0; c < C; ++c) {
        SIN *x = (SIN *)malloc(sizeof(SIN) * (size_t)T);                  // exactly the record: no padding to wander into
        for (long i = 0; i < T; ++i) rdx(f, x[i]);
        std::vector<int> loads((size_t)T, 0);
        for (long j0 = 0; j0 < J; j0 += g.TJ) {
            const int nj = (int)(J - j0 < g.TJ ? J - j0 : g.TJ);
            const Tile tl = tile_extent(off, j0, nj, (int)p, (int)q, g.Mmax);
            const size_t ntap = g.tap_bytes / sizeof(RT), nspan = (g.lds_bytes - g.tap_bytes) / sizeof(TX);
            RT *H = (RT *)malloc(g.tap_bytes);
            TX *X = (TX *)malloc(g.lds_bytes - g.tap_bytes);
            std::vector<char> tw(ntap, 0), xw(nspan, 0);
            if (tl.len < 1 || (size_t)tl.len > nspan) { fprintf(stderr, "tile: %d span elements, room for %zu\n", tl.len, nspan); return 3; }
            for (int t = 0; t < lanes; ++t)                               // the taps
                for (long k = t; k < K; k += lanes) {
                    if ((size_t)k >= ntap || tw[(size_t)k]) { fprintf(stderr, "taps: word %ld out of range or written twice\n", k); return 3; }
                    H[k] = h[k];
                    tw[(size_t)k] = 1;
                }
            for (int t = 0; t < lanes; ++t)                               // the span, once, with the edge rule
                for (int e = t; e < tl.len; e += lanes) {
                    int64_t anchor;
                    const int64_t src = edge_source(tl.i_lo + e, T, edge, anchor);
                    TX v;
                    memset(&v, 0, sizeof v);
                    if (src >= 0) {
                        v = ldv(x, (long)src);
                        ++loads[(size_t)src];
                        if (anchor >= 0) v = reflect(ldv(x, (long)anchor), v);
                    }
                    if (xw[(size_t)e]) { fprintf(stderr, "staging: element %d written twice\n", e); return 3; }
                    X[e] = v;
                    xw[(size_t)e] = 1;
                }
            for (int t = 0; t < lanes; ++t) {
                int b, phi;
                lane_start(tl.f0, t, (int)p, qd, qm, b, phi);
                for (int jj = t; jj < nj; jj += lanes) {
                    const long n = off + (j0 + jj) * q;
                    if (tl.d0 + b != n / p || phi != n % p) { fprintf(stderr, "carry: output %ld has (%ld, %d), not (%ld, %ld)\n", j0 + jj, (long)tl.d0 + b, phi, n / p, n % p); return 3; }
                    if (p == 1 && (phi != 0 || b != jj * (int)q)) { fprintf(stderr, "p = 1: output %d is not (jj q, 0)\n", jj); return 3; }   // what the kernel's shared-tap path takes
                    TX acc;
                    memset(&acc, 0, sizeof acc);
                    const int ms = last_tap(g.Mmax, g.rem, phi);
                    if (ms != (phi < K ? (int)((K - 1 - phi) / p) : -1)) { fprintf(stderr, "last_tap: phase %d ends at %d\n", phi, ms); return 3; }
                    for (int m = 0; m <= ms; ++m) {
                        const int w = tap_word(phi, m, (int)p), e = b + g.Mmax - m;
                        if (w < 0 || w >= K || w != phi + m * (int)p || !tw[(size_t)w]) { fprintf(stderr, "tap word %d was not written\n", w); return 3; }
                        if (e < 0 || e >= tl.len || !xw[(size_t)e]) { fprintf(stderr, "span element %d was not staged (len %d)\n", e, tl.len); return 3; }
                        mac(acc, X[e], H[w]);
                    }
                    out[(size_t)(j0 + jj + J * c)] = acc;
                    advance(b, phi, sd, sm, (int)p);
                }
            }
            free(H);
            free(X);
        }
        for (long i = 0; i < T; ++i) if (loads[(size_t)i] > loads_max) loads_max = loads[(size_t)i];
        free(x);
    }
    printf("%d %d %d %u %ld\n", g.TJ, g.lanes, g.span, g.lds_bytes, loads_max);
    for (const TX &v : out) printf("%a %a\n", re(v), im(v));
    free(h);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "geom")) {
        const Geom g = geometry(atol(argv[2]), atol(argv[3]), atol(argv[4]), atoi(argv[5]), atoi(argv[6]));
        printf("%d %d %d %d %d %d %u %u\n", g.TJ, g.lanes, g.S, g.Mmax, g.rem, g.span, g.tap_bytes, g.lds_bytes);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "reach")) {                          // reach off J p q K: "any lo hi"
        int64_t lo = 0, hi = 0;
        const bool any = reach(atol(argv[2]), atol(argv[3]), atol(argv[4]), atol(argv[5]), atol(argv[6]), lo, hi);
        printf("%d %lld %lld\n", (int)any, (long long)lo, (long long)hi);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    const int type = (int)rd(f), edge = (int)rd(f);
    const long T = (long)rd(f), C = (long)rd(f), K = (long)rd(f), p = (long)rd(f), q = (long)rd(f), off = (long)rd(f), J = (long)rd(f);
    if (T < 1 || C < 1 || K < 1 || K > MAX_K || p < 1 || p > MAX_PQ || q < 1 || q > MAX_PQ || off < 0 || J < 1) { fprintf(stderr, "bad sizes\n"); return 2; }
    int rc;
    switch (type) {
        case 0: rc = run<float, float, int16_t>(f, edge, T, C, K, p, q, off, J); break;
        case 1: rc = run<float, float, float>(f, edge, T, C, K, p, q, off, J); break;
        case 2: rc = run<float, Cplx<float>, Cplx<float>>(f, edge, T, C, K, p, q, off, J); break;
        case 3: rc = run<double, double, double>(f, edge, T, C, K, p, q, off, J); break;
        default: rc = run<double, Cplx<double>, Cplx<double>>(f, edge, T, C, K, p, q, off, J); break;
    }
    fclose(f);
    return rc;
}
