// demod_core_host.cpp -- qups_amd/csrc/demod_core.h on the CPU (TEST INFRASTRUCTURE): the index and phase arithmetic the device kernel compiles, built for the
// host with -fsanitize=address,undefined by tests/test_demod_host.py and run on the cases that test writes to a file.  The loops below are the kernel's, lane
// by lane: the modulated taps, per phase group the staging sweep (lanes along the global index, zero-fill outside the record), per phase the tap groups over
// the rotating eight-entry window, then the transpose and the phasor.  The taps, the rows and the transpose buffer are heap blocks of exactly the bytes the
// launch asks for, and the record a block of exactly T samples per trace: an address outside its block is a sanitizer report.  The program itself fails when a
// row element is multiplied that the staging sweep did not write, and counts how often each sample is loaded.
//
// Input (text): bits (32 | 64)  cplx  T C K R  fc_over_fs  step  G  gdiv
//               cyc0[G]  b[K]  x: C traces of T samples (complex: re im pairs)
// Output: first line "S NG QP EN PG lds_bytes loads_max", then one line per output element, j fastest, then c: "re im" in hexadecimal floating point.
// A second mode, "map K R elem_bytes cplx_bytes", prints the LDS map the header computes (print_map below).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "demod_core.h"

using namespace qdas::dm;

template <typename RT> struct Cplx { RT x, y; };

template <typename RT> static void mac(Cplx<RT> &a, RT x, Cplx<RT> h) { a.x = std::fma(x, h.x, a.x); a.y = std::fma(x, h.y, a.y); }
template <typename RT> static void mac(Cplx<RT> &a, Cplx<RT> x, Cplx<RT> h) {
    a.x = std::fma(x.x, h.x, a.x); a.x = std::fma(-x.y, h.y, a.x);
    a.y = std::fma(x.x, h.y, a.y); a.y = std::fma(x.y, h.x, a.y);
}
template <typename RT> static void sincos_cycles(double cyc, RT &s, RT &c) {
    const double a = M_PI * (double)(RT)(2.0 * centred(cyc));
    s = (RT)std::sin(a); c = (RT)std::cos(a);
}
static double rd(FILE *f) {
    char tok[64];
    if (fscanf(f, "%63s", tok) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return strtod(tok, nullptr);
}
template <typename RT> static void rdx(FILE *f, RT &v) { v = (RT)rd(f); }
template <typename RT> static void rdx(FILE *f, Cplx<RT> &v) { v.x = (RT)rd(f); v.y = (RT)rd(f); }

template <typename RT, typename TX>
static int run(FILE *f, long T, long C, long K, long R, double fc_over_fs, double step, long G, long gdiv) {
    using CT = Cplx<RT>;
    std::vector<double> cyc0((size_t)G);
    for (auto &v : cyc0) v = rd(f);
    RT *b = (RT *)malloc(sizeof(RT) * (size_t)K);
    for (long k = 0; k < K; ++k) b[k] = (RT)rd(f);
    const Geom g = geometry(K, R, (int)sizeof(TX), (int)sizeof(CT));
    if (g.PG < 1 || g.lds_bytes > LDS_MAX) { fprintf(stderr, "does not fit\n"); return 4; }
    const long J = (long)out_len((uint64_t)T, (uint64_t)R);
    std::vector<CT> out((size_t)(J * C));
    long loads_max = 0;
    for (long c = 0; c < C; ++c) {
        TX *x = (TX *)malloc(sizeof(TX) * (size_t)T);                     // exactly the record: no padding to wander into
        for (long i = 0; i < T; ++i) rdx(f, x[i]);
        std::vector<int> loads((size_t)T, 0);
        for (long j0 = 0; j0 < J; j0 += TILE) {
            CT *H = (CT *)malloc(g.tap_bytes);
            const size_t body = g.lds_bytes - g.tap_bytes;
            unsigned char *Xraw = (unsigned char *)malloc(body);
            TX *X = (TX *)Xraw;
            for (long k = 0; k < K; ++k) {
                RT s, co;
                sincos_cycles<RT>(tap_cycles(k, fc_over_fs), s, co);
                H[k] = CT{b[k] * co, b[k] * s};
            }
            std::vector<CT> acc((size_t)TILE, CT{0, 0});
            for (int sa = 0; sa < g.S; sa += g.PG) {
                const int pg = g.S - sa < g.PG ? g.S - sa : g.PG;
                std::vector<char> written(body / sizeof(TX), 0);
                for (int t = 0; t < LANES; ++t) {                         // the staging sweep
                    const int de = LANES / pg, dd = LANES % pg;
                    int d = t % pg, e = t / pg;
                    while (e < g.EN) {
                        const int64_t i = sample_index(j0, g.NG, e, R, sa + d);
                        TX v;
                        memset(&v, 0, sizeof v);
                        if (i >= 0 && i < T) { v = x[i]; ++loads[(size_t)i]; }
                        const int w = lds_word(d, e, g.QP);
                        if (w < 0 || (size_t)w >= written.size() || written[(size_t)w]) { fprintf(stderr, "staging: word %d out of range or written twice\n", w); return 3; }
                        X[w] = v;
                        written[(size_t)w] = 1;
                        d += dd; e += de;
                        if (d >= pg) { d -= pg; ++e; }
                    }
                }
                for (int t = 0; t < LANES; ++t)
                    for (int d = 0; d < pg; ++d) {
                        const int s = sa + d, ms = last_tap(K, R, s);
                        const int base = d * OPL * g.QP;
                        TX win[2 * OPL];
                        auto row = [&](int w, int q) -> TX {
                            const int word = base + w * g.QP + q;
                            if (q < 0 || q >= g.QP || !written[(size_t)word]) { fprintf(stderr, "window: quad %d of plane %d was not staged\n", q, w); exit(3); }
                            return X[word];
                        };
                        for (int w = 0; w < OPL; ++w) win[OPL + w] = row(w, window_quad(g.NG, t, 0, w));
                        for (int gi = 0; OPL * gi <= ms; ++gi) {
                            const int half = (gi & 1) ? OPL : 0;                 // even groups load the lower half, odd groups the upper
                            for (int w = 0; w < OPL; ++w) win[half + w] = row(w, window_quad(g.NG, t, gi, w - OPL));
                            for (int u = 0; u < OPL; ++u) {
                                const int m = OPL * gi + u;
                                if (m > ms) break;
                                const CT tap = H[s + (int64_t)m * R];
                                for (int r = 0; r < OPL; ++r) mac(acc[(size_t)(OPL * t + r)], win[(half + OPL + r - u) & (2 * OPL - 1)], tap);
                            }
                        }
                    }
            }
            CT *O = (CT *)Xraw;
            for (int e = 0; e < TILE; ++e) O[out_word(e, (int)sizeof(CT))] = acc[(size_t)e];
            const double c0 = cyc0[(size_t)((c / gdiv) % G)];
            for (int e = 0; e < TILE && j0 + e < J; ++e) {
                const CT a = O[out_word(e, (int)sizeof(CT))];
                RT s, co;
                sincos_cycles<RT>(out_cycles(c0, j0 + e, step), s, co);
                out[(size_t)(j0 + e + J * c)] = CT{std::fma(a.y, s, a.x * co), std::fma(-a.x, s, a.y * co)};
            }
            free(H);
            free(Xraw);
        }
        for (long i = 0; i < T; ++i) if (loads[(size_t)i] > loads_max) loads_max = loads[(size_t)i];
        free(x);
    }
    printf("%d %d %d %d %d %u %ld\n", g.S, g.NG, g.QP, g.EN, g.PG, g.lds_bytes, loads_max);
    for (const CT &v : out) printf("%a %a\n", (double)v.x, (double)v.y);
    free(b);
    return 0;
}

// "map K R elem_bytes cplx_bytes": the header's LDS map itself, for tests/test_demod_host.py to judge.  Line 1: NG QP EN pg (the phases of the first staging
// group); line 2: lds_word(d, e, QP) for d < pg, e < EN, d slowest; line 3: the word each of the LANES lanes writes in its first staging store.
static int print_map(long K, long R, int elem_bytes, int cplx_bytes) {
    const Geom g = geometry(K, R, elem_bytes, cplx_bytes);
    if (g.PG < 1 || g.lds_bytes > LDS_MAX) { fprintf(stderr, "does not fit\n"); return 4; }
    const int pg = g.S < g.PG ? g.S : g.PG;
    printf("%d %d %d %d\n", g.NG, g.QP, g.EN, pg);
    for (int d = 0; d < pg; ++d)
        for (int e = 0; e < g.EN; ++e) printf("%d ", lds_word(d, e, g.QP));
    printf("\n");
    for (int t = 0; t < LANES; ++t) printf("%d ", lds_word(t % pg, t / pg, g.QP));
    printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "map")) return print_map(atol(argv[2]), atol(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc != 2) { fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    const int bits = (int)rd(f), cplx = (int)rd(f);
    const long T = (long)rd(f), C = (long)rd(f), K = (long)rd(f), R = (long)rd(f);
    const double fc_over_fs = rd(f), step = rd(f);
    const long G = (long)rd(f), gdiv = (long)rd(f);
    if (T < 1 || C < 1 || K < 1 || K > MAX_K || R < 1 || R > MAX_R || G < 1 || gdiv < 1) { fprintf(stderr, "bad sizes\n"); return 2; }
    int rc;
    if (bits == 32) rc = cplx ? run<float, Cplx<float>>(f, T, C, K, R, fc_over_fs, step, G, gdiv) : run<float, float>(f, T, C, K, R, fc_over_fs, step, G, gdiv);
    else            rc = cplx ? run<double, Cplx<double>>(f, T, C, K, R, fc_over_fs, step, G, gdiv) : run<double, double>(f, T, C, K, R, fc_over_fs, step, G, gdiv);
    fclose(f);
    return rc;
}
