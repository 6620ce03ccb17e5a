/* run_resample.c -- drives the 'resample' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so (TEST INFRASTRUCTURE; needs a GPU).  Each
 * result is compared bit for bit with qdas_resample called directly on device arrays, and written to a file named on the command line so that
 * tests/test_mex_resample.py can compare it bit for bit with the Python layer's on the same data.  int16, single, double, real and complex; 41 taps; the rate
 * 5/4 with zeros outside the record (resample's shape) and the rate 1/1 with the odd edge (filtfilt's shape); an empty call; refused classes and sizes.
 * Prints "resample gateway OK".
 *
 * The data are a fixed integer sequence both sides can form: x[i] = ((i * 7919 + 13) mod 2001) - 1000 (imaginary part: the same of i + 5), scaled by 1 / 256 for
 * the floating classes; h[k] = ((k * 31 + 7) mod 17 - 8) / 64. */
#include <math.h>
#include <setjmp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { NT = 301, NC = 3, NK = 41 };
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s / %s)\n", __LINE__, #c, fake_mex_last_id, fake_mex_last_msg); return 1; } } while (0)

static int call(int nlhs, mxArray **out, int nrhs, const mxArray **in) {     /* 0: returned, 1: raised */
    if (setjmp(fake_mex_jmp)) return 1;
    mexFunction(nlhs, out, nrhs, in);
    return 0;
}
static mxArray *vec(const double *v, int n) {
    mxArray *a = mxCreateNumericMatrix(1, (mwSize)n, mxDOUBLE_CLASS, mxREAL);
    if (n) memcpy(mxGetData(a), v, (size_t)n * sizeof(double));
    return a;
}
static void *stage(const void *h, size_t bytes) {
    void *p = NULL;
    if (qdas_device_malloc(&p, bytes, -1) || qdas_device_copy(p, h, bytes, 0, -1)) return NULL;
    return p;
}
static double sample(long i) { return (double)((i * 7919 + 13) % 2001 - 1000); }

static int one(mxClassID cls, int cplx, int p, int q, int edge, FILE *dump) {
    const int dbl = cls == mxDOUBLE_CLASS;
    const size_t es = cls == mxINT16_CLASS ? 2 : (dbl ? 8 : 4), n = (size_t)NT * NC, J = (size_t)qdas_resample_len(NT, (uint64_t)p, (uint64_t)q);
    const mwSize xd[2] = {NT, NC};
    mxArray *x = mxCreateNumericArray(2, xd, cls, cplx ? mxCOMPLEX : mxREAL);
    for (size_t i = 0; i < n; ++i)
        for (int r = 0; r <= cplx; ++r) {
            const double v = sample((long)i + 5 * r);
            const size_t at = i * (size_t)(1 + cplx) + (size_t)r;
            if (cls == mxINT16_CLASS) ((int16_t *)mxGetData(x))[at] = (int16_t)v;
            else if (dbl) ((double *)mxGetData(x))[at] = v / 256.0;
            else ((float *)mxGetData(x))[at] = (float)(v / 256.0);
        }
    double h[NK];
    for (int k = 0; k < NK; ++k) h[k] = (double)((k * 31 + 7) % 17 - 8) / 64.0;
    const double prm[6] = {NT, p, q, (NK - 1) / 2, (double)J, edge};
    mxArray *cmd = mxCreateString("resample"), *ha = vec(h, NK), *pa = vec(prm, 6), *out[2] = {NULL, NULL};
    const mxArray *in[4] = {cmd, x, ha, pa};
    CHECK(call(1, out, 4, in) == 0 && out[0]);
    CHECK(mxGetClassID(out[0]) == (dbl ? mxDOUBLE_CLASS : mxSINGLE_CLASS) && (mxIsComplex(out[0]) ? 1 : 0) == cplx && mxGetNumberOfElements(out[0]) == J * NC);

    qdas_resample_desc d;
    memset(&d, 0, sizeof d);
    d.T = NT; d.C = NC; d.K = NK; d.J = J; d.p = (uint64_t)p; d.q = (uint64_t)q; d.off = (NK - 1) / 2; d.x_ld = NT; d.out_ld = J;
    d.in_type = cls == mxINT16_CLASS ? QDAS_RESAMPLE_I16 : !dbl ? (cplx ? QDAS_RESAMPLE_C64 : QDAS_RESAMPLE_F32) : (cplx ? QDAS_RESAMPLE_C128 : QDAS_RESAMPLE_F64);
    d.edge = edge;
    d.device = -1;
    float hf[NK];
    for (int k = 0; k < NK; ++k) hf[k] = (float)h[k];
    const size_t obytes = J * NC * (dbl ? 8 : 4) * (size_t)(1 + cplx);
    void *dx = stage(mxGetData(x), n * es * (size_t)(1 + cplx)), *dh = dbl ? stage(h, sizeof h) : stage(hf, sizeof hf), *dout = NULL;
    void *hb = malloc(obytes);
    CHECK(dx && dh && hb && !qdas_device_malloc(&dout, obytes, -1));
    CHECK(qdas_resample(&d, dx, dh, dout) == 0);
    CHECK(!qdas_device_copy(hb, dout, obytes, 1, -1));
    CHECK(memcmp(hb, mxGetData(out[0]), obytes) == 0);
    size_t nonzero = 0;
    for (size_t k = 0; k < obytes; ++k) nonzero += ((const unsigned char *)hb)[k] != 0;
    CHECK(nonzero > obytes / 4);
    if (dump) CHECK(fwrite(mxGetData(out[0]), 1, obytes, dump) == obytes);
    mxDestroyArray(out[0]);
    free(hb);
    qdas_device_free(dx, -1); qdas_device_free(dh, -1); qdas_device_free(dout, -1);
    return 0;
}

int main(int argc, char **argv) {
    FILE *dump = argc > 1 ? fopen(argv[1], "wb") : NULL;
    if (argc > 1 && !dump) { perror(argv[1]); return 2; }
    /* the order the Python side reads the file in: per class (int16, single, single complex, double, double complex) the rate 5/4, then the odd edge at 1/1 */
    const mxClassID cl[5] = {mxINT16_CLASS, mxSINGLE_CLASS, mxSINGLE_CLASS, mxDOUBLE_CLASS, mxDOUBLE_CLASS};
    const int cx[5] = {0, 0, 1, 0, 1};
    for (int k = 0; k < 5; ++k)
        if (one(cl[k], cx[k], 5, 4, 0, dump) || one(cl[k], cx[k], 1, 1, 1, dump)) return 1;
    if (dump) fclose(dump);
    printf("resample through the gateway: bit-identical to the C ABI\n");
    /* a tiny call by hand; an empty call; refused: an integer class, complex int16, a sample count that is no multiple of T, p = 0, no taps, too many taps,
     * the odd edge beyond its reach, nargin, nargout */
    const double prm[6] = {8, 2, 1, 0, 16, 0}, prm0[5] = {8, 2, 1, 0, 0}, prmp[5] = {8, 0, 1, 0, 16}, prm3[5] = {3, 2, 1, 0, 16}, prmo[6] = {8, 1, 1, 0, 8, 1}, h[2] = {0.5, 0.25};
    static double many[QDAS_RESAMPLE_MAX_K + 1];
    mxArray *cmd = mxCreateString("resample"), *x = mxCreateNumericMatrix(8, 2, mxSINGLE_CLASS, mxREAL), *xi = mxCreateNumericMatrix(8, 2, mxINT32_CLASS, mxREAL);
    mxArray *xc = mxCreateNumericMatrix(8, 2, mxINT16_CLASS, mxCOMPLEX);
    mxArray *ha = vec(h, 2), *hn = vec(h, 0), *hm = vec(many, QDAS_RESAMPLE_MAX_K + 1), *pa = vec(prm, 6), *p0 = vec(prm0, 5), *pp = vec(prmp, 5), *p3 = vec(prm3, 5), *po = vec(prmo, 6);
    mxArray *out[2] = {NULL, NULL};
    for (int k = 0; k < 16; ++k) ((float *)mxGetData(x))[k] = (float)(k + 1);
    const mxArray *ok[4] = {cmd, x, ha, pa};
    CHECK(call(1, out, 4, ok) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 32 && !mxIsComplex(out[0]) && mxGetClassID(out[0]) == mxSINGLE_CLASS);
    const float *v = (const float *)mxGetData(out[0]);
    CHECK(v[0] == 0.5f && v[1] == 0.25f && v[2] == 1.0f && v[3] == 0.5f);                 /* upfirdn([1 2 ..], [0.5 0.25], 2, 1) */
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *e0[4] = {cmd, x, ha, p0};
    CHECK(call(1, out, 4, e0) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0 && mxGetClassID(out[0]) == mxSINGLE_CLASS);
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *f1[4] = {cmd, xi, ha, pa}, *f2[4] = {cmd, xc, ha, pa}, *f3[4] = {cmd, x, ha, p3}, *f4[4] = {cmd, x, ha, pp};
    const mxArray *f5[4] = {cmd, x, hn, pa}, *f6[4] = {cmd, x, hm, pa}, *f7[4] = {cmd, x, ha, po};
    CHECK(call(1, out, 4, f1) == 1 && strstr(fake_mex_last_msg, "int16 (real), single or double"));
    CHECK(call(1, out, 4, f2) == 1 && strstr(fake_mex_last_msg, "int16 (real), single or double"));
    CHECK(call(1, out, 4, f3) == 1 && strstr(fake_mex_last_msg, "traces of T"));
    CHECK(call(1, out, 4, f4) == 1 && strstr(fake_mex_last_msg, "prm ="));
    CHECK(call(1, out, 4, f5) == 1 && strstr(fake_mex_last_msg, "must not be empty"));
    CHECK(call(1, out, 4, f6) == 1 && strstr(fake_mex_last_msg, "taps"));
    CHECK(call(1, out, 4, f7) == 0 && out[0]);                                             /* off = 0, K = 2: reads x[-1], within the reach of 8 samples */
    mxDestroyArray(out[0]); out[0] = NULL;
    const double prmfar[6] = {2, 1, 1, 0, 2, 1}, h4[4] = {1, 1, 1, 1};
    mxArray *x2 = mxCreateNumericMatrix(2, 1, mxSINGLE_CLASS, mxREAL), *pf = vec(prmfar, 6), *h4a = vec(h4, 4);
    const mxArray *f8[4] = {cmd, x2, h4a, pf};
    CHECK(call(1, out, 4, f8) == 1 && strstr(fake_mex_last_msg, "reach"));                 /* reads x[-3] of a record of 2 */
    CHECK(call(1, out, 3, ok) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(2, out, 4, ok) == 1 && strstr(fake_mex_last_id, "nargout"));
    printf("resample gateway OK\n");
    return 0;
}
