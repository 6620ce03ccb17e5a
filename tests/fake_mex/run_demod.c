/* run_demod.c -- drives the 'demod' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so (TEST INFRASTRUCTURE; needs a GPU).  Each
 * result is compared bit for bit with qdas_demod called directly on device arrays, and written to a file named on the command line so that
 * tests/test_mex_demod.py can compare it bit for bit with the Python layer's on the same data.  int16, single, double, real and complex; 25 taps, ratio 4, two
 * start times (gdiv = 3); an empty call; refused classes and sizes.  Prints "demod gateway OK".
 *
 * The data are a fixed integer sequence both sides can form: x[i] = ((i * 7919 + 13) mod 2001) - 1000 (imaginary part: the same of i + 5), scaled by 1 / 256 for
 * the floating classes; b[k] = ((k * 31 + 7) mod 17 - 8) / 64. */
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

enum { NT = 1101, NC = 6, NK = 25, NRATIO = 4 };
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

static int one(mxClassID cls, int cplx, FILE *dump) {
    const double fc = 5.1e6, fs = 20e6, t0[2] = {3.3e-6, -1.7e-6};
    const int dbl = cls == mxDOUBLE_CLASS;
    const size_t es = cls == mxINT16_CLASS ? 2 : (dbl ? 8 : 4), n = (size_t)NT * NC, J = (NT + NRATIO - 1) / NRATIO;
    const mwSize xd[2] = {NT, NC};
    mxArray *x = mxCreateNumericArray(2, xd, cls, cplx ? mxCOMPLEX : mxREAL);
    for (size_t i = 0; i < n; ++i)
        for (int q = 0; q <= cplx; ++q) {
            const double v = sample((long)i + 5 * q);
            const size_t at = i * (size_t)(1 + cplx) + (size_t)q;
            if (cls == mxINT16_CLASS) ((int16_t *)mxGetData(x))[at] = (int16_t)v;
            else if (dbl) ((double *)mxGetData(x))[at] = v / 256.0;
            else ((float *)mxGetData(x))[at] = (float)(v / 256.0);
        }
    double b[NK];
    for (int k = 0; k < NK; ++k) b[k] = (double)((k * 31 + 7) % 17 - 8) / 64.0;
    const double prm[5] = {NT, fc, fs, NRATIO, 3};
    mxArray *cmd = mxCreateString("demod"), *ba = vec(b, NK), *pa = vec(prm, 5), *ta = vec(t0, 2), *out[2] = {NULL, NULL};
    const mxArray *in[5] = {cmd, x, ba, pa, ta};
    CHECK(call(1, out, 5, in) == 0 && out[0]);
    CHECK(mxGetClassID(out[0]) == (dbl ? mxDOUBLE_CLASS : mxSINGLE_CLASS) && mxIsComplex(out[0]) && mxGetNumberOfElements(out[0]) == J * NC);

    qdas_demod_desc d;
    memset(&d, 0, sizeof d);
    d.T = NT; d.C = NC; d.K = NK; d.R = NRATIO; d.x_ld = NT; d.out_ld = J;
    d.in_type = cls == mxINT16_CLASS ? QDAS_DEMOD_I16 : !dbl ? (cplx ? QDAS_DEMOD_C64 : QDAS_DEMOD_F32) : (cplx ? QDAS_DEMOD_C128 : QDAS_DEMOD_F64);
    d.device = -1;
    d.fc_over_fs = fc / fs; d.step = fc * (double)NRATIO / fs;
    d.gdiv = 3; d.G = 2;
    double cyc[2];
    for (int k = 0; k < 2; ++k) { const double c = fc * t0[k]; cyc[k] = c - floor(c); }
    float bf[NK];
    for (int k = 0; k < NK; ++k) bf[k] = (float)b[k];
    const size_t obytes = J * NC * (dbl ? 16 : 8);
    void *dx = stage(mxGetData(x), n * es * (size_t)(1 + cplx)), *db = dbl ? stage(b, sizeof b) : stage(bf, sizeof bf), *dc = stage(cyc, sizeof cyc), *dout = NULL;
    void *h = malloc(obytes);
    CHECK(dx && db && dc && h && !qdas_device_malloc(&dout, obytes, -1));
    d.cyc0 = (const double *)dc;
    CHECK(qdas_demod(&d, dx, db, dout) == 0);
    CHECK(!qdas_device_copy(h, dout, obytes, 1, -1));
    CHECK(memcmp(h, mxGetData(out[0]), obytes) == 0);
    size_t nonzero = 0;
    for (size_t k = 0; k < obytes; ++k) nonzero += ((const unsigned char *)h)[k] != 0;
    CHECK(nonzero > obytes / 4);
    if (dump) CHECK(fwrite(mxGetData(out[0]), 1, obytes, dump) == obytes);
    mxDestroyArray(out[0]);
    free(h);
    qdas_device_free(dx, -1); qdas_device_free(db, -1); qdas_device_free(dc, -1); qdas_device_free(dout, -1);
    return 0;
}

int main(int argc, char **argv) {
    FILE *dump = argc > 1 ? fopen(argv[1], "wb") : NULL;
    if (argc > 1 && !dump) { perror(argv[1]); return 2; }
    /* the order the Python side reads the file in: int16, single, single complex, double, double complex */
    if (one(mxINT16_CLASS, 0, dump) || one(mxSINGLE_CLASS, 0, dump) || one(mxSINGLE_CLASS, 1, dump) || one(mxDOUBLE_CLASS, 0, dump) || one(mxDOUBLE_CLASS, 1, dump)) return 1;
    if (dump) fclose(dump);
    printf("demod through the gateway: bit-identical to the C ABI\n");
    /* an empty record; refused: an integer class, complex int16, a sample count that is no multiple of T, a ratio of 0, no taps, too many taps, nargin, nargout */
    const double prm[5] = {8, 5e6, 20e6, 2, 1}, prm0[5] = {0, 5e6, 20e6, 2, 1}, prmr[5] = {8, 5e6, 20e6, 0, 1}, prm3[5] = {3, 5e6, 20e6, 2, 1}, b[2] = {0.5, 0.5}, t0[1] = {0.0};
    static double many[QDAS_DEMOD_MAX_K + 1];
    mxArray *cmd = mxCreateString("demod"), *x = mxCreateNumericMatrix(8, 2, mxSINGLE_CLASS, mxREAL), *xi = mxCreateNumericMatrix(8, 2, mxINT32_CLASS, mxREAL);
    mxArray *xc = mxCreateNumericMatrix(8, 2, mxINT16_CLASS, mxCOMPLEX), *x0 = mxCreateNumericMatrix(0, 2, mxDOUBLE_CLASS, mxREAL);
    mxArray *ba = vec(b, 2), *bn = vec(b, 0), *bm = vec(many, QDAS_DEMOD_MAX_K + 1), *pa = vec(prm, 5), *p0 = vec(prm0, 5), *pr = vec(prmr, 5), *p3 = vec(prm3, 5), *ta = vec(t0, 1);
    mxArray *out[2] = {NULL, NULL};
    for (int k = 0; k < 16; ++k) ((float *)mxGetData(x))[k] = (float)(k + 1);
    const mxArray *ok[5] = {cmd, x, ba, pa, ta};
    CHECK(call(1, out, 5, ok) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8 && mxIsComplex(out[0]) && mxGetClassID(out[0]) == mxSINGLE_CLASS);
    const float *v = (const float *)mxGetData(out[0]);
    CHECK(fabsf(v[0] - 0.5f) < 1e-6f && fabsf(v[1]) < 1e-6f);                              /* out[0] = b[0] x[0] at phase 0 */
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *e0[5] = {cmd, x0, ba, p0, ta};
    CHECK(call(1, out, 5, e0) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0 && mxGetClassID(out[0]) == mxDOUBLE_CLASS);
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *f1[5] = {cmd, xi, ba, pa, ta}, *f2[5] = {cmd, xc, ba, pa, ta}, *f3[5] = {cmd, x, ba, p3, ta}, *f4[5] = {cmd, x, ba, pr, ta};
    const mxArray *f5[5] = {cmd, x, bn, pa, ta}, *f6[5] = {cmd, x, bm, pa, ta};
    CHECK(call(1, out, 5, f1) == 1 && strstr(fake_mex_last_msg, "int16 (real), single or double"));
    CHECK(call(1, out, 5, f2) == 1 && strstr(fake_mex_last_msg, "int16 (real), single or double"));
    CHECK(call(1, out, 5, f3) == 1 && strstr(fake_mex_last_msg, "traces of T"));
    CHECK(call(1, out, 5, f4) == 1 && strstr(fake_mex_last_msg, "prm ="));
    CHECK(call(1, out, 5, f5) == 1 && strstr(fake_mex_last_msg, "must not be empty"));
    CHECK(call(1, out, 5, f6) == 1 && strstr(fake_mex_last_msg, "taps"));
    CHECK(call(1, out, 4, ok) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(2, out, 5, ok) == 1 && strstr(fake_mex_last_id, "nargout"));
    printf("demod gateway OK\n");
    return 0;
}
