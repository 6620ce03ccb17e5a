/* run_scanconvert.c -- drives the 'scanconvert' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result with
 * qdas_scanconvert called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU): bit for bit.  A polar image of 9 x 7 nodes in 3 pages and a spherical
 * volume of 9 x 7 x 4 nodes in 2, single and double, real and complex, pre = none / abs / dB with a floor, fill NaN and 0; an empty call; refused classes and
 * sizes.  Prints "scanconvert gateway OK". */
#include <math.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { NR = 9, NA = 7, NE = 4, NZ = 21, NX = 17, NY = 5 };
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
static const double *stage_axis(const double *v, int n, int degrees) {
    double h[32];
    for (int k = 0; k < n; ++k) h[k] = degrees ? v[k] * 3.14159265358979323846 / 180.0 : v[k];
    return (const double *)stage(h, (size_t)n * sizeof(double));
}

/* the command against the C ABI: one class, real | complex, polar | spherical, one pre, one fill */
static int one(mxClassID cls, int cplx, int sph, int pre, double fill) {
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4;
    const int P = sph ? 2 : 3, E = sph ? NE : 0, Y = sph ? NY : 0;
    double r[NR], a[NA], e[NE], x[NX], y[NY], z[NZ];
    const double og[3] = {1e-3, -0.5e-3, -20e-3};
    for (int k = 0; k < NR; ++k) r[k] = 20e-3 + 30e-3 * pow((double)k / (NR - 1), 1.2);           /* non-uniform */
    for (int k = 0; k < NA; ++k) a[k] = -30.0 + 60.0 * k / (NA - 1);
    for (int k = 0; k < NE; ++k) e[k] = -12.0 + 27.0 * k / (NE - 1);
    for (int k = 0; k < NX; ++k) x[k] = og[0] - 30e-3 + 60e-3 * k / (NX - 1) + 1.3e-5;
    for (int k = 0; k < NY; ++k) y[k] = og[1] - 12e-3 + 27e-3 * k / (NY - 1) + 0.7e-5;
    for (int k = 0; k < NZ; ++k) z[k] = -6e-3 + 42e-3 * k / (NZ - 1) + 0.9e-5;
    const size_t nb = (size_t)NR * NA * (sph ? NE : 1) * P, nout = (size_t)NZ * NX * (sph ? NY : 1) * P;
    const mwSize bd[2] = {(mwSize)(NR * NA), (mwSize)(nb / (NR * NA))};
    mxArray *b = mxCreateNumericArray(2, bd, cls, cplx ? mxCOMPLEX : mxREAL);
    unsigned s = 1234u + (unsigned)(cplx + 2 * sph + 4 * pre);
    for (size_t k = 0; k < nb * (cplx ? 2 : 1); ++k) {
        s = s * 1664525u + 1013904223u;
        double v = ((double)((s >> 8) & 0xffff) / 32768.0 - 1.0) * 3.0;
        if (k % 37 == 5) v = 0.0;                                                                    /* exact zeros: the floor's reason */
        if (cls == mxDOUBLE_CLASS) ((double *)mxGetData(b))[k] = v; else ((float *)mxGetData(b))[k] = (float)v;
    }
    const double ov[3] = {(double)pre, -90.0, fill};
    mxArray *cmd = mxCreateString("scanconvert"), *ra = vec(r, NR), *aa = vec(a, NA), *ea = vec(e, E), *oa = vec(og, 3), *xa = vec(x, NX), *ya = vec(y, Y), *za = vec(z, NZ);
    mxArray *opts = vec(ov, 3), *out[2] = {NULL, NULL};
    const mxArray *in[10] = {cmd, b, ra, aa, ea, oa, xa, ya, za, opts};
    CHECK(call(1, out, 10, in) == 0 && out[0]);
    const int ocplx = cplx && pre == QDAS_SC_PRE_NONE;
    CHECK(mxGetClassID(out[0]) == cls && mxIsComplex(out[0]) == ocplx && mxGetNumberOfElements(out[0]) == nout);

    qdas_scanconvert_desc d;
    memset(&d, 0, sizeof d);
    d.R = NR; d.A = NA; d.E = (uint64_t)E; d.Z = NZ; d.X = NX; d.Y = (uint64_t)Y; d.P = (uint64_t)P;
    d.sr = 1; d.sa = NR; d.se = sph ? NR * NA : 0; d.sp = NR * NA * (sph ? NE : 1);
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32; d.cplx = cplx; d.pre = pre; d.device = -1;
    memcpy(d.origin, og, sizeof og);
    d.fill = fill; d.db_floor = -90.0;
    d.r = stage_axis(r, NR, 0); d.a = stage_axis(a, NA, 1); d.x = stage_axis(x, NX, 0); d.z = stage_axis(z, NZ, 0);
    if (sph) { d.e = stage_axis(e, NE, 1); d.y = stage_axis(y, NY, 0); }
    const size_t obytes = nout * es * (ocplx ? 2 : 1);
    void *db = stage(mxGetData(b), nb * es * (cplx ? 2 : 1)), *dout = NULL, *h = malloc(obytes);
    CHECK(d.r && d.a && d.x && d.z && db && h && !qdas_device_malloc(&dout, obytes, -1));
    CHECK(qdas_scanconvert(&d, db, dout) == 0);
    CHECK(!qdas_device_copy(h, dout, obytes, 1, -1));
    CHECK(memcmp(h, mxGetData(out[0]), obytes) == 0);
    size_t outside = 0, inside = 0;                                                                  /* both kinds of pixel occur, and outside holds fill */
    for (size_t k = 0; k < nout * (ocplx ? 2 : 1); k += (ocplx ? 2 : 1)) {
        const double v = cls == mxDOUBLE_CLASS ? ((const double *)h)[k] : (double)((const float *)h)[k];
        if (fill != fill ? v != v : v == fill) ++outside; else ++inside;
    }
    CHECK(outside > 0 && inside > 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    free(h);
    qdas_device_free((void *)d.r, -1); qdas_device_free((void *)d.a, -1); qdas_device_free((void *)d.x, -1); qdas_device_free((void *)d.z, -1);
    if (sph) { qdas_device_free((void *)d.e, -1); qdas_device_free((void *)d.y, -1); }
    qdas_device_free(db, -1); qdas_device_free(dout, -1);
    return 0;
}

int main(void) {
    for (int sph = 0; sph < 2; ++sph)
        for (int cplx = 0; cplx < 2; ++cplx)
            for (int pre = 0; pre < 3; ++pre) {
                if (one(mxSINGLE_CLASS, cplx, sph, pre, NAN) || one(mxDOUBLE_CLASS, cplx, sph, pre, pre == 1 ? 0.0 : NAN)) return 1;
            }
    printf("scanconvert through the gateway: bit-identical to the C ABI\n");
    /* opts = []: the defaults; no pages: an empty result; refused: an integer image, a sample count that is no multiple of R A, one range node, two outputs */
    const double r[3] = {1e-2, 2e-2, 3e-2}, a[3] = {-20, 0, 20}, og[3] = {0, 0, 0}, x[4] = {-1e-2, -1e-3, 2e-3, 1e-2}, z[2] = {1.5e-2, 2.5e-2};
    mxArray *cmd = mxCreateString("scanconvert"), *ra = vec(r, 3), *aa = vec(a, 3), *none = vec(r, 0), *oa = vec(og, 3), *xa = vec(x, 4), *za = vec(z, 2);
    mxArray *b = mxCreateNumericMatrix(9, 1, mxDOUBLE_CLASS, mxREAL), *bi = mxCreateNumericMatrix(9, 1, mxINT32_CLASS, mxREAL), *b10 = mxCreateNumericMatrix(10, 1, mxDOUBLE_CLASS, mxREAL);
    mxArray *b0 = mxCreateNumericMatrix(9, 0, mxSINGLE_CLASS, mxCOMPLEX), *r1 = vec(r, 1), *out[2] = {NULL, NULL};
    for (int k = 0; k < 9; ++k) ((double *)mxGetData(b))[k] = 1.0 + k;
    const mxArray *ok[10] = {cmd, b, ra, aa, none, oa, xa, none, za, none};
    CHECK(call(1, out, 10, ok) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8 && !mxIsComplex(out[0]));
    const double *v = (const double *)mxGetData(out[0]);
    CHECK(v[0] != v[0] && v[2] == v[2] && v[4] == v[4] && v[6] != v[6]);          /* x = -10 mm at z = 15 mm is outside +-20 degrees, x = -1 and 2 mm are inside */
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *e0[10] = {cmd, b0, ra, aa, none, oa, xa, none, za, none};
    CHECK(call(1, out, 10, e0) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0 && mxGetClassID(out[0]) == mxSINGLE_CLASS);
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *f1[10] = {cmd, bi, ra, aa, none, oa, xa, none, za, none}, *f2[10] = {cmd, b10, ra, aa, none, oa, xa, none, za, none};
    const mxArray *f3[10] = {cmd, b, r1, aa, none, oa, xa, none, za, none};
    CHECK(call(1, out, 10, f1) == 1 && strstr(fake_mex_last_msg, "single or double"));
    CHECK(call(1, out, 10, f2) == 1 && strstr(fake_mex_last_msg, "pages of R x A"));
    CHECK(call(1, out, 10, f3) == 1 && strstr(fake_mex_last_msg, "2 x 2"));
    CHECK(call(1, out, 9, ok) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(2, out, 10, ok) == 1 && strstr(fake_mex_last_id, "nargout"));
    printf("scanconvert gateway OK\n");
    return 0;
}
