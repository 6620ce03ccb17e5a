/* run_raybackproject.c -- drives the 'raybackproject' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result
 * bit for bit with qdas_raypaths_backproject called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  The grid and the rays of run_raypaths.c (the
 * reference's -5:5 x -4:4 with the ray of its example, a vertical ray on the last column, a ray that misses, a point ray and a NaN); double and single; both
 * map layouts; one origin against many end points; the column sums alone (F = 0); no rays; refused strides, classes and argument counts.  With a file name as
 * argv[1] the double case's r (J x F), g (X Z x F, strides [Z 1]) and col (X Z) are written there as raw float64, for the test to hold against the Python layer.
 * Prints "raybackproject gateway OK". */
#include <math.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { X = 11, Z = 9, J = 6, F = 2 };
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s / %s)\n", __LINE__, #c, fake_mex_last_id, fake_mex_last_msg); return 1; } } while (0)

static int call(int nlhs, mxArray **out, int nrhs, const mxArray **in) {     /* 0: returned, 1: raised */
    if (setjmp(fake_mex_jmp)) return 1;
    mexFunction(nlhs, out, nrhs, in);
    return 0;
}
static mxArray *arr(int m, int n, mxClassID cls) { return mxCreateNumericMatrix((mwSize)m, (mwSize)n, cls, mxREAL); }
static void *stage(const void *h, size_t bytes) {
    void *p = NULL;
    if (qdas_device_malloc(&p, bytes, -1) || qdas_device_copy(p, h, bytes, 0, -1)) return NULL;
    return p;
}
static void put(mxArray *a, const double *v, int n) {                        /* doubles into an array of either class */
    for (int k = 0; k < n; ++k) {
        if (mxGetClassID(a) == mxDOUBLE_CLASS) ((double *)mxGetData(a))[k] = v[k];
        else ((float *)mxGetData(a))[k] = (float)v[k];
    }
}

/* the command against the C ABI for one class, one pair of point strides and one map layout (zx: a Z x X array, strides [Z 1]; otherwise [1 X]) */
static int one(mxClassID cls, int sa, int sb, int zx, const char *dump) {
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4, I = (size_t)X * Z;
    const double xv[X] = {-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5}, zv[Z] = {-4, -3, -2, -1, 0, 1, 2, 3, 4};
    const double av[2 * J] = {-4, 1, 5, -4, -7, 0, 2, 2, NAN, 0, -4.5, 3.25}, bv[2 * J] = {3, -2, 5, 4, -6, 3, 2, 2, 1, 1, 4.75, -3.5};
    mxArray *gsz = arr(1, 8, mxDOUBLE_CLASS), *x = arr(1, X, cls), *z = arr(1, Z, cls), *pa = arr(2, sa ? J : 1, cls), *pb = arr(2, sb ? J : 1, cls);
    mxArray *r = arr(J, F, cls);
    const double g[8] = {X, Z, J, sa, sb, F, zx ? Z : 1, zx ? 1 : X};
    put(gsz, g, 8); put(x, xv, X); put(z, zv, Z); put(pa, av, sa ? 2 * J : 2); put(pb, bv, sb ? 2 * J : 2);
    unsigned s = 7u;
    for (int k = 0; k < J * F; ++k) {
        s = s * 1664525u + 1013904223u;
        const double v = -1.0 + (double)((s >> 8) & 0xffff) / 32768.0;
        if (cls == mxDOUBLE_CLASS) ((double *)mxGetData(r))[k] = v; else ((float *)mxGetData(r))[k] = (float)v;
    }
    mxArray *cb = mxCreateString("raybackproject");
    mxArray *out[3] = {NULL, NULL, NULL};

    qdas_raypaths_desc d;
    memset(&d, 0, sizeof d);
    d.X = X; d.Z = Z; d.J = J; d.F = F; d.xstride = zx ? Z : 1; d.zstride = zx ? 1 : X; d.pa_stride = sa; d.pb_stride = sb;
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32; d.device = -1;
    d.xg = stage(mxGetData(x), X * es); d.zg = stage(mxGetData(z), Z * es);
    d.pa = stage(mxGetData(pa), (sa ? J : 1) * 2 * es); d.pb = stage(mxGetData(pb), (sb ? J : 1) * 2 * es);
    void *dr = stage(mxGetData(r), (size_t)J * F * es), *dg = NULL, *dc = NULL;
    CHECK(d.xg && d.zg && d.pa && d.pb && dr);
    CHECK(!qdas_device_malloc(&dg, I * F * es, -1) && !qdas_device_malloc(&dc, I * es, -1));
    void *hg = malloc(I * F * es), *hc = malloc(I * es);

    /* both outputs */
    const mxArray *a[7] = {cb, gsz, x, z, pa, pb, r};
    CHECK(call(2, out, 7, a) == 0 && out[0] && out[1] && mxGetClassID(out[0]) == cls && mxGetClassID(out[1]) == cls);
    CHECK(mxGetNumberOfElements(out[0]) == I * F && mxGetNumberOfElements(out[1]) == I);
    CHECK(qdas_raypaths_backproject(&d, dr, dg, dc) == 0);
    CHECK(!qdas_device_copy(hg, dg, I * F * es, 1, -1) && !qdas_device_copy(hc, dc, I * es, 1, -1));
    CHECK(memcmp(hg, mxGetData(out[0]), I * F * es) == 0 && memcmp(hc, mxGetData(out[1]), I * es) == 0);
    double total = 0;
    for (size_t k = 0; k < I; ++k) {
        const double c = cls == mxDOUBLE_CLASS ? ((const double *)hc)[k] : (double)((const float *)hc)[k];
        CHECK(c >= 0 && c == c);
        total += c;
    }
    CHECK(total > 0);
    if (sa && sb) CHECK(total > sqrt(58.0));                                  /* ray 0: (-4, 1) -> (3, -2), inside the grid, and others */
    if (dump) {
        FILE *f = fopen(dump, "wb");
        CHECK(f && fwrite(mxGetData(r), 8, (size_t)J * F, f) == (size_t)J * F && fwrite(hg, 8, I * F, f) == I * F && fwrite(hc, 8, I, f) == I);
        fclose(f);
    }
    mxDestroyArray(out[0]); mxDestroyArray(out[1]); out[0] = out[1] = NULL;
    /* one output asked for: one given, the same */
    CHECK(call(1, out, 7, a) == 0 && out[0] && !out[1] && memcmp(hg, mxGetData(out[0]), I * F * es) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;

    /* F = 0: the column sums are the whole job, r may be empty */
    mxArray *none = arr(0, 0, cls);
    const mxArray *a0[7] = {cb, gsz, x, z, pa, pb, none};
    ((double *)mxGetData(gsz))[5] = 0;
    CHECK(call(2, out, 7, a0) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0 && out[1] && memcmp(hc, mxGetData(out[1]), I * es) == 0);
    mxDestroyArray(out[0]); mxDestroyArray(out[1]); out[0] = out[1] = NULL;
    ((double *)mxGetData(gsz))[5] = F;
    /* no rays: zeros, nothing staged */
    ((double *)mxGetData(gsz))[2] = 0;
    CHECK(call(2, out, 7, a) == 0 && out[0] && mxGetNumberOfElements(out[0]) == I * F && out[1] && mxGetNumberOfElements(out[1]) == I);
    for (size_t k = 0; k < I * F * es; ++k) CHECK(((const unsigned char *)mxGetData(out[0]))[k] == 0);
    mxDestroyArray(out[0]); mxDestroyArray(out[1]); out[0] = out[1] = NULL;
    ((double *)mxGetData(gsz))[2] = J;
    /* strides that are not a map's; a grid of one node (the library's text) */
    ((double *)mxGetData(gsz))[6] = Z + 1;
    CHECK(call(1, out, 7, a) == 1 && strstr(fake_mex_last_msg, "strides"));
    ((double *)mxGetData(gsz))[6] = zx ? Z : 1;
    ((double *)mxGetData(gsz))[0] = 1;
    CHECK(call(1, out, 7, a) == 1 && strstr(fake_mex_last_msg, zx ? "2 x 2" : "strides"));
    ((double *)mxGetData(gsz))[0] = X;
    CHECK(call(1, out, 7, a) == 0 && out[0]);
    mxDestroyArray(out[0]);
    free(hg); free(hc);
    qdas_device_free((void *)d.xg, -1); qdas_device_free((void *)d.zg, -1); qdas_device_free((void *)d.pa, -1); qdas_device_free((void *)d.pb, -1);
    qdas_device_free(dr, -1); qdas_device_free(dg, -1); qdas_device_free(dc, -1);
    return 0;
}

int main(int argc, char **argv) {
    if (one(mxDOUBLE_CLASS, 1, 1, 1, argc > 1 ? argv[1] : NULL) || one(mxSINGLE_CLASS, 1, 1, 1, NULL) || one(mxDOUBLE_CLASS, 0, 1, 0, NULL) || one(mxSINGLE_CLASS, 1, 0, 0, NULL)) return 1;
    /* refused: an integer grid, residuals of another class, too few arguments, three outputs */
    mxArray *cb = mxCreateString("raybackproject"), *gsz = arr(1, 8, mxDOUBLE_CLASS), *xi = arr(1, X, mxINT32_CLASS), *xd = arr(1, X, mxDOUBLE_CLASS), *zd = arr(1, Z, mxDOUBLE_CLASS);
    mxArray *pd = arr(2, J, mxDOUBLE_CLASS), *rf = arr(J, F, mxSINGLE_CLASS), *rd = arr(J, F, mxDOUBLE_CLASS), *out[3] = {NULL, NULL, NULL};
    const double g[8] = {X, Z, J, 1, 1, F, Z, 1};
    memcpy(mxGetData(gsz), g, sizeof g);
    const mxArray *r1[7] = {cb, gsz, xi, zd, pd, pd, rd}, *r2[7] = {cb, gsz, xd, zd, pd, pd, rf}, *r3[7] = {cb, gsz, xd, zd, pd, pd, rd};
    CHECK(call(1, out, 7, r1) == 1 && strstr(fake_mex_last_msg, "single or double"));
    CHECK(call(1, out, 7, r2) == 1 && strstr(fake_mex_last_msg, "grid's class"));
    CHECK(call(1, out, 6, r3) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(3, out, 7, r3) == 1 && strstr(fake_mex_last_id, "nargout"));
    printf("raybackproject through the gateway: bit-identical to the C ABI\n");
    printf("raybackproject gateway OK\n");
    return 0;
}
