/* run_eikonal.c -- drives the 'msfm' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result bit for
 * bit with qdas_eikonal called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  A 45 x 37 layered speed map; one point per map, source
 * sets, an empty map, no points, the reference's range errors, and the pass cap as an error.  Prints "eikonal gateway OK". */
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { C1 = 45, C2 = 37 };
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s / %s)\n", __LINE__, #c, fake_mex_last_id, fake_mex_last_msg); return 1; } } while (0)

static int call(int nlhs, mxArray **out, int nrhs, const mxArray **in) {     /* 0: returned, 1: raised */
    if (setjmp(fake_mex_jmp)) return 1;
    mexFunction(nlhs, out, nrhs, in);
    return 0;
}
static mxArray *mat(int m, int n, const double *v) {
    mxArray *a = mxCreateNumericMatrix((mwSize)m, (mwSize)n, mxDOUBLE_CLASS, mxREAL);
    if (v) memcpy(mxGetData(a), v, sizeof(double) * (size_t)m * (size_t)n);
    return a;
}

/* the same solve through the C ABI: the speed map staged by hand, the maps fetched and compared with the gateway's array */
static int direct(const double *F, const double *src, uint64_t npts, const uint64_t *first, uint64_t K, const mxArray *T) {
    qdas_eikonal_desc d;
    memset(&d, 0, sizeof d);
    d.C1 = C1; d.C2 = C2; d.K = K; d.npts = npts; d.set_begin = first; d.dp = 1.0; d.base = 1; d.device = -1;
    const size_t cb = sizeof(double) * C1 * C2, tb = cb * K;
    if (mxGetNumberOfElements(T) != (size_t)C1 * C2 * K) return 0;
    void *dc = NULL, *dT = NULL;
    if (qdas_device_malloc(&dc, cb, -1) || qdas_device_copy(dc, F, cb, 0, -1) || qdas_device_malloc(&dT, tb, -1)) return 0;
    if (qdas_eikonal(&d, (const double *)dc, src, (double *)dT, NULL)) return 0;
    double *h = (double *)malloc(tb);
    const int ok = qdas_device_copy(h, dT, tb, 1, -1) == 0 && memcmp(h, mxGetData(T), tb) == 0 && h[0] == h[0];
    free(h);
    qdas_device_free(dc, -1); qdas_device_free(dT, -1);
    return ok;
}

int main(void) {
    mxArray *F = mat(C1, C2, NULL);
    double *f = (double *)mxGetData(F);
    for (int j = 0; j < C2; ++j)
        for (int i = 0; i < C1; ++i) f[i + C1 * j] = (i < 15 ? 6.0e6 : (i < 30 ? 5.6e6 : 6.4e6)) + 1.0e5 * ((i * 7 + j * 3) % 5);      /* cells per second */
    const double csz[2] = {C1, C2}, pts[10] = {1.0, 1.0, 45.0, 37.0, 20.7, 5.2, 3.3, 30.9, 44.99, 1.5};
    mxArray *c_msfm = mxCreateString("msfm"), *sz = mat(1, 2, csz), *src = mat(2, 5, pts), *empty = mat(0, 0, NULL);
    mxArray *out[1] = {NULL};

    /* five points, five maps */
    const mxArray *a1[4] = {c_msfm, sz, F, src};
    CHECK(call(1, out, 4, a1) == 0 && out[0] && mxGetClassID(out[0]) == mxDOUBLE_CLASS && !mxIsComplex(out[0]));
    CHECK(direct(f, pts, 5, NULL, 5, out[0]));
    CHECK(((const double *)mxGetData(out[0]))[0] == 0.0);                       /* the first source is node (1, 1) of map 1 */
    mxDestroyArray(out[0]);
    /* the same points as two source sets {1:2}, {3:5} (a cell of the caller) */
    const double fo[3] = {0, 2, 5};
    const uint64_t fu[3] = {0, 2, 5};
    mxArray *first = mat(1, 3, fo);
    const mxArray *a2[5] = {c_msfm, sz, F, src, first};
    CHECK(call(1, out, 5, a2) == 0);
    CHECK(direct(f, pts, 5, fu, 2, out[0]));
    {   /* both points of set 1 are sources of map 1 */
        const double *t = (const double *)mxGetData(out[0]);
        CHECK(t[0] == 0.0 && t[(C1 - 1) + C1 * (C2 - 1)] == 0.0);
    }
    mxDestroyArray(out[0]);
    /* empty in, empty out: an empty map, no points */
    const double z0[2] = {0, C2};
    mxArray *sz0 = mat(1, 2, z0);
    const mxArray *e1[4] = {c_msfm, sz0, empty, src};
    CHECK(call(1, out, 4, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    const mxArray *e2[4] = {c_msfm, sz, F, empty};
    CHECK(call(1, out, 4, e2) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    /* the reference's range errors (kern/msfm.m:96-99) */
    const double lo[2] = {0.5, 3.0}, hi[2] = {3.0, 37.5};
    mxArray *slo = mat(2, 1, lo), *shi = mat(2, 1, hi);
    const mxArray *r1[4] = {c_msfm, sz, F, slo};
    CHECK(call(1, out, 4, r1) == 1 && !strcmp(fake_mex_last_msg, "Source points must be >= 1 to be within the field."));
    const mxArray *r2[4] = {c_msfm, sz, F, shi};
    CHECK(call(1, out, 4, r2) == 1 && !strcmp(fake_mex_last_msg, "Source points must be <= 37 in dimension 2 to be in the field."));
    /* the pass cap is an error, not a map */
    const double one[1] = {1};
    mxArray *cap = mat(1, 1, one);
    const mxArray *r3[6] = {c_msfm, sz, F, src, empty, cap};
    CHECK(call(1, out, 6, r3) == 1 && strstr(fake_mex_last_msg, "no fixed point within 1 passes"));
    /* ... and the next call works */
    CHECK(call(1, out, 4, a1) == 0 && direct(f, pts, 5, NULL, 5, out[0]));
    mxDestroyArray(out[0]);
    printf("msfm through the gateway: bit-identical to the C ABI\n");
    printf("eikonal gateway OK\n");
    return 0;
}
