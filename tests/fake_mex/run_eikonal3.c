/* run_eikonal3.c -- drives the 'msfm3d' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result bit for
 * bit with qdas_eikonal3 called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  A 19 x 13 x 10 layered speed volume; one point per map,
 * source sets, an empty volume, no points, the reference's range errors, and the pass cap as an error.  With a file name as argument, map 1 of the
 * two-set call is written there.  Prints "eikonal3 gateway OK". */
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { C1 = 19, C2 = 13, C3 = 10, CC = C1 * C2 * C3 };
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

/* the same solve through the C ABI: the speed volume and the work space staged by hand, the maps fetched and compared with the gateway's array */
static int direct(const double *F, const double *src, uint64_t npts, const uint64_t *first, uint64_t K, const mxArray *T) {
    qdas_eikonal3_desc d;
    memset(&d, 0, sizeof d);
    d.C1 = C1; d.C2 = C2; d.C3 = C3; d.K = K; d.npts = npts; d.set_begin = first; d.dp = 1.0; d.base = 1; d.device = -1;
    const size_t cb = sizeof(double) * CC, tb = cb * K;
    if (mxGetNumberOfElements(T) != (size_t)CC * K) return 0;
    uint64_t wb = 0;
    uint32_t passes = 0;
    void *dc = NULL, *dT = NULL, *dw = NULL;
    if (qdas_eikonal3_work_bytes(&d, &wb) || wb == 0) return 0;
    if (qdas_device_malloc(&dc, cb, -1) || qdas_device_copy(dc, F, cb, 0, -1) || qdas_device_malloc(&dT, tb, -1) || qdas_device_malloc(&dw, (size_t)wb, -1)) return 0;
    if (qdas_eikonal3(&d, (const double *)dc, src, (double *)dT, dw, wb, &passes) || passes == 0) return 0;
    double *h = (double *)malloc(tb);
    const int ok = qdas_device_copy(h, dT, tb, 1, -1) == 0 && memcmp(h, mxGetData(T), tb) == 0 && h[0] == h[0];
    free(h);
    qdas_device_free(dc, -1); qdas_device_free(dT, -1); qdas_device_free(dw, -1);
    return ok;
}

int main(int argc, char **argv) {       /* argv[1]: a file that receives map 1 of the two-set call (raw doubles, column-major) */
    mxArray *F = mat(CC, 1, NULL);
    double *f = (double *)mxGetData(F);
    for (int l = 0; l < C3; ++l)
        for (int j = 0; j < C2; ++j)
            for (int i = 0; i < C1; ++i)
                f[i + C1 * (j + C2 * l)] = (i < 6 ? 6.0e6 : (i < 12 ? 5.6e6 : 6.4e6)) + 1.0e5 * ((i * 7 + j * 3 + l * 5) % 5);      /* cells per second */
    const double csz[3] = {C1, C2, C3}, pts[15] = {1.0, 1.0, 1.0, 19.0, 13.0, 10.0, 8.7, 9.2, 5.5, 9.0, 9.0, 9.0, 18.99, 1.5, 3.3};
    mxArray *c_msfm = mxCreateString("msfm3d"), *sz = mat(1, 3, csz), *src = mat(3, 5, pts), *empty = mat(0, 0, NULL);
    mxArray *out[1] = {NULL};

    /* five points, five maps */
    const mxArray *a1[4] = {c_msfm, sz, F, src};
    CHECK(call(1, out, 4, a1) == 0 && out[0] && mxGetClassID(out[0]) == mxDOUBLE_CLASS && !mxIsComplex(out[0]));
    CHECK(direct(f, pts, 5, NULL, 5, out[0]));
    CHECK(((const double *)mxGetData(out[0]))[0] == 0.0);                       /* the first source is node (1, 1, 1) of map 1 */
    mxDestroyArray(out[0]);
    /* the same points as two source sets {1:2}, {3:5} */
    const double fo[3] = {0, 2, 5};
    const uint64_t fu[3] = {0, 2, 5};
    mxArray *first = mat(1, 3, fo);
    const mxArray *a2[5] = {c_msfm, sz, F, src, first};
    CHECK(call(1, out, 5, a2) == 0);
    CHECK(direct(f, pts, 5, fu, 2, out[0]));
    {   /* both points of set 1 are sources of map 1 */
        const double *t = (const double *)mxGetData(out[0]);
        CHECK(t[0] == 0.0 && t[CC - 1] == 0.0);
        if (argc > 1) {
            FILE *fp = fopen(argv[1], "wb");
            CHECK(fp && fwrite(t, sizeof(double), CC, fp) == (size_t)CC && fclose(fp) == 0);
        }
    }
    mxDestroyArray(out[0]);
    /* empty in, empty out: an empty volume, no points */
    const double z0[3] = {C1, 0, C3};
    mxArray *sz0 = mat(1, 3, z0);
    const mxArray *e1[4] = {c_msfm, sz0, empty, src};
    CHECK(call(1, out, 4, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    const mxArray *e2[4] = {c_msfm, sz, F, empty};
    CHECK(call(1, out, 4, e2) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    /* the reference's range errors (kern/msfm.m:96-99) */
    const double lo[3] = {3.0, 0.5, 3.0}, hi[3] = {3.0, 3.0, 10.5};
    mxArray *slo = mat(3, 1, lo), *shi = mat(3, 1, hi);
    const mxArray *r1[4] = {c_msfm, sz, F, slo};
    CHECK(call(1, out, 4, r1) == 1 && !strcmp(fake_mex_last_msg, "Source points must be >= 1 to be within the field."));
    const mxArray *r2[4] = {c_msfm, sz, F, shi};
    CHECK(call(1, out, 4, r2) == 1 && !strcmp(fake_mex_last_msg, "Source points must be <= 10 in dimension 3 to be in the field."));
    /* the pass cap is an error, not a map */
    const double one[1] = {1};
    mxArray *cap = mat(1, 1, one);
    const mxArray *r3[6] = {c_msfm, sz, F, src, empty, cap};
    CHECK(call(1, out, 6, r3) == 1 && strstr(fake_mex_last_msg, "no fixed point within 1 passes"));
    /* ... and the next call works */
    CHECK(call(1, out, 4, a1) == 0 && direct(f, pts, 5, NULL, 5, out[0]));
    mxDestroyArray(out[0]);
    printf("msfm3d through the gateway: bit-identical to the C ABI\n");
    printf("eikonal3 gateway OK\n");
    return 0;
}
