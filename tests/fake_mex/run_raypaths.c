/* run_raypaths.c -- drives the 'wbilerp' and 'rayintegrals' commands of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each
 * result with qdas_raypaths_weights / qdas_raypaths_integrate called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU): the weights and integrals
 * bit for bit, the indices shifted to 1-based with 0 for an empty slot.  The reference's grid (-5:5 x -4:4) with the ray of its example, a vertical ray on the
 * last column, a ray that misses, a point ray and a NaN; double and single; one origin against many end points; an empty call; refused classes.
 * Prints "raypaths gateway OK". */
#include <math.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { X = 11, Z = 9, J = 6, F = 2, K4 = 4 * (X + Z + 1) };
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

/* both commands against the C ABI for one class and one pair of point strides; a = {cmd, gsz, x, z, pa, pb[, maps]} */
static int one(mxClassID cls, int sa, int sb) {
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4;
    const double xv[X] = {-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5}, zv[Z] = {-4, -3, -2, -1, 0, 1, 2, 3, 4};
    const double av[2 * J] = {-4, 1, 5, -4, -7, 0, 2, 2, NAN, 0, -4.5, 3.25}, bv[2 * J] = {3, -2, 5, 4, -6, 3, 2, 2, 1, 1, 4.75, -3.5};
    mxArray *gsz = arr(1, 8, mxDOUBLE_CLASS), *x = arr(1, X, cls), *z = arr(1, Z, cls), *pa = arr(2, sa ? J : 1, cls), *pb = arr(2, sb ? J : 1, cls);
    mxArray *maps = arr(X * Z, F, cls);
    const double g[8] = {X, Z, J, sa, sb, F, Z, 1};
    put(gsz, g, 8); put(x, xv, X); put(z, zv, Z); put(pa, av, sa ? 2 * J : 2); put(pb, bv, sb ? 2 * J : 2);
    unsigned s = 99u;
    for (int k = 0; k < X * Z * F; ++k) { s = s * 1664525u + 1013904223u; const double v = 0.5 + (double)((s >> 8) & 0xffff) / 65536.0; put(maps, &v, 1); if (cls == mxDOUBLE_CLASS) ((double *)mxGetData(maps))[k] = v; else ((float *)mxGetData(maps))[k] = (float)v; }
    mxArray *cw = mxCreateString("wbilerp"), *ci = mxCreateString("rayintegrals");
    mxArray *out[3] = {NULL, NULL, NULL};

    qdas_raypaths_desc d;
    memset(&d, 0, sizeof d);
    d.X = X; d.Z = Z; d.J = J; d.F = F; d.xstride = Z; d.zstride = 1; d.pa_stride = sa; d.pb_stride = sb;
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32; d.device = -1;
    d.xg = stage(mxGetData(x), X * es); d.zg = stage(mxGetData(z), Z * es);
    d.pa = stage(mxGetData(pa), (sa ? J : 1) * 2 * es); d.pb = stage(mxGetData(pb), (sb ? J : 1) * 2 * es);
    void *dm = stage(mxGetData(maps), (size_t)X * Z * F * es), *dw = NULL, *dy = NULL, *dl = NULL;
    int32_t *dix = NULL, *diz = NULL;
    const size_t n = (size_t)K4 * J;
    CHECK(d.xg && d.zg && d.pa && d.pb && dm);
    CHECK(!qdas_device_malloc(&dw, n * es, -1) && !qdas_device_malloc((void **)&dix, n * 4, -1) && !qdas_device_malloc((void **)&diz, n * 4, -1));
    CHECK(!qdas_device_malloc(&dy, (size_t)J * F * es, -1) && !qdas_device_malloc(&dl, J * es, -1));

    /* the triplets */
    const mxArray *a1[6] = {cw, gsz, x, z, pa, pb};
    CHECK(call(3, out, 6, a1) == 0 && out[0] && out[1] && out[2]);
    CHECK(mxGetClassID(out[0]) == cls && mxGetClassID(out[1]) == mxINT32_CLASS && mxGetClassID(out[2]) == mxINT32_CLASS);
    CHECK(mxGetNumberOfElements(out[0]) == n && mxGetNumberOfElements(out[1]) == n && mxGetNumberOfElements(out[2]) == n);
    CHECK(qdas_raypaths_weights(&d, dw, dix, diz) == 0);
    void *hw = malloc(n * es);
    int32_t *hx = (int32_t *)malloc(n * 4), *hz = (int32_t *)malloc(n * 4);
    CHECK(!qdas_device_copy(hw, dw, n * es, 1, -1) && !qdas_device_copy(hx, dix, n * 4, 1, -1) && !qdas_device_copy(hz, diz, n * 4, 1, -1));
    CHECK(memcmp(hw, mxGetData(out[0]), n * es) == 0);
    size_t used = 0;
    double sum0 = 0;
    for (size_t k = 0; k < n; ++k) {
        const int32_t gx = ((const int32_t *)mxGetData(out[1]))[k], gz = ((const int32_t *)mxGetData(out[2]))[k];
        CHECK(gx == hx[k] + 1 && gz == hz[k] + 1 && gx >= 0 && gx <= X && gz >= 0 && gz <= Z && (gx == 0) == (gz == 0));
        used += gx != 0;
        if (k < (size_t)K4) sum0 += cls == mxDOUBLE_CLASS ? ((const double *)hw)[k] : (double)((const float *)hw)[k];
    }
    CHECK(used > 0 && used % 4 == 0);
    if (sa && sb) CHECK(fabs(sum0 - sqrt(58.0)) < (cls == mxDOUBLE_CLASS ? 1e-13 : 1e-5));      /* ray 0: (-4, 1) -> (3, -2), inside the grid */
    for (int k = 0; k < 3; ++k) { mxDestroyArray(out[k]); out[k] = NULL; }
    /* one output asked for: one given */
    CHECK(call(1, out, 6, a1) == 0 && out[0] && !out[1]);
    mxDestroyArray(out[0]); out[0] = NULL;

    /* the integrals */
    const mxArray *a2[7] = {ci, gsz, x, z, pa, pb, maps};
    CHECK(call(2, out, 7, a2) == 0 && out[0] && out[1] && mxGetClassID(out[0]) == cls && mxGetClassID(out[1]) == cls);
    CHECK(mxGetNumberOfElements(out[0]) == (size_t)J * F && mxGetNumberOfElements(out[1]) == (size_t)J);
    CHECK(qdas_raypaths_integrate(&d, dm, dy, dl) == 0);
    void *hy = malloc((size_t)J * F * es), *hl = malloc(J * es);
    CHECK(!qdas_device_copy(hy, dy, (size_t)J * F * es, 1, -1) && !qdas_device_copy(hl, dl, J * es, 1, -1));
    CHECK(memcmp(hy, mxGetData(out[0]), (size_t)J * F * es) == 0 && memcmp(hl, mxGetData(out[1]), J * es) == 0);
    const double l0 = cls == mxDOUBLE_CLASS ? ((const double *)hl)[0] : (double)((const float *)hl)[0];
    CHECK(l0 > 0);
    mxDestroyArray(out[0]); mxDestroyArray(out[1]); out[0] = out[1] = NULL;

    /* no rays: empty results, nothing staged */
    ((double *)mxGetData(gsz))[2] = 0;
    CHECK(call(3, out, 6, a1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0 && out[2] && mxGetNumberOfElements(out[2]) == 0);
    for (int k = 0; k < 3; ++k) { mxDestroyArray(out[k]); out[k] = NULL; }
    CHECK(call(2, out, 7, a2) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0 && out[1]);
    mxDestroyArray(out[0]); mxDestroyArray(out[1]); out[0] = out[1] = NULL;
    ((double *)mxGetData(gsz))[2] = J;
    /* strides that leave the map; a grid of one node (the library's text) */
    ((double *)mxGetData(gsz))[6] = Z + 1;
    CHECK(call(1, out, 7, a2) == 1 && strstr(fake_mex_last_msg, "strides"));
    ((double *)mxGetData(gsz))[6] = Z;
    ((double *)mxGetData(gsz))[0] = 1;
    CHECK(call(1, out, 6, a1) == 1 && strstr(fake_mex_last_msg, "2 x 2"));
    ((double *)mxGetData(gsz))[0] = X;
    CHECK(call(1, out, 6, a1) == 0 && out[0]);
    mxDestroyArray(out[0]);
    free(hw); free(hx); free(hz); free(hy); free(hl);
    qdas_device_free((void *)d.xg, -1); qdas_device_free((void *)d.zg, -1); qdas_device_free((void *)d.pa, -1); qdas_device_free((void *)d.pb, -1);
    qdas_device_free(dm, -1); qdas_device_free(dw, -1); qdas_device_free(dix, -1); qdas_device_free(diz, -1); qdas_device_free(dy, -1); qdas_device_free(dl, -1);
    return 0;
}

int main(void) {
    if (one(mxDOUBLE_CLASS, 1, 1) || one(mxSINGLE_CLASS, 1, 1) || one(mxDOUBLE_CLASS, 0, 1) || one(mxSINGLE_CLASS, 1, 0)) return 1;
    /* refused: an integer grid, end points of another class, four outputs */
    mxArray *cw = mxCreateString("wbilerp"), *gsz = arr(1, 5, mxDOUBLE_CLASS), *xi = arr(1, X, mxINT32_CLASS), *xd = arr(1, X, mxDOUBLE_CLASS), *zd = arr(1, Z, mxDOUBLE_CLASS);
    mxArray *pf = arr(2, J, mxSINGLE_CLASS), *pd = arr(2, J, mxDOUBLE_CLASS), *out[4] = {NULL, NULL, NULL, NULL};
    const double g[5] = {X, Z, J, 1, 1};
    memcpy(mxGetData(gsz), g, sizeof g);
    const mxArray *r1[6] = {cw, gsz, xi, zd, pd, pd}, *r2[6] = {cw, gsz, xd, zd, pf, pd}, *r3[6] = {cw, gsz, xd, zd, pd, pd};
    CHECK(call(1, out, 6, r1) == 1 && strstr(fake_mex_last_msg, "single or double"));
    CHECK(call(1, out, 6, r2) == 1 && strstr(fake_mex_last_msg, "one class"));
    CHECK(call(4, out, 6, r3) == 1 && strstr(fake_mex_last_id, "nargout"));
    printf("wbilerp and rayintegrals through the gateway: bit-identical to the C ABI\n");
    printf("raypaths gateway OK\n");
    return 0;
}
