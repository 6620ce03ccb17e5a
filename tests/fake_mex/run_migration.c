/* run_migration.c -- drives the 'migration' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result bit
 * for bit with qdas_migration called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  A padded shape of tests/test_gpu_migration.py:
 * 48 samples x 12 elements x 3 plane waves, Nfft = [96, 24]; the summed image, keep_tx with two frames, an empty problem, a refused class, a length
 * the in-LDS kernels do not take.  Prints "migration gateway OK". */
#include <math.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { T = 48, N = 12, M = 3, FR = 2, F = 96, K = 24 };
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s / %s)\n", __LINE__, #c, fake_mex_last_id, fake_mex_last_msg); return 1; } } while (0)

static int call(int nlhs, mxArray **out, int nrhs, const mxArray **in) {     /* 0: returned, 1: raised */
    if (setjmp(fake_mex_jmp)) return 1;
    mexFunction(nlhs, out, nrhs, in);
    return 0;
}
static mxArray *arr(int m, int n, mxClassID cls, int cplx) { return mxCreateNumericMatrix((mwSize)m, (mwSize)n, cls, cplx ? mxCOMPLEX : mxREAL); }
static void *stage(const void *h, size_t bytes) {
    void *p = NULL;
    if (qdas_device_malloc(&p, bytes, -1) || qdas_device_copy(p, h, bytes, 0, -1)) return NULL;
    return p;
}

/* the same call through the C ABI: every array staged by hand, b fetched and compared with the gateway's array */
static int direct(const mxArray **a, int frames, int keep_tx, const mxArray *b) {
    qdas_migration_desc d;
    memset(&d, 0, sizeof d);
    const double *p = (const double *)mxGetData(a[5]);
    d.T = T; d.N = N; d.M = M; d.frames = (uint64_t)frames; d.F = F; d.K = K;
    d.fs = p[0]; d.fmod = p[1]; d.t0 = p[2]; d.c0 = p[3]; d.pitch = p[4];
    d.flag = 2; d.keep_tx = keep_tx; d.jacobian = 1; d.device = -1;
    const size_t nb = (size_t)T * N * (keep_tx ? M : 1) * frames * 8;
    if (mxGetNumberOfElements(b) * 8 != nb) return 0;
    void *x = stage(mxGetData(a[2]), (size_t)T * N * M * frames * 8), *db = NULL;
    d.tau = (const double *)stage(mxGetData(a[3]), 8 * N * M);
    d.gamma = (const double *)stage(mxGetData(a[4]), 8 * M);
    if (!x || !d.tau || !d.gamma || qdas_device_malloc(&db, nb, -1)) return 0;
    if (qdas_migration(&d, x, db, NULL)) return 0;
    float *h = (float *)malloc(nb);
    int ok = qdas_device_copy(h, db, nb, 1, -1) == 0 && memcmp(h, mxGetData(b), nb) == 0;
    double e = 0;
    for (size_t k = 0; k < nb / 4; ++k) { if (h[k] != h[k]) ok = 0; e += (double)h[k] * h[k]; }
    free(h);
    return ok && e > 0;
}

int main(void) {
    const double c0 = 1540.0, pitch = 0.3e-3, pi = 3.14159265358979323846, ang[M] = {-3.0, 0.0, 5.0};
    mxArray *cmd = mxCreateString("migration"), *sz = arr(1, 6, mxDOUBLE_CLASS, 0), *x1 = arr(T * N, M, mxSINGLE_CLASS, 1), *x2 = arr(T * N, M * FR, mxSINGLE_CLASS, 1);
    mxArray *tau = arr(N, M, mxDOUBLE_CLASS, 0), *gam = arr(1, M, mxDOUBLE_CLASS, 0), *par = arr(1, 5, mxDOUBLE_CLASS, 0), *fl = arr(1, 3, mxDOUBLE_CLASS, 0);
    mxArray *empty = arr(0, 0, mxSINGLE_CLASS, 1);
    double *szv = (double *)mxGetData(sz);
    const double sz1[6] = {T, N, M, 1, F, K}, pv[5] = {20e6, 2.5e6, 1.3e-6, c0, pitch}, f0[3] = {2, 0, 1};
    memcpy(szv, sz1, sizeof sz1);
    memcpy(mxGetData(par), pv, sizeof pv);
    memcpy(mxGetData(fl), f0, sizeof f0);
    unsigned s = 4321u;
    float *v = (float *)mxGetData(x2);
    for (int k = 0; k < 2 * T * N * M * FR; ++k) { s = s * 1664525u + 1013904223u; v[k] = (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f; }
    memcpy(mxGetData(x1), v, (size_t)T * N * M * 8);
    for (int m = 0; m < M; ++m) {
        const double th = ang[m] * pi / 180;
        ((double *)mxGetData(gam))[m] = sin(th) / (2 - cos(th));
        for (int n = 0; n < N; ++n) ((double *)mxGetData(tau))[n + N * m] = -sin(th) * (n - 5.5) * pitch / c0;
    }
    mxArray *out[1] = {NULL};
    double *flags = (double *)mxGetData(fl);

    /* the summed image */
    const mxArray *a1[7] = {cmd, sz, x1, tau, gam, par, fl};
    CHECK(call(1, out, 7, a1) == 0 && out[0] && mxGetClassID(out[0]) == mxSINGLE_CLASS && mxIsComplex(out[0]));
    CHECK(direct(a1, 1, 0, out[0]));
    mxDestroyArray(out[0]);
    /* keep_tx, two frames */
    flags[1] = 1; szv[3] = FR;
    const mxArray *a2[7] = {cmd, sz, x2, tau, gam, par, fl};
    CHECK(call(1, out, 7, a2) == 0 && direct(a2, FR, 1, out[0]));
    mxDestroyArray(out[0]);
    flags[1] = 0; szv[3] = 1;
    /* empty in, empty out */
    szv[0] = 0;
    const mxArray *e1[7] = {cmd, sz, empty, tau, gam, par, fl};
    CHECK(call(1, out, 7, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    szv[0] = T;
    /* double data is refused; a length with the radix 17 raises the library's text; and the next call works */
    mxArray *xd = arr(T * N, M, mxDOUBLE_CLASS, 1);
    const mxArray *r1[7] = {cmd, sz, xd, tau, gam, par, fl};
    CHECK(call(1, out, 7, r1) == 1 && strstr(fake_mex_last_msg, "single complex"));
    szv[4] = 68;
    CHECK(call(1, out, 7, a1) == 1 && strstr(fake_mex_last_msg, "in-LDS"));
    szv[4] = F;
    CHECK(call(1, out, 7, a1) == 0 && direct(a1, 1, 0, out[0]));
    mxDestroyArray(out[0]);
    printf("migration through the gateway: bit-identical to the C ABI\n");
    printf("migration gateway OK\n");
    return 0;
}
