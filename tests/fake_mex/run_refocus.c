/* run_refocus.c -- drives the 'refocus' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result bit for bit
 * with qdas_refocus called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  A shape of tests/test_gpu_refocus.py: 48 samples x 3 receivers x
 * 8 pulses -> 8 elements; one t0 and one frame, a t0 per pulse and two frames, an empty problem, a refused class, a length the in-LDS kernels do not take.
 * Prints "refocus gateway OK". */
#include <math.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { T = 48, N = 3, V = 8, M = 8, FR = 2 };
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

/* the same call through the C ABI: every array staged by hand, y fetched and compared with the gateway's array.  a = {cmd, sizes, x, Hi, t0, fs} */
static int direct(const mxArray **a, int frames, const mxArray *y) {
    qdas_refocus_desc d;
    memset(&d, 0, sizeof d);
    const double *t0 = (const double *)mxGetData(a[4]);
    const size_t nt0 = mxGetNumberOfElements(a[4]);
    d.T = T; d.N = N; d.V = V; d.M = M; d.frames = (uint64_t)frames;
    d.fs = *(const double *)mxGetData(a[5]); d.device = -1; d.one_t0 = nt0 == 1;
    d.t0_out = t0[0];
    for (size_t v = 1; v < nt0; ++v) if (t0[v] < d.t0_out) d.t0_out = t0[v];
    const size_t nb = (size_t)T * N * M * frames * 8;
    if (mxGetNumberOfElements(y) * 8 != nb) return 0;
    uint64_t wb = 0;
    if (qdas_refocus_work_bytes(&d, &wb) || !wb) return 0;
    void *x = stage(mxGetData(a[2]), (size_t)T * N * V * frames * 8), *Hi = stage(mxGetData(a[3]), (size_t)M * V * T * 8), *dy = NULL, *work = NULL;
    if (!d.one_t0) d.t0 = (const double *)stage(t0, 8 * nt0);
    if (!x || !Hi || (!d.one_t0 && !d.t0) || qdas_device_malloc(&dy, nb, -1) || qdas_device_malloc(&work, (size_t)wb, -1)) return 0;
    if (qdas_refocus(&d, x, Hi, dy, work, wb)) return 0;
    float *h = (float *)malloc(nb);
    int ok = qdas_device_copy(h, dy, nb, 1, -1) == 0 && memcmp(h, mxGetData(y), nb) == 0;
    double e = 0;
    for (size_t k = 0; k < nb / 4; ++k) { if (h[k] != h[k]) ok = 0; e += (double)h[k] * h[k]; }
    free(h);
    return ok && e > 0;
}

int main(void) {
    mxArray *cmd = mxCreateString("refocus"), *sz = arr(1, 5, mxDOUBLE_CLASS, 0), *x1 = arr(T * N, V, mxSINGLE_CLASS, 1), *x2 = arr(T * N, V * FR, mxSINGLE_CLASS, 1);
    mxArray *Hi = arr(M * V, T, mxSINGLE_CLASS, 1), *t1 = arr(1, 1, mxDOUBLE_CLASS, 0), *tv = arr(1, V, mxDOUBLE_CLASS, 0), *fs = arr(1, 1, mxDOUBLE_CLASS, 0);
    mxArray *empty = arr(0, 0, mxSINGLE_CLASS, 1);
    double *szv = (double *)mxGetData(sz);
    const double sz1[5] = {T, N, V, M, 1};
    memcpy(szv, sz1, sizeof sz1);
    *(double *)mxGetData(fs) = 20e6;
    *(double *)mxGetData(t1) = 1.3e-6;
    for (int v = 0; v < V; ++v) ((double *)mxGetData(tv))[v] = 1.3e-6 + ((V - 1 - v) * 0.37 + 0.21) / 20e6;
    unsigned s = 4321u;
    float *p = (float *)mxGetData(x2);
    for (int k = 0; k < 2 * T * N * V * FR; ++k) { s = s * 1664525u + 1013904223u; p[k] = (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f; }
    memcpy(mxGetData(x1), p, (size_t)T * N * V * 8);
    p = (float *)mxGetData(Hi);
    for (int k = 0; k < 2 * M * V * T; ++k) { s = s * 1664525u + 1013904223u; p[k] = ((float)((s >> 8) & 0xffff) / 32768.0f - 1.0f) * 0.35f; }
    mxArray *out[1] = {NULL};

    /* one t0, one frame */
    const mxArray *a1[6] = {cmd, sz, x1, Hi, t1, fs};
    CHECK(call(1, out, 6, a1) == 0 && out[0] && mxGetClassID(out[0]) == mxSINGLE_CLASS && mxIsComplex(out[0]));
    CHECK(direct(a1, 1, out[0]));
    mxDestroyArray(out[0]);
    /* a t0 per pulse, two frames */
    szv[4] = FR;
    const mxArray *a2[6] = {cmd, sz, x2, Hi, tv, fs};
    CHECK(call(1, out, 6, a2) == 0 && direct(a2, FR, out[0]));
    mxDestroyArray(out[0]);
    szv[4] = 1;
    /* empty in, empty out */
    szv[0] = 0;
    const mxArray *e1[6] = {cmd, sz, empty, empty, t1, fs};
    CHECK(call(1, out, 6, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    szv[0] = T;
    /* double data is refused; three t0 values for eight pulses too; a length with the radix 17 raises the library's text; and the next call works */
    mxArray *xd = arr(T * N, V, mxDOUBLE_CLASS, 1), *t3 = arr(1, 3, mxDOUBLE_CLASS, 0);
    const mxArray *r1[6] = {cmd, sz, xd, Hi, t1, fs}, *r2[6] = {cmd, sz, x1, Hi, t3, fs};
    CHECK(call(1, out, 6, r1) == 1 && strstr(fake_mex_last_msg, "single complex"));
    CHECK(call(1, out, 6, r2) == 1 && strstr(fake_mex_last_msg, "one per pulse"));
    szv[0] = 34;
    CHECK(call(1, out, 6, a1) == 1 && strstr(fake_mex_last_msg, "in-LDS"));
    szv[0] = T;
    CHECK(call(1, out, 6, a1) == 0 && direct(a1, 1, out[0]));
    mxDestroyArray(out[0]);
    printf("refocus through the gateway: bit-identical to the C ABI\n");
    printf("refocus gateway OK\n");
    return 0;
}
