/* run_adjoint.c -- drives the 'adjoint' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result bit for
 * bit with qdas_adjoint called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  The core shape of tests/test_gpu_adjoint.py: 37 x 5 pixels,
 * 20 elements, 7 steered plane waves, 48 frequencies; the summed image, keep_tx, keep_rx with a_n and a_m, an empty image, a refused class.
 * Prints "adjoint gateway OK". */
#include <math.h>
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { I1 = 37, I2 = 5, NI = I1 * I2, N = 20, V = 7, K = 48 };
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
static int direct(const mxArray **a, int keep_rx, int keep_tx, const mxArray *b) {
    qdas_adjoint_desc d;
    memset(&d, 0, sizeof d);
    d.I = NI; d.N = N; d.M = N; d.V = V; d.Ksel = K; d.cinv_count = 1; d.dtype = QDAS_F32; d.device = -1;
    d.keep_rx = keep_rx; d.keep_tx = keep_tx;
    const size_t nb = (size_t)NI * (keep_rx ? N : 1) * (keep_tx ? V : 1) * 8;
    if (mxGetNumberOfElements(b) * 8 != nb) return 0;
    void *x = stage(mxGetData(a[2]), (size_t)N * V * K * 8), *db = NULL;
    d.freq = (const double *)mxGetData(a[3]);
    d.Pi = (const float *)stage(mxGetData(a[4]), 12 * NI); d.Pr = (const float *)stage(mxGetData(a[5]), 12 * N); d.Pt = (const float *)stage(mxGetData(a[6]), 12 * N);
    d.cinv = (const float *)stage(mxGetData(a[7]), 4);
    d.del_tx = (const double *)stage(mxGetData(a[8]), 8 * N * V); d.apod_tx = (const float *)stage(mxGetData(a[9]), 4 * N * V);
    d.a_n = mxIsEmpty(a[10]) ? NULL : (const float *)stage(mxGetData(a[10]), 4 * NI * N);
    d.a_m = mxIsEmpty(a[11]) ? NULL : (const float *)stage(mxGetData(a[11]), 4 * NI * V);
    if (!x || !d.Pi || !d.Pr || !d.Pt || !d.cinv || !d.del_tx || !d.apod_tx || qdas_device_malloc(&db, nb, -1)) return 0;
    if (qdas_adjoint(&d, x, db, NULL)) return 0;
    float *h = (float *)malloc(nb);
    int ok = qdas_device_copy(h, db, nb, 1, -1) == 0 && memcmp(h, mxGetData(b), nb) == 0;
    double e = 0;
    for (size_t k = 0; k < nb / 4; ++k) { if (h[k] != h[k]) ok = 0; e += (double)h[k] * h[k]; }
    free(h);
    return ok && e > 0;
}

int main(void) {
    const double fs = 20e6, c0 = 1540.0, pi = 3.14159265358979323846;
    mxArray *cmd = mxCreateString("adjoint"), *sz = arr(1, 5, mxDOUBLE_CLASS, 0), *xk = arr(N * V, K, mxSINGLE_CLASS, 1), *f = arr(1, K, mxDOUBLE_CLASS, 0);
    mxArray *Pi = arr(3, NI, mxSINGLE_CLASS, 0), *Pr = arr(3, N, mxSINGLE_CLASS, 0), *cinv = arr(1, 1, mxSINGLE_CLASS, 0);
    mxArray *del = arr(N, V, mxDOUBLE_CLASS, 0), *apod = arr(N, V, mxSINGLE_CLASS, 0), *an = arr(NI, N, mxSINGLE_CLASS, 0), *am = arr(NI, V, mxSINGLE_CLASS, 0);
    mxArray *empty = arr(0, 0, mxDOUBLE_CLASS, 0), *fl = arr(1, 2, mxDOUBLE_CLASS, 0);
    const double szv[5] = {NI, N, N, V, K};
    memcpy(mxGetData(sz), szv, sizeof szv);
    unsigned s = 12345u;
    float *x = (float *)mxGetData(xk);
    for (int k = 0; k < 2 * N * V * K; ++k) { s = s * 1664525u + 1013904223u; x[k] = (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f; }
    for (int k = 0; k < K; ++k) ((double *)mxGetData(f))[k] = k * fs / 96;
    for (int j = 0; j < I2; ++j)
        for (int i = 0; i < I1; ++i) {
            float *p = (float *)mxGetData(Pi) + 3 * (i + I1 * j);
            p[0] = (float)(-1.1e-3 + 0.6e-3 * j); p[1] = 0.f; p[2] = (float)(6e-3 + 6e-3 / 36 * i);
        }
    for (int n = 0; n < N; ++n) { float *p = (float *)mxGetData(Pr) + 3 * n; p[0] = (float)((n - 9.5) * 0.3e-3); p[1] = p[2] = 0.f; }
    ((float *)mxGetData(cinv))[0] = (float)(1.0 / c0);
    for (int v = 0; v < V; ++v)
        for (int n = 0; n < N; ++n) {
            ((double *)mxGetData(del))[n + N * v] = -sin((-10.0 + 20.0 / 6 * v) * pi / 180) * (n - 9.5) * 0.3e-3 / c0;
            ((float *)mxGetData(apod))[n + N * v] = 1.f;
        }
    for (int k = 0; k < NI * N; ++k) ((float *)mxGetData(an))[k] = 0.25f + 0.75f * (float)((k * 7) % 11) / 10.f;
    for (int k = 0; k < NI * V; ++k) ((float *)mxGetData(am))[k] = 0.5f + 0.5f * (float)((k * 5) % 7) / 6.f;
    mxArray *out[1] = {NULL};
    double *flags = (double *)mxGetData(fl);

    /* the summed image */
    const mxArray *a1[13] = {cmd, sz, xk, f, Pi, Pr, Pr, cinv, del, apod, empty, empty, fl};
    CHECK(call(1, out, 13, a1) == 0 && out[0] && mxGetClassID(out[0]) == mxSINGLE_CLASS && mxIsComplex(out[0]));
    CHECK(direct(a1, 0, 0, out[0]));
    mxDestroyArray(out[0]);
    /* keep_tx, with a_m */
    flags[1] = 1;
    const mxArray *a2[13] = {cmd, sz, xk, f, Pi, Pr, Pr, cinv, del, apod, empty, am, fl};
    CHECK(call(1, out, 13, a2) == 0 && direct(a2, 0, 1, out[0]));
    mxDestroyArray(out[0]);
    /* keep_rx, with a_n and a_m */
    flags[0] = 1; flags[1] = 0;
    const mxArray *a3[13] = {cmd, sz, xk, f, Pi, Pr, Pr, cinv, del, apod, an, am, fl};
    CHECK(call(1, out, 13, a3) == 0 && direct(a3, 1, 0, out[0]));
    mxDestroyArray(out[0]);
    flags[0] = 0;
    /* empty in, empty out */
    mxArray *sz0 = arr(1, 5, mxDOUBLE_CLASS, 0);
    const double z0[5] = {0, N, N, V, K};
    memcpy(mxGetData(sz0), z0, sizeof z0);
    const mxArray *e1[13] = {cmd, sz0, xk, f, empty, Pr, Pr, cinv, del, apod, empty, empty, fl};
    CHECK(call(1, out, 13, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]);
    /* a double spectrum is refused, and the next call works */
    mxArray *xd = arr(N * V, K, mxDOUBLE_CLASS, 1);
    const mxArray *r1[13] = {cmd, sz, xd, f, Pi, Pr, Pr, cinv, del, apod, empty, empty, fl};
    CHECK(call(1, out, 13, r1) == 1 && strstr(fake_mex_last_msg, "single complex"));
    CHECK(call(1, out, 13, a1) == 0 && direct(a1, 0, 0, out[0]));
    mxDestroyArray(out[0]);
    printf("adjoint through the gateway: bit-identical to the C ABI\n");
    printf("adjoint gateway OK\n");
    return 0;
}
