/* run_coherence.c -- drives the 'slsc', 'dmas', 'cohfac' and 'pcf' commands of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so,
 * and compares each result bit for bit with qdas_coherence called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  The image is
 * A x N x B x K column-major (a time kernel K behind the aperture), complex single; also pcf with one output and an empty image.  Prints "coherence gateway OK". */
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { A = 37, N = 24, B = 3, K = 2 };
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s / %s)\n", __LINE__, #c, fake_mex_last_id, fake_mex_last_msg); return 1; } } while (0)

static int call(int nlhs, mxArray **out, int nrhs, const mxArray **in) {     /* 0: returned, 1: raised */
    if (setjmp(fake_mex_jmp)) return 1;
    mexFunction(nlhs, out, nrhs, in);
    return 0;
}
static mxArray *row(int n, const double *v) {
    mxArray *a = mxCreateNumericMatrix(1, (mwSize)n, mxDOUBLE_CLASS, mxREAL);
    memcpy(mxGetData(a), v, sizeof(double) * (size_t)n);
    return a;
}

/* the same call through the C ABI: x staged by hand, y (and pcf's sf) fetched, compared with the gateway's arrays */
static int direct(int method, int kk, int kpix, const int64_t *lags, uint64_t nlags, uint64_t lo, uint64_t hi, const float *xh, const mxArray *y, const mxArray *y2) {
    qdas_coherence_desc d;
    memset(&d, 0, sizeof d);
    d.method = method; d.dtype = QDAS_F32; d.cplx = 1; d.device = -1; d.gamma = 1.0;
    d.N = N; d.K = (uint64_t)kk; d.strideN = A; d.strideK = A * N * B;
    d.size[0] = A; d.stride[0] = 1; d.size[1] = B; d.stride[1] = A * N; d.size[2] = kpix ? K : 1; d.stride[2] = kpix ? A * N * B : 0;   /* kpix: K is an image dimension */
    d.lag_lo = lo; d.lag_hi = hi; d.lags = lags; d.nlags = nlags;
    const size_t xb = sizeof(float) * 2 * A * N * B * K, P = (size_t)A * B * (kpix ? K : 1);
    const int cy = method != QDAS_COH_COHFAC && method != QDAS_COH_PCF;
    void *dx = NULL, *dy = NULL, *dy2 = NULL;
    if (qdas_device_malloc(&dx, xb, -1) || qdas_device_copy(dx, xh, xb, 0, -1) || qdas_device_malloc(&dy, P * 4 * (cy ? 2 : 1), -1)) return 0;
    if (method == QDAS_COH_PCF && qdas_device_malloc(&dy2, P * 4, -1)) return 0;
    if (qdas_coherence(&d, dx, dy, dy2, NULL)) return 0;
    float *h = (float *)malloc(P * 4 * 2), *h2 = (float *)malloc(P * 4);
    int ok = qdas_device_copy(h, dy, P * 4 * (cy ? 2 : 1), 1, -1) == 0 && memcmp(h, mxGetData(y), P * 4 * (cy ? 2 : 1)) == 0;
    if (ok && dy2) ok = qdas_device_copy(h2, dy2, P * 4, 1, -1) == 0 && memcmp(h2, mxGetData(y2), P * 4) == 0;
    free(h); free(h2);
    qdas_device_free(dx, -1); qdas_device_free(dy, -1);
    if (dy2) qdas_device_free(dy2, -1);
    return ok;
}

int main(void) {
    const mwSize xd[4] = {A, N, B, K};
    mxArray *x = mxCreateNumericArray(4, xd, mxSINGLE_CLASS, mxCOMPLEX);
    float *xp = (float *)mxGetData(x);
    srand(11);
    for (size_t k = 0; k < (size_t)2 * A * N * B * K; ++k) xp[k] = (float)rand() / RAND_MAX - 0.5f;
    const double k1[6] = {A, N, B, 1, K, 0}, k2[6] = {A, N, B, K, 1, 0}, l05[2] = {0, 5}, l3[1] = {3};
    mxArray *ksz1 = row(6, k1), *ksz2 = row(6, k2), *L05 = row(2, l05), *L3 = row(1, l3), *empty = mxCreateNumericMatrix(0, 0, mxDOUBLE_CLASS, mxREAL);
    mxArray *c_slsc = mxCreateString("slsc"), *c_dmas = mxCreateString("dmas"), *c_coh = mxCreateString("cohfac"), *c_pcf = mxCreateString("pcf");
    mxArray *avg = mxCreateString("average"), *ens = mxCreateString("ensemble");
    const int64_t t05[2] = {0, 5};
    mxArray *out[2] = {NULL, NULL};

    /* slsc, average, default lags; the time kernel K behind the image (ksz1 treats it as an image dimension, ksz2 as slsc's kdim) */
    const mxArray *a1[5] = {c_slsc, ksz1, x, empty, avg};
    CHECK(call(1, out, 5, a1) == 0 && mxIsComplex(out[0]) && mxGetNumberOfElements(out[0]) == (size_t)A * B * K);
    CHECK(direct(QDAS_COH_SLSC_AVERAGE, 1, 1, NULL, 0, 1, N / 4, xp, out[0], NULL));
    mxDestroyArray(out[0]);
    const mxArray *a2[5] = {c_slsc, ksz2, x, L05, ens};
    CHECK(call(1, out, 5, a2) == 0);
    CHECK(direct(QDAS_COH_SLSC_ENSEMBLE, K, 0, t05, 2, 0, 0, xp, out[0], NULL));
    mxDestroyArray(out[0]);
    const mxArray *a3[5] = {c_slsc, ksz2, x, L3, avg};
    CHECK(call(1, out, 5, a3) == 0);
    CHECK(direct(QDAS_COH_SLSC_AVERAGE, K, 0, NULL, 0, 1, 3, xp, out[0], NULL));
    mxDestroyArray(out[0]);
    /* dmas over the aperture (K = 1: ksz = [A N B*K]) */
    const double k3[3] = {A, N, B * K};
    mxArray *ksz3 = row(3, k3);
    const mxArray *a4[4] = {c_dmas, ksz3, x, empty};
    CHECK(call(1, out, 4, a4) == 0);
    {   /* (the direct call sees the same B*K columns as one pixel group of stride A N) */
        qdas_coherence_desc d;
        memset(&d, 0, sizeof d);
        d.method = QDAS_COH_DMAS; d.dtype = QDAS_F32; d.cplx = 1; d.device = -1; d.N = N; d.K = 1; d.strideN = A;
        d.size[0] = A; d.stride[0] = 1; d.size[1] = B * K; d.stride[1] = A * N; d.size[2] = 1; d.lag_lo = 1; d.lag_hi = N - 1;
        const size_t xb = sizeof(float) * 2 * A * N * B * K, yb = sizeof(float) * 2 * A * B * K;
        void *dx = NULL, *dy = NULL;
        CHECK(qdas_device_malloc(&dx, xb, -1) == 0 && qdas_device_copy(dx, xp, xb, 0, -1) == 0 && qdas_device_malloc(&dy, yb, -1) == 0);
        CHECK(qdas_coherence(&d, dx, dy, NULL, NULL) == 0);
        float *h = (float *)malloc(yb);
        CHECK(qdas_device_copy(h, dy, yb, 1, -1) == 0 && memcmp(h, mxGetData(out[0]), yb) == 0);
        free(h); qdas_device_free(dx, -1); qdas_device_free(dy, -1);
    }
    mxDestroyArray(out[0]);
    /* cohfac over the aperture and the time kernel */
    const mxArray *a5[3] = {c_coh, ksz2, x};
    CHECK(call(1, out, 3, a5) == 0 && !mxIsComplex(out[0]));
    CHECK(direct(QDAS_COH_COHFAC, K, 0, NULL, 0, 0, 0, xp, out[0], NULL));
    mxDestroyArray(out[0]);
    /* pcf: two outputs */
    const mxArray *a6[4] = {c_pcf, ksz1, x, empty};
    CHECK(call(2, out, 4, a6) == 0 && out[1] && !mxIsComplex(out[1]));
    CHECK(direct(QDAS_COH_PCF, 1, 1, NULL, 0, 0, 0, xp, out[0], out[1]));
    mxArray *w2 = out[0];
    mxDestroyArray(out[1]);
    /* pcf with one output (w = qdas_mex('pcf', ...)): one slot is all MATLAB provides; w is the same */
    mxArray *one[1] = {NULL};
    CHECK(call(1, one, 4, a6) == 0 && one[0] && memcmp(mxGetData(one[0]), mxGetData(w2), sizeof(float) * A * B * K) == 0);
    mxDestroyArray(one[0]); mxDestroyArray(w2);
    /* an empty image (B = 0): empty results, nothing launched */
    const double k0[6] = {A, N, 0, 1, K, 0};
    mxArray *ksz0 = row(6, k0), *x0 = mxCreateNumericArray(2, (const mwSize[2]){0, 0}, mxSINGLE_CLASS, mxCOMPLEX);
    const mxArray *z1[5] = {c_slsc, ksz0, x0, empty, avg};
    CHECK(call(1, out, 5, z1) == 0 && mxGetNumberOfElements(out[0]) == 0 && mxIsComplex(out[0]));
    mxDestroyArray(out[0]);
    const mxArray *z2[4] = {c_pcf, ksz0, x0, empty};
    out[0] = out[1] = NULL;
    CHECK(call(2, out, 4, z2) == 0 && mxGetNumberOfElements(out[0]) == 0 && out[1] && mxGetNumberOfElements(out[1]) == 0);
    mxDestroyArray(out[0]); mxDestroyArray(out[1]);
    /* errors: pcf of real data, a bad method, too many outputs */
    mxArray *xr = mxCreateNumericArray(4, xd, mxSINGLE_CLASS, mxREAL);
    const mxArray *e1[4] = {c_pcf, ksz1, xr, empty};
    CHECK(call(2, out, 4, e1) == 1 && !strcmp(fake_mex_last_id, "QUPS:pcf:realInput"));
    mxArray *bogus = mxCreateString("bogus");
    const mxArray *e2[5] = {c_slsc, ksz1, x, empty, bogus};
    CHECK(call(1, out, 5, e2) == 1);
    const mxArray *e3[3] = {c_coh, ksz2, x};
    CHECK(call(2, out, 3, e3) == 1);
    printf("slsc / dmas / cohfac / pcf through the gateway: bit-identical to the C ABI\n");
    printf("coherence gateway OK\n");
    return 0;
}
