/* run_pwznxcorr.c -- drives the 'pwznxcorr' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so, and compares each result bit for
 * bit with qdas_pwznxcorr called directly on device arrays (TEST INFRASTRUCTURE; needs a GPU).  x is T x NC x B column-major, complex single and real double;
 * neighbouring channels (xl = x(:, 1:NC-1, :), xr = x(:, 2:NC, :)), one reference trace for all, an empty result, errors.  Prints "pwznxcorr gateway OK". */
#include <setjmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

enum { T = 300, NC = 5, N = NC - 1, B = 2, W = 9, NL = 4 };
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

/* the same call through the C ABI on hand-staged arrays; rn / rb: the right operand has its own channels / batch entries */
static int direct(int f64, int cplx, int rn, int rb, const void *xl, const void *xr, const void *w, const int64_t *lags, const mxArray *y) {
    qdas_pwznxcorr_desc d;
    memset(&d, 0, sizeof d);
    d.dtype = f64 ? QDAS_F64 : QDAS_F32; d.cplx = cplx; d.device = -1; d.zero = 1; d.norm = 1; d.pad = 1;
    d.T = T; d.N = N; d.W = W; d.nlags = NL; d.bsize[0] = B; d.bsize[1] = 1;
    d.xl_strideN = T; d.xl_bstride[0] = T * N;
    d.xr_strideN = rn ? T : 0; d.xr_bstride[0] = rb ? T * (rn ? N : 1) : 0;
    d.y_strideN = T; d.y_bstride[0] = T * N; d.y_strideL = T * N * B;
    const size_t es = f64 ? 8 : 4, xs = es * (cplx ? 2 : 1);
    const size_t lb = xs * T * N * B, rbts = xs * T * (rn ? N : 1) * (rb ? B : 1), yb = xs * T * N * B * NL;
    void *dl = NULL, *dr = NULL, *dw = NULL, *dy = NULL;
    if (qdas_device_malloc(&dl, lb, -1) || qdas_device_copy(dl, xl, lb, 0, -1) || qdas_device_malloc(&dr, rbts, -1) || qdas_device_copy(dr, xr, rbts, 0, -1)) return 0;
    if (qdas_device_malloc(&dw, es * W, -1) || qdas_device_copy(dw, w, es * W, 0, -1) || qdas_device_malloc(&dy, yb, -1)) return 0;
    if (qdas_pwznxcorr(&d, dl, dr, dw, lags, dy, NULL)) return 0;
    void *h = malloc(yb);
    const int ok = qdas_device_copy(h, dy, yb, 1, -1) == 0 && mxGetNumberOfElements(y) == (size_t)T * N * B * NL && memcmp(h, mxGetData(y), yb) == 0;
    free(h);
    qdas_device_free(dl, -1); qdas_device_free(dr, -1); qdas_device_free(dw, -1); qdas_device_free(dy, -1);
    return ok;
}

int main(void) {
    srand(7);
    /* complex single: x is T x NC x B; the gateway takes the two slices as arrays of their own */
    const mwSize ld[3] = {T, N, B}, od[3] = {T, 1, 1};
    mxArray *xl = mxCreateNumericArray(3, ld, mxSINGLE_CLASS, mxCOMPLEX), *xr = mxCreateNumericArray(3, ld, mxSINGLE_CLASS, mxCOMPLEX);
    mxArray *x0 = mxCreateNumericArray(3, od, mxSINGLE_CLASS, mxCOMPLEX);
    float *x = (float *)malloc(sizeof(float) * 2 * T * NC * B), *pl = (float *)mxGetData(xl), *pr = (float *)mxGetData(xr), *p0 = (float *)mxGetData(x0);
    for (size_t k = 0; k < (size_t)2 * T * NC * B; ++k) x[k] = (float)rand() / RAND_MAX - 0.5f;
    for (int b = 0; b < B; ++b) {
        memcpy(pl + (size_t)2 * T * N * b, x + (size_t)2 * T * NC * b, sizeof(float) * 2 * T * N);
        memcpy(pr + (size_t)2 * T * N * b, x + (size_t)2 * T * (NC * b + 1), sizeof(float) * 2 * T * N);
    }
    memcpy(p0, x + 2 * T * 2, sizeof(float) * 2 * T);
    mxArray *w = mxCreateNumericMatrix(W, 1, mxSINGLE_CLASS, mxREAL);
    for (int k = 0; k < W; ++k) ((float *)mxGetData(w))[k] = 0.5f + 0.1f * (float)k;
    const double lg[NL] = {3, -1, 3, 0}, ps[8] = {T, N, B, 1, 1, 1, 1, 1}, ps0[8] = {T, N, B, 1, 1, 1, 0, 0};
    const int64_t tab[NL] = {3, -1, 3, 0};
    mxArray *lags = row(NL, lg), *psz = row(8, ps), *psz0 = row(8, ps0), *cmd = mxCreateString("pwznxcorr");
    mxArray *out[1] = {NULL};

    const mxArray *a1[6] = {cmd, psz, xl, xr, w, lags};
    CHECK(call(1, out, 6, a1) == 0 && mxIsComplex(out[0]) && mxGetClassID(out[0]) == mxSINGLE_CLASS);
    CHECK(direct(0, 1, 1, 1, pl, pr, mxGetData(w), tab, out[0]));
    mxDestroyArray(out[0]);
    /* one reference trace for every channel and batch entry (ref = "x0" / "center") */
    const mxArray *a2[6] = {cmd, psz0, xl, x0, w, lags};
    CHECK(call(1, out, 6, a2) == 0);
    CHECK(direct(0, 1, 0, 0, pl, p0, mxGetData(w), tab, out[0]));
    mxDestroyArray(out[0]);
    /* real double */
    mxArray *dl = mxCreateNumericArray(3, ld, mxDOUBLE_CLASS, mxREAL), *dr = mxCreateNumericArray(3, ld, mxDOUBLE_CLASS, mxREAL);
    mxArray *dw = mxCreateNumericMatrix(W, 1, mxDOUBLE_CLASS, mxREAL);
    for (size_t k = 0; k < (size_t)T * N * B; ++k) { ((double *)mxGetData(dl))[k] = (double)rand() / RAND_MAX - 0.5; ((double *)mxGetData(dr))[k] = (double)rand() / RAND_MAX - 0.5; }
    for (int k = 0; k < W; ++k) ((double *)mxGetData(dw))[k] = 1.0 / W;
    const mxArray *a3[6] = {cmd, psz, dl, dr, dw, lags};
    CHECK(call(1, out, 6, a3) == 0 && !mxIsComplex(out[0]) && mxGetClassID(out[0]) == mxDOUBLE_CLASS);
    CHECK(direct(1, 0, 1, 1, mxGetData(dl), mxGetData(dr), mxGetData(dw), tab, out[0]));
    mxDestroyArray(out[0]);
    /* no channel pairs (N <= stride): an empty result, nothing launched */
    const double pe[6] = {T, 0, B, 1, 1, 1};
    mxArray *pse = row(6, pe), *xe = mxCreateNumericArray(2, (const mwSize[2]){0, 0}, mxSINGLE_CLASS, mxCOMPLEX);
    const mxArray *z1[6] = {cmd, pse, xe, xe, w, lags};
    CHECK(call(1, out, 6, z1) == 0 && mxGetNumberOfElements(out[0]) == 0 && mxIsComplex(out[0]));
    mxDestroyArray(out[0]);
    /* errors: non-integer lags, a negative weight with norm, mixed classes, a window past the LDS budget, too few arguments */
    const double lh[2] = {0.5, 1};
    mxArray *lbad = row(2, lh);
    const mxArray *e1[6] = {cmd, psz, xl, xr, w, lbad};
    CHECK(call(1, out, 6, e1) == 1 && strstr(fake_mex_last_msg, "integers"));
    mxArray *wn = mxCreateNumericMatrix(W, 1, mxSINGLE_CLASS, mxREAL);
    ((float *)mxGetData(wn))[3] = -1.0f;
    const mxArray *e2[6] = {cmd, psz, xl, xr, wn, lags};
    CHECK(call(1, out, 6, e2) == 1 && strstr(fake_mex_last_msg, "negative weight"));
    const mxArray *e3[6] = {cmd, psz, xl, dr, w, lags};
    CHECK(call(1, out, 6, e3) == 1 && strstr(fake_mex_last_msg, "same class"));
    mxArray *wbig = mxCreateNumericMatrix(6000, 1, mxSINGLE_CLASS, mxREAL);
    const mxArray *e4[6] = {cmd, psz, xl, xr, wbig, lags};
    CHECK(call(1, out, 6, e4) == 1 && strstr(fake_mex_last_msg, "LDS"));
    CHECK(call(1, out, 5, a1) == 1 && !strcmp(fake_mex_last_id, "QUPS:das_spec:nargin"));
    free(x);
    printf("pwznxcorr through the gateway: bit-identical to the C ABI\n");
    printf("pwznxcorr gateway OK\n");
    return 0;
}
