/* run_fdtd3.c -- drives the 'fdtd3' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so (TEST INFRASTRUCTURE; needs a GPU).  The case
 * is read from a file tests/test_mex_fdtd3.py writes (the tables of qups_amd/fdtd3.py `prepare`, already in the class under test, so that both sides see the
 * same bits); the result is compared bit for bit with qdas_fdtd3 called directly on device arrays and written to a second file, which the test compares bit
 * for bit with the Python layer's record.  Then an empty call and the refusals.  Prints "fdtd3 gateway OK".
 *
 * usage: run_fdtd3 in.bin out.bin.  in.bin: int64 [dbl Nz Nx Ny V Nt M Ts N order], double [dt_h inv_h], then in the class (single | double): med
 * (5 Nz Nx Ny), pml (2 Nz + 2 Nx + 2 Ny), s (Ts M V, pulse fastest), then double: src (4 M: node, wz, wx, wy per source), sen (N). */
#include <math.h>
#include <setjmp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#include "qdas.h"

extern jmp_buf fake_mex_jmp;
extern char fake_mex_last_id[128], fake_mex_last_msg[1024];

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s / %s)\n", __LINE__, #c, fake_mex_last_id, fake_mex_last_msg); return 1; } } while (0)

static int call(int nlhs, mxArray **out, int nrhs, const mxArray **in) {     /* 0: returned, 1: raised */
    if (setjmp(fake_mex_jmp)) return 1;
    mexFunction(nlhs, out, nrhs, in);
    return 0;
}
static mxArray *vec(const double *v, size_t n) {
    mxArray *a = mxCreateNumericMatrix(1, (mwSize)n, mxDOUBLE_CLASS, mxREAL);
    if (n) memcpy(mxGetData(a), v, n * sizeof(double));
    return a;
}
static mxArray *read_arr(FILE *f, size_t n, mxClassID cls) {
    mxArray *a = mxCreateNumericMatrix(1, (mwSize)n, cls, mxREAL);
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4;
    if (n && fread(mxGetData(a), es, n, f) != n) return NULL;
    return a;
}
static void *stage(const void *h, size_t bytes) {
    void *p = NULL;
    if (qdas_device_malloc(&p, bytes ? bytes : 1, -1) || (bytes && qdas_device_copy(p, h, bytes, 0, -1))) return NULL;
    return p;
}

static int parity(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) { perror(in_path); return 2; }
    int64_t hd[10];
    double sc[2];
    CHECK(fread(hd, sizeof(int64_t), 10, f) == 10 && fread(sc, sizeof(double), 2, f) == 2);
    const mxClassID cls = hd[0] ? mxDOUBLE_CLASS : mxSINGLE_CLASS;
    const size_t rs = hd[0] ? 8 : 4, Nz = (size_t)hd[1], Nx = (size_t)hd[2], Ny = (size_t)hd[3], V = (size_t)hd[4], Nt = (size_t)hd[5], M = (size_t)hd[6], Ts = (size_t)hd[7],
                 N = (size_t)hd[8];
    const size_t cells = Nz * Nx * Ny, npml = 2 * (Nz + Nx + Ny);
    mxArray *med = read_arr(f, 5 * cells, cls), *pml = read_arr(f, npml, cls), *s = read_arr(f, Ts * M * V, cls);
    mxArray *src = read_arr(f, 4 * M, mxDOUBLE_CLASS), *sen = read_arr(f, N, mxDOUBLE_CLASS);
    CHECK(med && pml && s && src && sen);
    fclose(f);
    const double prm[8] = {(double)Nz, (double)Nx, (double)Ny, (double)V, (double)Nt, sc[0], sc[1], (double)hd[9]};
    mxArray *cmd = mxCreateString("fdtd3"), *pa = vec(prm, 8), *out[2] = {NULL, NULL};
    const mxArray *in[7] = {cmd, med, pml, s, src, sen, pa};
    CHECK(call(1, out, 7, in) == 0 && out[0]);
    CHECK(mxGetClassID(out[0]) == cls && !mxIsComplex(out[0]) && mxGetNumberOfElements(out[0]) == Nt * N * V);

    /* the C ABI directly, on the same tables */
    const uint64_t nb = qdas_fdtd3_bricks(Nz, Nx, Ny);
    int32_t *hi = (int32_t *)calloc(2 * M + 2 * N + 2 * (nb + 1) + 1, sizeof(int32_t));
    void *hw = calloc(3 * M + 1, rs), *hz = calloc(7 * cells * V, rs), *hb = malloc(Nt * N * V * rs + 1);
    CHECK(hi && hw && hz && hb);
    int32_t *src_node = hi, *src_start = src_node + M, *src_list = src_start + nb + 1, *sen_node = src_list + M, *sen_start = sen_node + N, *sen_list = sen_start + nb + 1;
    const double *sv = (const double *)mxGetData(src), *nv = (const double *)mxGetData(sen);
    for (size_t m = 0; m < M; ++m) {
        src_node[m] = (int32_t)sv[4 * m];
        for (int r = 0; r < 3; ++r) { if (hd[0]) ((double *)hw)[r * M + m] = sv[4 * m + 1 + r]; else ((float *)hw)[r * M + m] = (float)sv[4 * m + 1 + r]; }
    }
    for (size_t j = 0; j < N; ++j) sen_node[j] = (int32_t)nv[j];
    CHECK(qdas_fdtd3_brick_lists(Nz, Nx, Ny, M, src_node, src_start, src_list) == 0 && qdas_fdtd3_brick_lists(Nz, Nx, Ny, N, sen_node, sen_start, sen_list) == 0);
    char *dmed = (char *)stage(mxGetData(med), 5 * cells * rs), *dpml = (char *)stage(mxGetData(pml), npml * rs), *dst = (char *)stage(hz, 7 * cells * V * rs);
    void *ds = stage(mxGetData(s), Ts * M * V * rs), *dw = stage(hw, 3 * M * rs), *di = stage(hi, (2 * M + 2 * N + 2 * (nb + 1)) * sizeof(int32_t)), *drec = NULL;
    CHECK(dmed && dpml && dst && ds && dw && di && !qdas_device_malloc(&drec, Nt * N * V * rs, -1));
    qdas_fdtd3_desc d;
    memset(&d, 0, sizeof d);
    d.Nz = Nz; d.Nx = Nx; d.Ny = Ny; d.V = V; d.Nt = Nt; d.ld = Nz; d.pstride = Nz * Nx; d.vstride = cells; d.M = M; d.Ts = Ts; d.N = N;
    d.rec_st = 1; d.rec_sn = Nt; d.rec_sv = Nt * N;
    d.dt_h = sc[0]; d.inv_h = sc[1]; d.dtype = hd[0] ? QDAS_F64 : QDAS_F32; d.order = (int32_t)hd[9]; d.device = -1;
    qdas_fdtd3_args a;
    memset(&a, 0, sizeof a);
    const size_t sb = cells * V * rs;
    a.p = dst; a.uz = dst + sb; a.ux = dst + 2 * sb; a.uy = dst + 3 * sb; a.rz = dst + 4 * sb; a.rx = dst + 5 * sb; a.ry = dst + 6 * sb;
    a.c2 = dmed; a.rho = dmed + cells * rs; a.dtrz = dmed + 2 * cells * rs; a.dtrx = dmed + 3 * cells * rs; a.dtry = dmed + 4 * cells * rs;
    a.az = dpml; a.azs = dpml + Nz * rs; a.ax = dpml + 2 * Nz * rs; a.axs = dpml + (2 * Nz + Nx) * rs; a.ay = dpml + 2 * (Nz + Nx) * rs; a.ays = dpml + (2 * (Nz + Nx) + Ny) * rs;
    a.s = ds; a.src_wz = dw; a.src_wx = (char *)dw + M * rs; a.src_wy = (char *)dw + 2 * M * rs;
    const int32_t *dii = (const int32_t *)di;
    a.src_node = dii; a.src_start = dii + M; a.src_list = a.src_start + nb + 1; a.sen_node = a.src_list + M; a.sen_start = a.sen_node + N; a.sen_list = a.sen_start + nb + 1;
    a.rec = drec;
    CHECK(qdas_fdtd3(&d, &a) == 0);
    const size_t obytes = Nt * N * V * rs;
    CHECK(!qdas_device_copy(hb, drec, obytes, 1, -1));
    CHECK(memcmp(hb, mxGetData(out[0]), obytes) == 0);
    size_t nonzero = 0;
    for (size_t k = 0; k < obytes; ++k) nonzero += ((const unsigned char *)hb)[k] != 0;
    CHECK(nonzero > obytes / 4);
    FILE *dump = fopen(out_path, "wb");
    CHECK(dump && fwrite(mxGetData(out[0]), 1, obytes, dump) == obytes);
    fclose(dump);
    mxDestroyArray(out[0]);
    free(hi); free(hw); free(hz); free(hb);
    qdas_device_free(dmed, -1); qdas_device_free(dpml, -1); qdas_device_free(dst, -1); qdas_device_free(ds, -1); qdas_device_free(dw, -1);
    qdas_device_free(di, -1); qdas_device_free(drec, -1);
    printf("fdtd3 through the gateway: bit-identical to the C ABI\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) { printf("usage: run_fdtd3 in.bin out.bin\n"); return 2; }
    const int rc = parity(argv[1], argv[2]);
    if (rc) return rc;
    /* a tiny homogeneous grid by hand: no steps, no sensors; refused: a class, sizes, a node outside the grid, an order, nargin, nargout */
    enum { NZ = 6, NX = 5, NY = 4, CELLS = NZ * NX * NY, NPML = 2 * (NZ + NX + NY), NODE = (2 * NX + 2) * NZ + 3 };
    const double prm[8] = {NZ, NX, NY, 1, 4, 0.3, 1e4, 2}, prm0[8] = {NZ, NX, NY, 1, 0, 0.3, 1e4, 2}, prmo[8] = {NZ, NX, NY, 1, 4, 0.3, 1e4, 6};
    const double prmz[8] = {NZ, NX, NY + 1, 1, 4, 0.3, 1e4, 2};
    const double src[4] = {NODE, 0.5, 0.0, 0.25}, srcbad[4] = {CELLS, 0.5, 0.0, 0.0}, sen[2] = {NODE, 0}, sv[2] = {1.0, -1.0};
    mxArray *cmd = mxCreateString("fdtd3"), *med = mxCreateNumericMatrix(1, 5 * CELLS, mxDOUBLE_CLASS, mxREAL), *pml = mxCreateNumericMatrix(1, NPML, mxDOUBLE_CLASS, mxREAL);
    mxArray *medi = mxCreateNumericMatrix(1, 5 * CELLS, mxINT32_CLASS, mxREAL), *pmlf = mxCreateNumericMatrix(1, NPML, mxSINGLE_CLASS, mxREAL);
    const double fill[5] = {2.25e6, 1000.0, 1e-11, 1e-11, 1e-11};
    for (int q = 0; q < 5; ++q) for (int k = 0; k < CELLS; ++k) ((double *)mxGetData(med))[q * CELLS + k] = fill[q];
    for (int k = 0; k < NPML; ++k) ((double *)mxGetData(pml))[k] = 1.0;
    mxArray *s = vec(sv, 2), *sa = vec(src, 4), *sb = vec(srcbad, 4), *na = vec(sen, 2), *n0 = vec(sen, 0), *pa = vec(prm, 8), *p0 = vec(prm0, 8), *po = vec(prmo, 8), *pz = vec(prmz, 8);
    mxArray *out[2] = {NULL, NULL};
    const mxArray *ok[7] = {cmd, med, pml, s, sa, na, pa};
    CHECK(call(1, out, 7, ok) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8 && mxGetClassID(out[0]) == mxDOUBLE_CLASS);
    const double *v = (const double *)mxGetData(out[0]);
    CHECK(v[0] != 0.0 && v[4] == 0.0 && v[5] == 0.0);                                   /* the source's own node answers in step 0; node 0 is two steps away or more */
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *e0[7] = {cmd, med, pml, s, sa, na, p0}, *e1[7] = {cmd, med, pml, s, sa, n0, pa}, *e2[7] = {cmd, med, pml, n0, n0, na, pa};
    CHECK(call(1, out, 7, e2) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8);       /* no sources: the sensors record the medium at rest */
    for (int k = 0; k < 8; ++k) CHECK(((const double *)mxGetData(out[0]))[k] == 0.0);
    mxDestroyArray(out[0]); out[0] = NULL;
    CHECK(call(1, out, 7, e0) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    CHECK(call(1, out, 7, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *f1[7] = {cmd, medi, pml, s, sa, na, pa}, *f2[7] = {cmd, med, pmlf, s, sa, na, pa}, *f3[7] = {cmd, med, pml, s, sa, na, pz};
    const mxArray *f4[7] = {cmd, med, pml, s, sb, na, pa}, *f5[7] = {cmd, med, pml, s, sa, na, po}, *f6[7] = {cmd, med, pml, s, na, na, pa};
    CHECK(call(1, out, 7, f1) == 1 && strstr(fake_mex_last_msg, "real single or double"));
    CHECK(call(1, out, 7, f2) == 1 && strstr(fake_mex_last_msg, "class of med"));
    CHECK(call(1, out, 7, f3) == 1 && strstr(fake_mex_last_msg, "Nz x Nx x Ny x 5"));
    CHECK(call(1, out, 7, f4) == 1 && strstr(fake_mex_last_msg, "[0, Nz Nx Ny)"));
    CHECK(call(1, out, 7, f5) == 1 && strstr(fake_mex_last_msg, "order 6"));
    CHECK(call(1, out, 7, f6) == 1 && strstr(fake_mex_last_msg, "4 x M"));
    CHECK(call(1, out, 6, ok) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(2, out, 7, ok) == 1 && strstr(fake_mex_last_id, "nargout"));
    printf("fdtd3 gateway OK\n");
    return 0;
}
