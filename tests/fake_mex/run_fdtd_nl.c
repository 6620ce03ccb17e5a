/* run_fdtd_nl.c -- drives the 'fdtdnl' command of mex/qdas_mex.c over the fake MEX runtime and the REAL libqdas.so (TEST INFRASTRUCTURE; needs a GPU).
 * The case is read from a file tests/test_mex_fdtd_nl.py writes (the tables of qups_amd/fdtd.py `prepare`, the loss map and the map bq, already in the class
 * under test, so that both sides see the same bits); the result is compared bit for bit with qdas_fdtd_nonlinear called directly on device arrays and
 * written to a second file, which the test compares bit for bit with the Python layer's record.  Then the zero block against the linear commands, empty
 * calls and the refusals.  Prints "fdtdnl gateway OK".
 *
 * usage: run_fdtd_nl in.bin out.bin.  in.bin: int64 [dbl Nz Nx V Nt M Ts N order L lossy flags], double [dt_h inv_h], then in the class (single | double):
 * med (4 Nz Nx), pml (2 Nz + 2 Nx), s (Ts M V, pulse fastest), kap (Nz Nx), bq (Nz Nx), then double: loss (1 + 2 L: mode, g, E), src (3 M: node, wz, wx per
 * source), sen (N).  lossy = 0: kap and loss are read and not used. */
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
    int64_t hd[12];
    double sc[2];
    CHECK(fread(hd, sizeof(int64_t), 12, f) == 12 && fread(sc, sizeof(double), 2, f) == 2);
    const mxClassID cls = hd[0] ? mxDOUBLE_CLASS : mxSINGLE_CLASS;
    const size_t rs = hd[0] ? 8 : 4, Nz = (size_t)hd[1], Nx = (size_t)hd[2], V = (size_t)hd[3], Nt = (size_t)hd[4], M = (size_t)hd[5], Ts = (size_t)hd[6], N = (size_t)hd[7], L = (size_t)hd[9];
    const int lossy = (int)hd[10];
    const size_t cells = Nz * Nx;
    mxArray *med = read_arr(f, 4 * cells, cls), *pml = read_arr(f, 2 * (Nz + Nx), cls), *s = read_arr(f, Ts * M * V, cls), *kap = read_arr(f, cells, cls);
    mxArray *bq = read_arr(f, cells, cls);
    mxArray *loss = read_arr(f, 1 + 2 * L, mxDOUBLE_CLASS);
    mxArray *src = read_arr(f, 3 * M, mxDOUBLE_CLASS), *sen = read_arr(f, N, mxDOUBLE_CLASS);
    CHECK(med && pml && s && kap && bq && loss && src && sen && L <= 4 && (lossy || L == 0));
    fclose(f);
    const double prm[7] = {(double)Nz, (double)Nx, (double)V, (double)Nt, sc[0], sc[1], (double)hd[8]}, flv[1] = {(double)hd[11]};
    mxArray *cmd = mxCreateString("fdtdnl"), *pa = vec(prm, 7), *fl = vec(flv, 1), *out[2] = {NULL, NULL};
    const mxArray *in[11] = {cmd, med, pml, s, src, sen, pa, bq, fl, kap, loss};
    CHECK(call(1, out, lossy ? 11 : 9, in) == 0 && out[0]);
    CHECK(mxGetClassID(out[0]) == cls && !mxIsComplex(out[0]) && mxGetNumberOfElements(out[0]) == Nt * N * V);

    /* the C ABI directly, on the same tables */
    const uint64_t nt = qdas_fdtd_tiles(Nz, Nx);
    int32_t *hi = (int32_t *)calloc(2 * M + 2 * N + 2 * (nt + 1) + 1, sizeof(int32_t));
    void *hw = calloc(2 * M + 1, rs), *hz = calloc((5 + L) * cells * V + 1, rs), *hb = malloc(Nt * N * V * rs + 1);
    CHECK(hi && hw && hz && hb);
    int32_t *src_node = hi, *src_start = src_node + M, *src_list = src_start + nt + 1, *sen_node = src_list + M, *sen_start = sen_node + N, *sen_list = sen_start + nt + 1;
    const double *sv = (const double *)mxGetData(src), *nv = (const double *)mxGetData(sen);
    for (size_t m = 0; m < M; ++m) {
        src_node[m] = (int32_t)sv[3 * m];
        for (int r = 0; r < 2; ++r) { if (hd[0]) ((double *)hw)[r * M + m] = sv[3 * m + 1 + r]; else ((float *)hw)[r * M + m] = (float)sv[3 * m + 1 + r]; }
    }
    for (size_t j = 0; j < N; ++j) sen_node[j] = (int32_t)nv[j];
    CHECK(qdas_fdtd_tile_lists(Nz, Nx, M, src_node, src_start, src_list) == 0 && qdas_fdtd_tile_lists(Nz, Nx, N, sen_node, sen_start, sen_list) == 0);
    char *dmed = (char *)stage(mxGetData(med), 4 * cells * rs), *dpml = (char *)stage(mxGetData(pml), 2 * (Nz + Nx) * rs), *dst = (char *)stage(hz, (5 + L) * cells * V * rs);
    void *ds = stage(mxGetData(s), Ts * M * V * rs), *dw = stage(hw, 2 * M * rs), *di = stage(hi, (2 * M + 2 * N + 2 * (nt + 1)) * sizeof(int32_t)), *drec = NULL;
    void *dkap = stage(mxGetData(kap), cells * rs), *dbq = stage(mxGetData(bq), cells * rs);
    CHECK(dkap && dbq);
    CHECK(dmed && dpml && dst && ds && dw && di && !qdas_device_malloc(&drec, Nt * N * V * rs, -1));
    qdas_fdtd_desc d;
    memset(&d, 0, sizeof d);
    d.Nz = Nz; d.Nx = Nx; d.V = V; d.Nt = Nt; d.ld = Nz; d.vstride = cells; d.M = M; d.Ts = Ts; d.N = N;
    d.rec_st = 1; d.rec_sn = Nt; d.rec_sv = Nt * N;
    d.dt_h = sc[0]; d.inv_h = sc[1]; d.dtype = hd[0] ? QDAS_F64 : QDAS_F32; d.order = (int32_t)hd[8]; d.device = -1;
    qdas_fdtd_args a;
    memset(&a, 0, sizeof a);
    const size_t sb = cells * V * rs;
    a.p = dst; a.uz = dst + sb; a.ux = dst + 2 * sb; a.rz = dst + 3 * sb; a.rx = dst + 4 * sb;
    a.c2 = dmed; a.rho = dmed + cells * rs; a.dtrz = dmed + 2 * cells * rs; a.dtrx = dmed + 3 * cells * rs;
    a.az = dpml; a.azs = dpml + Nz * rs; a.ax = dpml + 2 * Nz * rs; a.axs = dpml + (2 * Nz + Nx) * rs;
    a.s = ds; a.src_wz = dw; a.src_wx = (char *)dw + M * rs;
    const int32_t *dii = (const int32_t *)di;
    a.src_node = dii; a.src_start = dii + M; a.src_list = a.src_start + nt + 1; a.sen_node = a.src_list + M; a.sen_start = a.sen_node + N; a.sen_list = a.sen_start + nt + 1;
    a.rec = drec;
    qdas_fdtd_loss q;
    memset(&q, 0, sizeof q);
    const double *lv = (const double *)mxGetData(loss);
    q.mode = (int32_t)lv[0]; q.L = (int32_t)L; q.kap = dkap; q.e = L ? dst + 5 * sb : NULL;
    for (size_t k = 0; k < L; ++k) { q.g[k] = lv[1 + k]; q.E[k] = lv[1 + L + k]; }
    qdas_fdtd_nl w;
    memset(&w, 0, sizeof w);
    w.bq = dbq; w.flags = (int32_t)hd[11];
    CHECK(qdas_fdtd_nonlinear(&d, &a, lossy ? &q : NULL, &w) == 0);
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
    qdas_device_free(di, -1); qdas_device_free(drec, -1); qdas_device_free(dkap, -1); qdas_device_free(dbq, -1);
    printf("fdtdnl through the gateway: bit-identical to the C ABI\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) { printf("usage: run_fdtd_nl in.bin out.bin\n"); return 2; }
    const int rc = parity(argv[1], argv[2]);
    if (rc) return rc;
    /* a tiny homogeneous grid by hand, driven hard (the source adds 0.5 x 0.4 m/s in its first step: 6 % of rho): the zero block against the linear commands, each term on its own,
     * no steps, no sensors; refused: the map's class and size, the flags, the loss arguments, nargin */
    enum { NZ = 6, NX = 5 };
    const double prm[7] = {NZ, NX, 1, 4, 0.3, 1e4, 2}, prm0[7] = {NZ, NX, 1, 0, 0.3, 1e4, 2};
    const double src[3] = {NZ * 2 + 3, 0.5, 0.0}, sen[2] = {NZ * 2 + 3, NZ * 2 + 2}, sv[2] = {0.4, -0.4};
    const double stokes[1] = {QDAS_FDTD_LOSS_STOKES}, relax[3] = {QDAS_FDTD_LOSS_RELAX, 0.7, 0.2}, mode9[3] = {9, 0.7, 0.2};
    const double f0[1] = {0}, f1v[1] = {QDAS_FDTD_NL_NO_CONVECTIVE}, f2v[1] = {2}, fh[1] = {0.5}, ff[2] = {0, 0};
    mxArray *cmd = mxCreateString("fdtdnl"), *plain = mxCreateString("fdtd"), *lossc = mxCreateString("fdtdloss");
    mxArray *med = mxCreateNumericMatrix(1, 4 * NZ * NX, mxDOUBLE_CLASS, mxREAL), *pml = mxCreateNumericMatrix(1, 2 * (NZ + NX), mxDOUBLE_CLASS, mxREAL);
    mxArray *kap = mxCreateNumericMatrix(1, NZ * NX, mxDOUBLE_CLASS, mxREAL), *bq = mxCreateNumericMatrix(1, NZ * NX, mxDOUBLE_CLASS, mxREAL);
    mxArray *bq0 = mxCreateNumericMatrix(1, NZ * NX, mxDOUBLE_CLASS, mxREAL);
    mxArray *bqf = mxCreateNumericMatrix(1, NZ * NX, mxSINGLE_CLASS, mxREAL), *bqs = mxCreateNumericMatrix(1, NZ * NX - 1, mxDOUBLE_CLASS, mxREAL);
    const double fill[4] = {2.25e6, 1000.0, 1e-11, 1e-11};
    for (int k4 = 0; k4 < 4; ++k4) for (int k = 0; k < NZ * NX; ++k) ((double *)mxGetData(med))[k4 * NZ * NX + k] = fill[k4];
    for (int k = 0; k < 2 * (NZ + NX); ++k) ((double *)mxGetData(pml))[k] = 1.0;
    for (int k = 0; k < NZ * NX; ++k) { ((double *)mxGetData(kap))[k] = 0.1; ((double *)mxGetData(bq))[k] = 3e-3; }
    mxArray *s = vec(sv, 2), *sa = vec(src, 3), *na = vec(sen, 2), *n0 = vec(sen, 0), *pa = vec(prm, 7), *p0 = vec(prm0, 7);
    mxArray *ls = vec(stokes, 1), *lr = vec(relax, 3), *l9 = vec(mode9, 3);
    mxArray *fa = vec(f0, 1), *fb = vec(f1v, 1), *fc = vec(f2v, 1), *fd = vec(fh, 1), *fe = vec(ff, 2);
    mxArray *out[2] = {NULL, NULL}, *ref[2] = {NULL, NULL}, *refl[2] = {NULL, NULL};
    const mxArray *base[7] = {plain, med, pml, s, sa, na, pa}, *basel[9] = {lossc, med, pml, s, sa, na, pa, kap, lr};
    CHECK(call(1, ref, 7, base) == 0 && ref[0] && mxGetNumberOfElements(ref[0]) == 8);
    CHECK(call(1, refl, 9, basel) == 0 && refl[0] && mxGetNumberOfElements(refl[0]) == 8);
    const double *w = (const double *)mxGetData(ref[0]), *wl = (const double *)mxGetData(refl[0]);
    CHECK(w[0] != 0.0 && memcmp(w, wl, 8 * sizeof(double)) != 0);
    /* the zero block: the bits of 'fdtd' without the loss arguments, of 'fdtdloss' with them */
    const mxArray *z1[9] = {cmd, med, pml, s, sa, na, pa, bq0, fb}, *z2[11] = {cmd, med, pml, s, sa, na, pa, bq0, fb, kap, lr};
    CHECK(call(1, out, 9, z1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8 && memcmp(mxGetData(out[0]), w, 8 * sizeof(double)) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    CHECK(call(1, out, 11, z2) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8 && memcmp(mxGetData(out[0]), wl, 8 * sizeof(double)) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    /* each term on its own and both: three different records, none of them the linear one */
    const mxArray *t1[9] = {cmd, med, pml, s, sa, na, pa, bq0, fa}, *t2[9] = {cmd, med, pml, s, sa, na, pa, bq, fb}, *t3[9] = {cmd, med, pml, s, sa, na, pa, bq, fa};
    double got[3][8];
    const mxArray **terms[3] = {t1, t2, t3};
    for (int k = 0; k < 3; ++k) {
        CHECK(call(1, out, 9, terms[k]) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 8 && mxGetClassID(out[0]) == mxDOUBLE_CLASS);
        memcpy(got[k], mxGetData(out[0]), sizeof got[k]);
        mxDestroyArray(out[0]); out[0] = NULL;
        CHECK(memcmp(got[k], w, sizeof got[k]) != 0 && isfinite(got[k][1]));
    }
    CHECK(memcmp(got[0], got[1], sizeof got[0]) != 0 && memcmp(got[0], got[2], sizeof got[0]) != 0 && memcmp(got[1], got[2], sizeof got[0]) != 0);
    const mxArray *st[11] = {cmd, med, pml, s, sa, na, pa, bq, fa, kap, ls};
    CHECK(call(1, out, 11, st) == 0 && out[0] && memcmp(mxGetData(out[0]), got[2], sizeof got[2]) != 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *e0[9] = {cmd, med, pml, s, sa, na, p0, bq, fa}, *e1[11] = {cmd, med, pml, s, sa, n0, pa, bq, fa, kap, lr};
    CHECK(call(1, out, 9, e0) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    CHECK(call(1, out, 11, e1) == 0 && out[0] && mxGetNumberOfElements(out[0]) == 0);
    mxDestroyArray(out[0]); out[0] = NULL;
    const mxArray *r1[9] = {cmd, med, pml, s, sa, na, pa, bqf, fa}, *r2[9] = {cmd, med, pml, s, sa, na, pa, bqs, fa}, *r3[9] = {cmd, med, pml, s, sa, na, pa, bq, fc};
    const mxArray *r4[9] = {cmd, med, pml, s, sa, na, pa, bq, fd}, *r5[9] = {cmd, med, pml, s, sa, na, pa, bq, fe}, *r6[9] = {cmd, med, pml, s, sa, na, p0, bq, fc};
    const mxArray *r7[11] = {cmd, med, pml, s, sa, na, pa, bq, fa, kap, l9}, *r8[11] = {cmd, med, pml, s, sa, na, pa, bq, fa, bqs, lr};
    CHECK(call(1, out, 9, r1) == 1 && strstr(fake_mex_last_msg, "class of med"));
    CHECK(call(1, out, 9, r2) == 1 && strstr(fake_mex_last_msg, "bq must be Nz x Nx"));
    CHECK(call(1, out, 9, r3) == 1 && strstr(fake_mex_last_msg, "unknown flags 0x2"));
    CHECK(call(1, out, 9, r4) == 1 && strstr(fake_mex_last_msg, "unknown flags"));
    CHECK(call(1, out, 9, r5) == 1 && strstr(fake_mex_last_msg, "flags is one value"));
    CHECK(call(1, out, 9, r6) == 1 && strstr(fake_mex_last_msg, "unknown flags 0x2"));       /* an empty call is still validated */
    CHECK(call(1, out, 11, r7) == 1 && strstr(fake_mex_last_msg, "unknown loss mode 9"));
    CHECK(call(1, out, 11, r8) == 1 && strstr(fake_mex_last_msg, "kap must be Nz x Nx"));
    CHECK(call(1, out, 10, st) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(1, out, 8, t3) == 1 && strstr(fake_mex_last_id, "nargin"));
    CHECK(call(2, out, 9, t3) == 1 && strstr(fake_mex_last_id, "nargout"));
    mxDestroyArray(ref[0]); mxDestroyArray(refl[0]);
    printf("fdtdnl gateway OK\n");
    return 0;
}
