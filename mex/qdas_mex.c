/* qdas_mex.c -- thin MEX gateway from MATLAB to libqdas.so (C ABI in include/qdas.h).
 *
 * MATLAB is not available in this repository's environment; this is the binding a QUPS maintainer builds,
 *
 *     mex -R2018a -I<repo>/include -L<repo>/qups_amd -lqdas mex/qdas_mex.c -output bin/qdas_mex
 *     mex -R2018a -DQDAS_MEX_GPU -I... -L... -lqdas -lmwgpu mex/qdas_mex.c -output bin/qdas_mex      % gpuArray inputs / outputs
 *
 * and what tests/test_mex_gateway.py compiles against a small stand-in for mex.h (tests/fake_mex/: a syntax / ABI / logic check of
 * THIS file, not a MATLAB).  It replaces ONE call site of the reference: the kernel object + constant upload + per-frame launch
 * inside das_spec (kern/das_spec.m:279-306, :367-378), including the reusable handle the reference returns to callers that stream
 * frames, [k, PRE_ARGS, POST_ARGS] (kern/das_spec.m:72-81, 387-390):
 *
 *   y = qdas_mex(sizes, Pi, Pr, Pv, Nv, apod, cinv, acstride, x, tvars)               one call = create + execute + destroy
 *   h = qdas_mex('create', sizes, Pi, Pr, Pv, Nv, apod, cinv, acstride, tvars [, opts]) plan handle (uint64 scalar), kept until
 *   y = qdas_mex('execute', h, x)                                                       'destroy' / clear mex; x: T x N x M x F
 *       qdas_mex('prepare', h, F)                                                       do now what the plan's first stream of F frames would do once (qdas_plan_prepare_frames)
 *   s = qdas_mex('info', h)                                                             char: kernel name, shards
 *       qdas_mex('destroy' [, h])
 *
 * The other launch sites of the path, one command each (stateless; arguments in the order of the reference's own k.feval lists):
 *   tau = qdas_mex('delays', sizes, Pi, Pr, Pv, Nv, cinv)                 kern/das_spec.m:376-377  k.feval(yg, Pi, Pr, Pv, Nv, cinv(1))       -> I x N x M real(prec)
 *   tau = qdas_mex('delays', h)                                           the same from a live plan (its geometry is on the device already)
 *   y   = qdas_mex('lut', lsizes, w, x, t1, t2, wstride, omega)           kern/wsinterpd2.m:236    k.feval(y, w, x, t1, t2, sizes, iflags, strides, flagnum, imag(omega))
 *         as bfDASLUT -> sample2sep calls it (src/UltrasoundSystem.m:4641-4660): lsizes = [T N M I flag dtype I1 w_real], t1 = receive table I x N, t2 = transmit
 *         table I x M (samples), w = [] or weights with element strides wstride = uint64 [si sn sm] (0 where singleton); y is I x [1|N] x [1|M] complex(prec)
 *   y   = qdas_mex('wsinterpd', wsz, size, strides, sumdims, w, x, t, tvars)   kern/wsinterpd.m:221-236  k.feval(y, w, x, t, sizes, iflags, strides, flagnum, imag(omega))
 *         the general single-delay launch (ChannelData.sample, rectifyt0): wsz = [T x_tstride ndim flag dtype w_real], size = the ndim sizes of the broadcast index
 *         space (dimension 1 = the sampled one), strides = int64 3 x ndim element strides of [t; x; w] (0 where singleton; the trace bases of x: row 2, entry 1 is 0),
 *         sumdims = 1 x ndim flags, tvars = [imag(omega) extrapval]; y is dense column-major over the kept dimensions (summed ones singleton), complex(prec)
 *   y   = qdas_mex('shiftsum', ssz, x, shift, w)                               src/UltrasoundSystem.m:3498 (focusTx: sample2sep(chd.time, -tau, interp, apd, mdim))
 *         ssz = [T To N M Mo F flag dtype cplx w_real]; x: T x N x M x F, shift: M x Mo real(prec) samples, w: M x Mo real or complex(prec) or []; y: To x N x Mo x F
 *   y   = qdas_mex('greens', gsizes, ps, as, pn, pv, x, tvars)            src/UltrasoundSystem.m:681-718  k.feval(x, ps, as, pn, pv, kn, sb, blocks, [t0k t0x fso fsr cinv R0], [E E], flagnum)
 *         gsizes = [S T N M I En Em flagnum dtype], tvars = [t0k t0x fso fsr cinv R0]; the sb / blocks culling tables are not needed; y is S x N x M complex
 *   z   = qdas_mex('convd', csizes, x, y)                                 kern/convd.m:150-199     kern.feval(x, y, z, sizes)
 *         csizes = [C M N S dtype cplx shape bcast y_real] (include/qdas.h qdas_convd_desc); z is C x L x S
 *   y   = qdas_mex('hilbert', psizes, x, tvars)                           src/ChannelData.m:935-966 (+ downmix :757-766)
 *         psizes = [T K Nfft in_type], tvars = [fs t0 fdown]; x real single or int16 T x K; y is Nfft x K complex single
 * Aperture-reduction images of a receive-kept image (kern/slsc.m, dmas.m, cohfac.m, pcf.m; the MATLAB branches), x real or complex single / double:
 *   z       = qdas_mex('slsc', ksz, x, L, method)   method 'average' | 'ensemble'; L: [] (max(1, floor(N/4))), a scalar (lags 1:L) or a vector of lags
 *   z       = qdas_mex('dmas', ksz, x, L)           L: [] (1:N-1), a scalar (1:L) or a vector (intersect(1:N-1, L))
 *   r       = qdas_mex('cohfac', ksz, x)            over both reduced dimensions
 *   [w, sf] = qdas_mex('pcf', ksz, x, gamma)        complex x only; gamma: [] = 1.  (With -DQDAS_MEX_GPU, sf returns as a host array.)
 *         ksz = [A N B K C kfirst]: x is A x N x B x K x C column-major (as kern/slsc.m's OpenCL branch sizes it: A = prod(sz(1:dim-1)), N = sz(dim),
 *         ...), N the reduced aperture, K a second reduced dimension (slsc's kdim, cohfac's second dim; omitted = 1), kfirst = 1: x is A x K x B x N x C
 *         (kdim < dim).  The result is A x B x C (the caller reshapes it to size(x) with the reduced dimensions set to 1); complex for complex slsc / dmas.
 * Pair-wise windowed zero-normalized cross-correlation (kern/pwznxcorr.m, the base-MATLAB branch: iflt = false), every lag in one launch:
 *   y       = qdas_mex('pwznxcorr', psz, xl, xr, w, lags)
 *         psz = [T N B zero norm pad rN rB]: xl is T x N x B column-major (real or complex single / double), the left traces; xr the right traces of the same
 *         class and complexity, T x (rN ? N : 1) x (rB ? B : 1) (rN / rB = 0: one trace for every channel / batch entry; omitted = 1); w: the real window
 *         weights of x's class (the caller expands a scalar W to ones(W, 1)); lags: integers, any order.  y is T x N x B x numel(lags), complex for complex x.
 *         The caller slices x into xl / xr as the reference does (sub(x, 1:N-S, ndim) / sub(x, 1+S:N, ndim), the centre trace, x0).
 * Travel times through a speed map (kern/msfm.m with two arguments: first order, four neighbours; what bfEikonal's parfor loops compute one element at a time):
 *   T       = qdas_mex('msfm', csz, F, src, first, max_passes)
 *         csz = [C1 C2]; F: C1 x C2 double, host or gpuArray, the speed in cells per second; src: 2 x P double (host), 1-based points, floored to a node;
 *         first: [] (every point is a source of its own: K = P maps) or the K + 1 offsets (0-based, ascending, last = P) that cut src into K source sets --
 *         a cell {s1, s2, ...} of 2 x P_k arrays is passed as src = [s1 s2 ...], first = [0 cumsum(P_k)]; max_passes: [] | 0 = the derived cap.
 *         T is C1 x C2 x K double (seconds).  An empty F or no points: an empty T, nothing is launched.
 *   T       = qdas_mex('msfm3d', csz, F, src, first, max_passes)
 *         the same through a VOLUME (kern/msfm.m for size(F, 3) > 1: msfm3d, first order, six neighbours): csz = [C1 C2 C3]; F: C1 x C2 x C3 double; src: 3 x P
 *         double; T is C1 x C2 x C3 x K double.
 * The frequency loop of bfAdjoint (src/UltrasoundSystem.m:3997-4037) as one call:
 *   b       = qdas_mex('adjoint', sizes, xk, f, Pi, Pr, Pt, cinv, del_tx, apod_tx, a_n, a_m, flags)
 *         sizes = [I N M V F], flags = [keep_rx keep_tx]; the arrays are described at cmd_adjoint below.  b is I x [N] x [V] single complex.
 *   b       = qdas_mex('migration', sizes, x, tau, gamma, params, flags)
 *         sizes = [T N M frames F K], params = [fs fmod t0 c0 pitch], flags = [interp keep_tx jacobian]; described at cmd_migration below.
 * REFoCUS (src/UltrasoundSystem.m:3735-3762: the decoder Hi applied to the data; building Hi stays in MATLAB, as the reference has it):
 *   y       = qdas_mex('refocus', sizes, x, Hi, t0, fs)
 *         sizes = [T N V M frames]; described at cmd_refocus below.
 * Straight-ray integrals over a rectilinear grid (kern/wbilerpg.m, and what kern/rayPaths.m / kern/globalAverageC.m make of its triplets):
 *   [cxy, ixo, iyo] = qdas_mex('wbilerp', gsz, x, y, pa, pb)
 *   [v, len]        = qdas_mex('rayintegrals', gsz, x, z, pa, pb, maps)
 *   [g, col]        = qdas_mex('raybackproject', gsz, x, z, pa, pb, r)
 *         gsz = [X Y J sa sb] (wbilerp) | [X Z J sa sb F xstride zstride] (rayintegrals, raybackproject); described at cmd_wbilerp / cmd_rayintegrals /
 *         cmd_raybackproject below.
 * Scan conversion (src/ScanPolar.m:143-201, src/ScanSpherical.m:121-188; e = [] for a polar scan; angles in degrees):
 *   bc      = qdas_mex('scanconvert', b, r, a, e, origin, x, y, z, opts)
 *         opts = [] | [pre db_floor fill] | a struct with those fields; described at cmd_scanconvert below.
 *   y       = qdas_mex('demod', x, b, [T fc fs ratio gdiv], t0)
 *         downmix -> filter -> downsample in one pass; described at cmd_demod below.
 *   y       = qdas_mex('resample', x, h, [T p q off J edge])
 *         rational-rate polyphase FIR: resample, upfirdn, FIR filtfilt; described at cmd_resample below.
 *   rec     = qdas_mex('fdtd', med, pml, s, src, sen, [Nz Nx V Nt dt_h inv_h order])
 *         2-D acoustic FDTD from rest, the record of the sensors; described at cmd_fdtd below.
 *   rec     = qdas_mex('fdtdloss', med, pml, s, src, sen, [Nz Nx V Nt dt_h inv_h order], kap, [mode g E])
 *         the same with power-law absorption (qdas_fdtd_lossy); described at cmd_fdtd below.
 *   rec     = qdas_mex('fdtdnl', med, pml, s, src, sen, [Nz Nx V Nt dt_h inv_h order], bq, flags[, kap, [mode g E]])
 *         the same with nonlinear propagation, with or without absorption (qdas_fdtd_nonlinear); described at cmd_fdtd below.
 *   rec     = qdas_mex('fdtd3', med, pml, s, src, sen, [Nz Nx Ny V Nt dt_h inv_h order])
 *         the same through a volume; described at cmd_fdtd3 below.
 * Host arrays are staged through device memory by the gateway (qdas_device_malloc / _copy / _free: no HIP headers needed); with -DQDAS_MEX_GPU gpuArrays
 * pass as device pointers and the result is a gpuArray.
 *
 *   sizes    : numeric row [T N M I1 I2 I3 S flag VS DV dtype]  (dtype: 0 double, 1 single, 2 half)   -- any real numeric class;
 *              the QUPS_* constants of kern/das_spec.m:294-298.  The one-call form takes a 12th entry F (frames).
 *   Pi..Nv   : real(prec) arrays laid out 3 x I, 3 x N, 4 x M (row 4 = t0, kern/das_spec.m:361), 3 x M
 *   apod     : complex(prec) column (concatenated arrays, kern/das_spec.m:344-345) or [] ; cinv: real(prec) array
 *   acstride : uint64 6 x (1+S)  [cstride, astride]                                     (kern/das_spec.m:257-260)
 *   tvars    : [fs fmod], any real numeric class
 *   opts     : struct, all fields optional: devices (row of device ordinals: a multi-GPU plan, qdas_plan_create_sharded),
 *              jit (true: QDAS_PLAN_JIT), reciprocal (false: QDAS_PLAN_NO_RECIPROCAL), mirror (false: QDAS_PLAN_NO_MIRROR), fold (false: QDAS_PLAN_NO_FOLD),
 *              approx_symmetry (true: QDAS_PLAN_APPROX_SYMMETRY), kernel (0 auto | 1 generic | 2 tiled)
 *   x, y     : complex(prec); half precision travels as uint16 arrays with a leading dimension of 2 (re, im), as the reference
 *              passes ushort2 (src/bf.cu:164-171)
 * Host arrays use QDAS_MEM_HOST (the library stages them through HBM).  With -DQDAS_MEX_GPU, gpuArray arguments are passed as
 * device pointers (QDAS_MEM_DEVICE, mxGPUArray API) and y is returned as a gpuArray: no gather() of the 1.5 GB frame.  A plan is
 * created for ONE memory kind (that of Pi); 'execute' refuses an x of the other kind.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"
#ifdef QDAS_MEX_GPU
#include "gpu/mxGPUArray.h"
#endif
#include "qdas.h"

#define QDAS_MEX_MAX_PLANS 64

typedef struct {
    int used;
    qdas_plan *plan;
    qdas_sharded_plan *splan;
    qdas_sizes sz;
    int mem;                                            /* QDAS_MEM_* of the plan */
} plan_slot;

static plan_slot g_slots[QDAS_MEX_MAX_PLANS];
static int g_nlive = 0, g_atexit = 0;

static void destroy_slot(plan_slot *s) {
    if (!s->used) return;
    if (s->plan) qdas_plan_destroy(s->plan);
    if (s->splan) qdas_plan_destroy_sharded(s->splan);
    memset(s, 0, sizeof *s);
    if (--g_nlive == 0 && mexIsLocked()) mexUnlock();
}
static void destroy_all(void) { for (int k = 0; k < QDAS_MEX_MAX_PLANS; ++k) destroy_slot(&g_slots[k]); }

/* element k of a real numeric array of any class, as double (sizes / tvars / opts may arrive as double, single or integers) */
static double num_at(const mxArray *a, mwSize k, const char *what) {
    if (!a || mxIsComplex(a) || k >= mxGetNumberOfElements(a)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s: real numeric array with more than %d entries expected.", what, (int)k);
    const void *p = mxGetData(a);
    switch (mxGetClassID(a)) {
        case mxDOUBLE_CLASS: return ((const double *)p)[k];
        case mxSINGLE_CLASS: return (double)((const float *)p)[k];
        case mxINT64_CLASS:  return (double)((const int64_t *)p)[k];
        case mxUINT64_CLASS: return (double)((const uint64_t *)p)[k];
        case mxINT32_CLASS:  return (double)((const int32_t *)p)[k];
        case mxUINT32_CLASS: return (double)((const uint32_t *)p)[k];
        case mxLOGICAL_CLASS: return (double)((const unsigned char *)p)[k];
        default: mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s: unsupported numeric class.", what);
    }
    return 0.0;
}

static mxClassID class_of(int dtype) { return dtype == QDAS_F64 ? mxDOUBLE_CLASS : (dtype == QDAS_F32 ? mxSINGLE_CLASS : mxUINT16_CLASS); }

/* data pointer of an argument; *is_dev tells whether it is a gpuArray (only with QDAS_MEX_GPU) */
typedef struct { const void *ptr; int is_dev;
#ifdef QDAS_MEX_GPU
    const mxGPUArray *g;
#endif
} argptr;

static argptr arg_data(const mxArray *a) {
    argptr r;
    memset(&r, 0, sizeof r);
    if (!a || mxIsEmpty(a)) return r;
#ifdef QDAS_MEX_GPU
    if (mxIsGPUArray(a)) { r.g = mxGPUCreateFromMxArray(a); r.ptr = mxGPUGetDataReadOnly(r.g); r.is_dev = 1; return r; }
#endif
    r.ptr = mxGetData(a);
    return r;
}
static void arg_release(argptr *r) {
#ifdef QDAS_MEX_GPU
    if (r->g) mxGPUDestroyGPUArray(r->g);
#endif
    (void)r;
}

static void read_sizes(const mxArray *sz, qdas_sizes *z, uint64_t *F) {
    const mwSize n = mxGetNumberOfElements(sz);
    if (n < 11) mexErrMsgIdAndTxt("QUPS:das_spec:sizes", "sizes must have at least 11 entries [T N M I1 I2 I3 S flag VS DV dtype].");
    z->T = (uint64_t)num_at(sz, 0, "sizes");  z->N = (uint64_t)num_at(sz, 1, "sizes");  z->M = (uint64_t)num_at(sz, 2, "sizes");
    z->I1 = (uint64_t)num_at(sz, 3, "sizes"); z->I2 = (uint64_t)num_at(sz, 4, "sizes"); z->I3 = (uint64_t)num_at(sz, 5, "sizes");
    z->S = (uint64_t)num_at(sz, 6, "sizes");  z->flag = (int32_t)num_at(sz, 7, "sizes");
    z->VS = (int32_t)num_at(sz, 8, "sizes");  z->DV = (int32_t)num_at(sz, 9, "sizes");  z->dtype = (int32_t)num_at(sz, 10, "sizes");
    if (F) *F = n >= 12 ? (uint64_t)num_at(sz, 11, "sizes") : 1;
}

/* create a plan from prhs[0..8] = sizes, Pi, Pr, Pv, Nv, apod, cinv, acstride, tvars (+ optional opts); returns the slot index */
static int create_plan(int nrhs, const mxArray *prhs[]) {
    if (nrhs < 9) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('create', ...) expects sizes, Pi, Pr, Pv, Nv, apod, cinv, acstride, tvars [, opts].");
    int slot = -1;
    for (int k = 0; k < QDAS_MEX_MAX_PLANS; ++k) if (!g_slots[k].used) { slot = k; break; }
    if (slot < 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "too many live plans (destroy some).");
    qdas_desc d;
    memset(&d, 0, sizeof d);
    read_sizes(prhs[0], &d.sz, NULL);
    if (mxGetClassID(prhs[7]) != mxUINT64_CLASS || mxGetNumberOfElements(prhs[7]) < 6 * (1 + d.sz.S))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "acstride must be uint64 with 6 x (1 + S) entries.");
    argptr a[6];
    const int idx[6] = {1, 2, 3, 4, 5, 6};
    for (int k = 0; k < 6; ++k) a[k] = arg_data(prhs[idx[k]]);
    d.Pi = a[0].ptr; d.Pr = a[1].ptr; d.Pv = a[2].ptr; d.Nv = a[3].ptr; d.apod = a[4].ptr; d.cinv = a[5].ptr;
    const int dev = a[0].is_dev;
    for (int k = 1; k < 6; ++k)
        if (a[k].ptr && a[k].is_dev != dev) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "Pi, Pr, Pv, Nv, apod, cinv must all be gpuArrays or all be host arrays.");
    d.acstride = (const uint64_t *)mxGetData(prhs[7]);       /* always a host array */
    d.fs = num_at(prhs[8], 0, "tvars"); d.fmod = num_at(prhs[8], 1, "tvars");
    d.mem = dev ? QDAS_MEM_DEVICE : QDAS_MEM_HOST;
    d.device = -1; d.kernel = QDAS_KERNEL_AUTO;
    /* gpuArray inputs: the handle outlives this call but the caller's gpuArrays do not (das_spec's workspace is freed when it
       returns `k = h`), and the mxGPUArray views are released below -- the plan must own device copies (qdas.h, LIFETIME) */
    if (dev) d.plan_flags |= QDAS_PLAN_COPY_INPUTS;
    int ndev = 0, devices[64];
    if (nrhs >= 10 && !mxIsEmpty(prhs[9])) {
        const mxArray *o = prhs[9], *f;
        if (!mxIsStruct(o)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "opts must be a struct.");
        if ((f = mxGetField(o, 0, "jit")) && num_at(f, 0, "opts.jit") != 0) d.plan_flags |= QDAS_PLAN_JIT;
        if ((f = mxGetField(o, 0, "reciprocal")) && num_at(f, 0, "opts.reciprocal") == 0) d.plan_flags |= QDAS_PLAN_NO_RECIPROCAL;
        if ((f = mxGetField(o, 0, "mirror")) && num_at(f, 0, "opts.mirror") == 0) d.plan_flags |= QDAS_PLAN_NO_MIRROR;
        if ((f = mxGetField(o, 0, "fold")) && num_at(f, 0, "opts.fold") == 0) d.plan_flags |= QDAS_PLAN_NO_FOLD;
        if ((f = mxGetField(o, 0, "approx_symmetry")) && num_at(f, 0, "opts.approx_symmetry") != 0) d.plan_flags |= QDAS_PLAN_APPROX_SYMMETRY;
        if ((f = mxGetField(o, 0, "kernel"))) d.kernel = (int32_t)num_at(f, 0, "opts.kernel");
        if ((f = mxGetField(o, 0, "devices"))) {
            ndev = (int)mxGetNumberOfElements(f);
            if (ndev > 64) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "at most 64 devices.");
            for (int k = 0; k < ndev; ++k) devices[k] = (int)num_at(f, (mwSize)k, "opts.devices");
        }
    }
    plan_slot *s = &g_slots[slot];
    int rc;
    if (ndev > 0) { d.device = devices[0]; rc = qdas_plan_create_sharded(&s->splan, &d, ndev, devices); }
    else rc = qdas_plan_create(&s->plan, &d);
    for (int k = 0; k < 6; ++k) arg_release(&a[k]);
    if (rc) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s", qdas_last_error());
    s->used = 1; s->sz = d.sz; s->mem = d.mem;
    if (g_nlive++ == 0) { if (!g_atexit) { mexAtExit(destroy_all); g_atexit = 1; } mexLock(); }   /* plans outlive the call */
    return slot;
}

/* y = execute(slot, x): F frames of T x N x M.  Returns NULL on success, else the message to raise -- so that the one-call form
 * can release its plan before raising (mexErrMsgIdAndTxt does not return). */
static char g_msg[600];
#define QFAIL(...) do { snprintf(g_msg, sizeof g_msg, __VA_ARGS__); return g_msg; } while (0)
static const char *execute_plan(plan_slot *s, const mxArray *xa, uint64_t F_hint, mxArray **out) {
    const qdas_sizes *z = &s->sz;
    const uint64_t per = z->T * z->N * z->M, I = z->I1 * z->I2 * z->I3;
    const uint64_t oN = (z->flag & QDAS_FLAG_KEEP_RX) ? z->N : 1, oM = (z->flag & QDAS_FLAG_KEEP_TX) ? z->M : 1;
    const int half = z->dtype == QDAS_F16;
    *out = NULL;
    if (!half && per && !mxIsComplex(xa)) QFAIL("x must be complex.");
    if (per && mxGetClassID(xa) != class_of(z->dtype)) QFAIL("x does not have the plan's precision.");
    const uint64_t nel = (uint64_t)mxGetNumberOfElements(xa) / (half ? 2 : 1);
    const uint64_t F = per ? nel / per : (F_hint ? F_hint : 1);
    if (per && (F == 0 || F * per != nel)) QFAIL("x must be T x N x M x F for the plan's T, N, M.");
    argptr x = arg_data(xa);
    if (per && x.is_dev != (s->mem == QDAS_MEM_DEVICE)) { arg_release(&x); QFAIL("x must be a %s array for this plan.", s->mem == QDAS_MEM_DEVICE ? "gpuArray" : "host"); }
    mxArray *ya;
    void *yp;
    mwSize dims[5], nd;
    if (half) { dims[0] = 2; dims[1] = (mwSize)I; dims[2] = (mwSize)oN; dims[3] = (mwSize)oM; dims[4] = (mwSize)F; nd = 5; }
    else { dims[0] = (mwSize)I; dims[1] = (mwSize)oN; dims[2] = (mwSize)oM; dims[3] = (mwSize)F; nd = 4; }
#ifdef QDAS_MEX_GPU
    mxGPUArray *yg = NULL;
    if (s->mem == QDAS_MEM_DEVICE) {
        yg = mxGPUCreateGPUArray(nd, dims, class_of(z->dtype), half ? mxREAL : mxCOMPLEX, MX_GPU_DO_NOT_INITIALIZE);
        yp = mxGPUGetData(yg);
        ya = NULL;
    } else
#endif
    {
        ya = mxCreateNumericArray(nd, dims, class_of(z->dtype), half ? mxREAL : mxCOMPLEX);
        yp = mxGetData(ya);
    }
    int rc = 0;
    if (s->splan) {
        const size_t ds = z->dtype == QDAS_F64 ? 16 : (z->dtype == QDAS_F32 ? 8 : 4);
        for (uint64_t f = 0; f < F && !rc; ++f)
            rc = qdas_plan_execute_sharded(s->splan, (const char *)x.ptr + f * per * ds, (char *)yp + f * I * oN * oM * ds, NULL);
    } else
        rc = qdas_plan_execute_frames(s->plan, x.ptr, yp, F, per, I * oN * oM, NULL);
    arg_release(&x);
#ifdef QDAS_MEX_GPU
    if (yg) { ya = mxGPUCreateMxArrayOnGPU(yg); mxGPUDestroyGPUArray(yg); }
#endif
    if (rc) { if (ya) mxDestroyArray(ya); QFAIL("%s", qdas_last_error()); }
    *out = ya;
    return NULL;
}

static plan_slot *slot_of(const mxArray *h) {
    const double v = num_at(h, 0, "handle");
    const int k = (int)v - 1;
    if (v != (double)(k + 1) || k < 0 || k >= QDAS_MEX_MAX_PLANS || !g_slots[k].used) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "invalid or destroyed plan handle.");
    return &g_slots[k];
}

/* ---- the stateless commands: device-pointer entries of the C ABI behind host arrays (staged here) or gpuArrays (passed through) */
typedef struct { const void *ptr; void *owned; argptr a; } devarg;
#define QDAS_MEX_MAX_DEVARGS 12
static devarg g_da[QDAS_MEX_MAX_DEVARGS];
static int g_nda = 0;
static void *g_out_dev = NULL;                          /* device image of a host output */
static void release_devargs(void) {
    for (int k = 0; k < g_nda; ++k) { if (g_da[k].owned) qdas_device_free(g_da[k].owned, -1); arg_release(&g_da[k].a); }
    g_nda = 0;
    if (g_out_dev) { qdas_device_free(g_out_dev, -1); g_out_dev = NULL; }
}
/* raise after releasing what the command staged (mexErrMsgIdAndTxt does not return) */
#define CFAIL(...) do { release_devargs(); mexErrMsgIdAndTxt("QUPS:das_spec:qdas", __VA_ARGS__); } while (0)

/* device pointer of an input of `bytes` bytes ([] -> NULL); *any_dev collects whether some argument was a gpuArray */
static const void *dev_in(const mxArray *a, size_t bytes, const char *what, int *any_dev) {
    if (g_nda >= QDAS_MEX_MAX_DEVARGS) CFAIL("too many array arguments.");
    devarg *d = &g_da[g_nda++];
    memset(d, 0, sizeof *d);
    d->a = arg_data(a);
    if (!d->a.ptr) return NULL;
    const size_t have = (size_t)mxGetNumberOfElements(a) * (mxGetClassID(a) == mxDOUBLE_CLASS || mxGetClassID(a) == mxINT64_CLASS || mxGetClassID(a) == mxUINT64_CLASS ? 8 :
                        mxGetClassID(a) == mxSINGLE_CLASS || mxGetClassID(a) == mxINT32_CLASS || mxGetClassID(a) == mxUINT32_CLASS ? 4 :
                        mxGetClassID(a) == mxINT16_CLASS || mxGetClassID(a) == mxUINT16_CLASS ? 2 : 1) * (mxIsComplex(a) ? 2 : 1);
    if (have < bytes) CFAIL("%s: %llu bytes expected, the array holds %llu (class / complexity / size mismatch).", what, (unsigned long long)bytes, (unsigned long long)have);
    if (d->a.is_dev) { *any_dev = 1; d->ptr = d->a.ptr; return d->ptr; }
    if (qdas_device_malloc(&d->owned, bytes, -1) || qdas_device_copy(d->owned, d->a.ptr, bytes, 0, -1)) CFAIL("%s", qdas_last_error());
    d->ptr = d->owned;
    return d->ptr;
}

/* output array of `nd` dims: a gpuArray when the inputs were (GPU build), else a host array with a device image in g_out_dev; returns the device pointer */
#ifdef QDAS_MEX_GPU
static mxGPUArray *g_out_gpu = NULL;
#endif
static void *dev_out(mwSize nd, const mwSize *dims, mxClassID cls, int cplx, int on_dev, size_t bytes, mxArray **host) {
    *host = NULL;
#ifdef QDAS_MEX_GPU
    if (on_dev) { g_out_gpu = mxGPUCreateGPUArray(nd, dims, cls, cplx ? mxCOMPLEX : mxREAL, MX_GPU_DO_NOT_INITIALIZE); return mxGPUGetData(g_out_gpu); }
#endif
    (void)on_dev;
    *host = mxCreateNumericArray(nd, dims, cls, cplx ? mxCOMPLEX : mxREAL);
    if (qdas_device_malloc(&g_out_dev, bytes, -1)) { mxDestroyArray(*host); *host = NULL; CFAIL("%s", qdas_last_error()); }
    return g_out_dev;
}
/* after the launch: the host image is fetched (synchronises) ... */
static int fetch_out(int rc, mxArray *host, size_t bytes) {
    if (!rc && host && g_out_dev) rc = qdas_device_copy(mxGetData(host), g_out_dev, bytes, 1, -1);
    return rc;
}
/* ... and everything staged is released; rc != 0 raises with the library's message */
static mxArray *conclude(int rc, mxArray *host) {
    mxArray *ret = host;
#ifdef QDAS_MEX_GPU
    if (g_out_gpu) { if (!rc) ret = mxGPUCreateMxArrayOnGPU(g_out_gpu); mxGPUDestroyGPUArray(g_out_gpu); g_out_gpu = NULL; }
#endif
    if (rc) { if (host) mxDestroyArray(host); CFAIL("%s", qdas_last_error()); }
    release_devargs();
    return ret;
}
static mxArray *finish(int rc, mxArray *host, size_t bytes) { return conclude(fetch_out(rc, host, bytes), host); }
static size_t cbytes(int dtype) { return dtype == QDAS_F64 ? 16 : (dtype == QDAS_F32 ? 8 : 4); }     /* complex sample */
static size_t rbytes(int dtype) { return dtype == QDAS_F64 ? 8 : 4; }                                   /* geometry / time (half data: single) */

/* tau = qdas_mex('delays', sizes, Pi, Pr, Pv, Nv, cinv) | qdas_mex('delays', h) -- kern/das_spec.m:376-377, src/bf.cu:209-298 */
static mxArray *cmd_delays(int nrhs, const mxArray *prhs[]) {
    mxArray *host;
    if (nrhs == 1) {                                    /* a live plan */
        plan_slot *s = slot_of(prhs[0]);
        if (!s->plan) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "'delays' needs a single-device plan.");
        const qdas_sizes *z = &s->sz;
        const mwSize dims[3] = {(mwSize)(z->I1 * z->I2 * z->I3), (mwSize)z->N, (mwSize)z->M};
        const size_t bytes = (size_t)dims[0] * dims[1] * dims[2] * rbytes(z->dtype);
        void *tau = dev_out(3, dims, z->dtype == QDAS_F64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, 0, s->mem == QDAS_MEM_DEVICE, bytes, &host);
        return finish(qdas_plan_delays(s->plan, tau, NULL), host, bytes);
    }
    if (nrhs != 6) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('delays', sizes, Pi, Pr, Pv, Nv, cinv) or qdas_mex('delays', h)");
    qdas_sizes z;
    read_sizes(prhs[0], &z, NULL);
    if (z.dtype == QDAS_F16) z.dtype = QDAS_F32;        /* (delays of half data are single: kern/das_spec.m:354-357) */
    const size_t rs = rbytes(z.dtype), I = (size_t)(z.I1 * z.I2 * z.I3);
    int dev = 0;
    const void *Pi = dev_in(prhs[1], 3 * I * rs, "Pi", &dev), *Pr = dev_in(prhs[2], 3 * z.N * rs, "Pr", &dev);
    const void *Pv = dev_in(prhs[3], 4 * z.M * rs, "Pv", &dev), *Nv = dev_in(prhs[4], 3 * z.M * rs, "Nv", &dev);
    const double cinv = num_at(prhs[5], 0, "cinv");    /* cinv(1), as the reference passes it */
    const mwSize dims[3] = {(mwSize)I, (mwSize)z.N, (mwSize)z.M};
    const size_t bytes = I * z.N * z.M * rs;
    void *tau = dev_out(3, dims, z.dtype == QDAS_F64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, 0, dev, bytes, &host);
    const int rc = z.dtype == QDAS_F64 ? qdas_delays(&z, (double *)tau, (const double *)Pi, (const double *)Pr, (const double *)Pv, (const double *)Nv, cinv, NULL)
                                       : qdas_delaysf(&z, (float *)tau, (const float *)Pi, (const float *)Pr, (const float *)Pv, (const float *)Nv, (float)cinv, NULL);
    return finish(rc, host, bytes);
}

/* y = qdas_mex('lut', lsizes, w, x, t1, t2, wstride, omega) -- kern/wsinterpd2.m:236 as bfDASLUT -> sample2sep reaches it */
static mxArray *cmd_lut(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 7) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('lut', lsizes, w, x, t1, t2, wstride, omega)");
    qdas_lut_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *ls = prhs[0];
    d.T = (uint64_t)num_at(ls, 0, "lsizes"); d.N = (uint64_t)num_at(ls, 1, "lsizes"); d.M = (uint64_t)num_at(ls, 2, "lsizes"); d.I = (uint64_t)num_at(ls, 3, "lsizes");
    d.flag = (int32_t)num_at(ls, 4, "lsizes"); d.dtype = (int32_t)num_at(ls, 5, "lsizes");
    d.I1 = mxGetNumberOfElements(ls) > 6 ? (uint64_t)num_at(ls, 6, "lsizes") : 0;
    d.w_real = mxGetNumberOfElements(ls) > 7 ? (int32_t)num_at(ls, 7, "lsizes") : 0;
    d.omega = num_at(prhs[6], 0, "omega");
    if (d.dtype < QDAS_F64 || d.dtype > QDAS_F16) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "lsizes(6): dtype must be 0 (double), 1 (single) or 2 (half).");
    const size_t cs = cbytes(d.dtype), ts = rbytes(d.dtype), ws = d.w_real ? cs / 2 : cs;
    const uint64_t oN = (d.flag & QDAS_FLAG_KEEP_RX) ? d.N : 1, oM = (d.flag & QDAS_FLAG_KEEP_TX) ? d.M : 1;
    int dev = 0;
    if (!mxIsEmpty(prhs[1])) {
        if (mxGetClassID(prhs[5]) != mxUINT64_CLASS || mxGetNumberOfElements(prhs[5]) < 3) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "wstride must be uint64 [si sn sm].");
        memcpy(d.wstride, mxGetData(prhs[5]), 3 * sizeof(uint64_t));
        const uint64_t nel = 1 + (d.I ? d.I - 1 : 0) * d.wstride[0] + (d.N ? d.N - 1 : 0) * d.wstride[1] + (d.M ? d.M - 1 : 0) * d.wstride[2];
        d.w = dev_in(prhs[1], (size_t)nel * ws, "w", &dev);
    }
    const void *x = dev_in(prhs[2], (size_t)(d.T * d.N * d.M) * cs, "x", &dev);
    d.tau_rx = dev_in(prhs[3], (size_t)(d.I * d.N) * ts, "t1", &dev);
    d.tau_tx = dev_in(prhs[4], (size_t)(d.I * d.M) * ts, "t2", &dev);
    const int half = d.dtype == QDAS_F16;
    mwSize dims[4], nd = 0;
    if (half) dims[nd++] = 2;
    dims[nd++] = (mwSize)d.I; dims[nd++] = (mwSize)oN; dims[nd++] = (mwSize)oM;
    const size_t bytes = (size_t)(d.I * oN * oM) * cs;
    mxArray *host;
    void *y = dev_out(nd, dims, class_of(d.dtype), !half, dev, bytes, &host);
    return finish(qdas_das_lut(&d, x, y, NULL), host, bytes);
}

/* y = qdas_mex('wsinterpd', wsz, size, strides, sumdims, w, x, t, tvars) -- kern/wsinterpd.m:221-236, src/interpd.cu:295-342 */
static mxArray *cmd_wsinterpd(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 8) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('wsinterpd', wsz, size, strides, sumdims, w, x, t, tvars)");
    qdas_wsinterpd_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *z = prhs[0];
    d.T = (uint64_t)num_at(z, 0, "wsz"); d.x_tstride = (uint64_t)num_at(z, 1, "wsz"); d.ndim = (int32_t)num_at(z, 2, "wsz"); d.flag = (int32_t)num_at(z, 3, "wsz");
    d.dtype = (int32_t)num_at(z, 4, "wsz"); d.w_real = (int32_t)num_at(z, 5, "wsz"); d.lane_dim = -1;
    if (d.ndim < 1 || d.ndim > 8) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "wsz(3): 1 to 8 dimensions.");
    if (d.dtype < QDAS_F64 || d.dtype > QDAS_F16) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "wsz(5): dtype must be 0 (double), 1 (single) or 2 (half).");
    if (mxGetNumberOfElements(prhs[1]) < (size_t)d.ndim || mxGetNumberOfElements(prhs[2]) < 3 * (size_t)d.ndim || mxGetNumberOfElements(prhs[3]) < (size_t)d.ndim)
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "size, strides (3 x ndim: t, x, w) and sumdims must cover ndim dimensions.");
    uint64_t nt = 1, nx = 1, nw = 1, ny = 1;               /* extents of t, x (trace bases), w, y in elements */
    for (int k = 0; k < d.ndim; ++k) {
        d.size[k] = (uint64_t)num_at(prhs[1], (mwSize)k, "size");
        d.tstride[k] = (int64_t)num_at(prhs[2], (mwSize)(3 * k), "strides"); d.xstride[k] = (int64_t)num_at(prhs[2], (mwSize)(3 * k + 1), "strides");
        d.wstride[k] = (int64_t)num_at(prhs[2], (mwSize)(3 * k + 2), "strides");
        d.sum[k] = num_at(prhs[3], (mwSize)k, "sumdims") != 0;
        if (d.tstride[k] < 0 || d.xstride[k] < 0 || d.wstride[k] < 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "strides must be non-negative (column-major MATLAB arrays).");
        if (d.size[k]) { nt += (d.size[k] - 1) * (uint64_t)d.tstride[k]; nx += (d.size[k] - 1) * (uint64_t)d.xstride[k]; nw += (d.size[k] - 1) * (uint64_t)d.wstride[k]; }
        if (!d.sum[k]) ny *= d.size[k];
    }
    d.omega = num_at(prhs[7], 0, "tvars"); d.extrap = num_at(prhs[7], 1, "tvars");
    const size_t cs = cbytes(d.dtype), ts = rbytes(d.dtype), ws = d.w_real ? cs / 2 : cs;
    int dev = 0;
    d.w = mxIsEmpty(prhs[4]) ? NULL : dev_in(prhs[4], (size_t)nw * ws, "w", &dev);
    d.x = dev_in(prhs[5], (size_t)(nx - 1 + (d.T ? (d.T - 1) * d.x_tstride + 1 : 0)) * cs, "x", &dev);
    d.t = dev_in(prhs[6], (size_t)nt * ts, "t", &dev);
    const int half = d.dtype == QDAS_F16;
    mwSize dims[9], nd = 0;
    if (half) dims[nd++] = 2;
    for (int k = 0; k < d.ndim; ++k) dims[nd++] = (mwSize)(d.sum[k] ? 1 : d.size[k]);
    const size_t bytes = (size_t)ny * cs;
    mxArray *host;
    void *y = dev_out(nd, dims, class_of(d.dtype), !half, dev, bytes, &host);
    return finish(qdas_wsinterpd(&d, y, NULL), host, bytes);
}

/* y = qdas_mex('shiftsum', ssz, x, shift, w) -- UltrasoundSystem.focusTx, src/UltrasoundSystem.m:3374-3503 (:3498) */
static mxArray *cmd_shiftsum(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 4) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('shiftsum', ssz, x, shift, w)");
    qdas_shift_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *z = prhs[0];
    d.T = (uint64_t)num_at(z, 0, "ssz"); d.To = (uint64_t)num_at(z, 1, "ssz"); d.N = (uint64_t)num_at(z, 2, "ssz"); d.M = (uint64_t)num_at(z, 3, "ssz");
    d.Mo = (uint64_t)num_at(z, 4, "ssz"); d.F = (uint64_t)num_at(z, 5, "ssz"); d.flag = (int32_t)num_at(z, 6, "ssz"); d.dtype = (int32_t)num_at(z, 7, "ssz");
    d.cplx = (int32_t)num_at(z, 8, "ssz"); d.w_real = mxGetNumberOfElements(z) > 9 ? (int32_t)num_at(z, 9, "ssz") : 1;
    d.tpad = mxGetNumberOfElements(z) > 10 ? (int32_t)num_at(z, 10, "ssz") : 0;      /* zeros behind the record that are not stored (include/qdas.h) */
    d.device = -1;
    if (d.dtype != QDAS_F64 && d.dtype != QDAS_F32) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "shiftsum: datatype must be double or single");
    const size_t rs = rbytes(d.dtype), es = rs * (d.cplx ? 2 : 1);
    int dev = 0;
    const void *x = dev_in(prhs[1], (size_t)(d.T * d.N * d.M * d.F) * es, "x", &dev);
    d.shift = dev_in(prhs[2], (size_t)(d.M * d.Mo) * rs, "shift", &dev);
    d.w = mxIsEmpty(prhs[3]) ? NULL : dev_in(prhs[3], (size_t)(d.M * d.Mo) * (d.w_real ? rs : 2 * rs), "w", &dev);
    const mwSize dims[4] = {(mwSize)d.To, (mwSize)d.N, (mwSize)d.Mo, (mwSize)d.F};
    const size_t bytes = (size_t)(d.To * d.N * d.Mo * d.F) * es;
    mxArray *host;
    void *y = dev_out(4, dims, d.dtype == QDAS_F64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, d.cplx, dev, bytes, &host);
    return finish(qdas_shift_sum(&d, x, y, NULL), host, bytes);
}

/* y = qdas_mex('greens', gsizes, ps, as, pn, pv, x, tvars) -- src/UltrasoundSystem.m:681-718, src/greens.cu:88-121 */
static mxArray *cmd_greens(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 7) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('greens', gsizes, ps, as, pn, pv, x, tvars)");
    qdas_greens_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *g = prhs[0], *tv = prhs[6];
    d.S = (uint64_t)num_at(g, 0, "gsizes"); d.T = (uint64_t)num_at(g, 1, "gsizes"); d.N = (uint64_t)num_at(g, 2, "gsizes"); d.M = (uint64_t)num_at(g, 3, "gsizes");
    d.I = (uint64_t)num_at(g, 4, "gsizes"); d.En = (int32_t)num_at(g, 5, "gsizes"); d.Em = (int32_t)num_at(g, 6, "gsizes");
    d.interp = (int32_t)num_at(g, 7, "gsizes"); d.dtype = (int32_t)num_at(g, 8, "gsizes");
    d.s0 = num_at(tv, 0, "tvars"); d.t0 = num_at(tv, 1, "tvars"); d.fs = num_at(tv, 2, "tvars"); d.fsr = num_at(tv, 3, "tvars"); d.cinv = num_at(tv, 4, "tvars"); d.R0 = num_at(tv, 5, "tvars");
    d.device = -1;
    if (d.dtype != QDAS_F64 && d.dtype != QDAS_F32) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "greens: datatype must be double or single");
    if (d.En < 1 || d.Em < 1) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "greens: element subdivisions must be >= 1");
    const size_t rs = rbytes(d.dtype), cs = cbytes(d.dtype);
    int dev = 0;
    d.Ps = dev_in(prhs[1], 3 * (size_t)d.I * rs, "ps", &dev);
    d.a = dev_in(prhs[2], (size_t)d.I * cs, "as", &dev);
    d.Pr = dev_in(prhs[3], 3 * (size_t)d.N * (size_t)d.En * rs, "pn", &dev);
    d.Pv = dev_in(prhs[4], 3 * (size_t)d.M * (size_t)d.Em * rs, "pv", &dev);
    d.x = dev_in(prhs[5], (size_t)d.T * cs, "x", &dev);
    const mwSize dims[3] = {(mwSize)d.S, (mwSize)d.N, (mwSize)d.M};
    const size_t bytes = (size_t)(d.S * d.N * d.M) * cs;
    mxArray *host;
    void *y = dev_out(3, dims, d.dtype == QDAS_F64 ? mxDOUBLE_CLASS : mxSINGLE_CLASS, 1, dev, bytes, &host);
    return finish(qdas_greens(&d, y, NULL), host, bytes);
}

/* z = qdas_mex('convd', csizes, x, y) -- kern/convd.m:150-199, src/convd.cu:95-146 */
static mxArray *cmd_convd(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 3) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('convd', csizes, x, y)");
    qdas_convd_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *c = prhs[0];
    d.C = (uint64_t)num_at(c, 0, "csizes"); d.M = (uint64_t)num_at(c, 1, "csizes"); d.N = (uint64_t)num_at(c, 2, "csizes"); d.S = (uint64_t)num_at(c, 3, "csizes");
    d.dtype = (int32_t)num_at(c, 4, "csizes"); d.cplx = (int32_t)num_at(c, 5, "csizes"); d.shape = (int32_t)num_at(c, 6, "csizes");
    d.bcast = mxGetNumberOfElements(c) > 7 ? (int32_t)num_at(c, 7, "csizes") : 0;
    d.y_real = mxGetNumberOfElements(c) > 8 ? (int32_t)num_at(c, 8, "csizes") : 0;
    d.device = -1;
    if (d.dtype < QDAS_F64 || d.dtype > QDAS_F16) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "csizes(5): dtype must be 0 (double), 1 (single) or 2 (half).");
    const size_t es = (d.dtype == QDAS_F64 ? 8 : d.dtype == QDAS_F32 ? 4 : 2), xs = es * (d.cplx ? 2 : 1), ys = es * ((d.cplx && !d.y_real) ? 2 : 1);
    const uint64_t L = qdas_convd_len(d.M, d.N, d.shape);
    const uint64_t xC = (d.bcast & QDAS_CONV_X_ONE_COLUMN) ? 1 : d.C, xS = (d.bcast & QDAS_CONV_X_ONE_SLICE) ? 1 : d.S;
    const uint64_t yC = (d.bcast & QDAS_CONV_Y_ONE_COLUMN) ? 1 : d.C, yS = (d.bcast & QDAS_CONV_Y_ONE_SLICE) ? 1 : d.S;
    int dev = 0;
    const void *x = dev_in(prhs[1], (size_t)(xC * d.M * xS) * xs, "x", &dev);
    const void *y = dev_in(prhs[2], (size_t)(yC * d.N * yS) * ys, "y", &dev);
    const int half = d.dtype == QDAS_F16;
    mwSize dims[4], nd = 0;
    if (half && d.cplx) dims[nd++] = 2;                 /* (half complex travels as uint16 pairs, like the DAS data) */
    dims[nd++] = (mwSize)d.C; dims[nd++] = (mwSize)L; dims[nd++] = (mwSize)d.S;
    const size_t bytes = (size_t)(d.C * L * d.S) * xs;
    mxArray *host;
    void *z = dev_out(nd, dims, class_of(d.dtype), d.cplx && !half, dev, bytes, &host);
    return finish(qdas_convd(&d, x, y, z, NULL), host, bytes);
}

/* y = qdas_mex('hilbert', psizes, x, tvars) -- src/ChannelData.m:935-966 (+ downmix :757-766): plan, one execute, destroy */
static mxArray *cmd_hilbert(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 3) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('hilbert', psizes, x, tvars)");
    qdas_pre_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *p = prhs[0], *tv = prhs[2];
    d.T = (uint64_t)num_at(p, 0, "psizes"); d.K = (uint64_t)num_at(p, 1, "psizes"); d.Nfft = (uint64_t)num_at(p, 2, "psizes");
    d.in_type = mxGetNumberOfElements(p) > 3 ? (int32_t)num_at(p, 3, "psizes") : QDAS_PRE_F32;
    d.device = -1;
    d.fs = num_at(tv, 0, "tvars"); d.t0 = num_at(tv, 1, "tvars"); d.fdown = num_at(tv, 2, "tvars");
    if (d.in_type != QDAS_PRE_F32 && d.in_type != QDAS_PRE_I16) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "psizes(4): in_type must be 0 (single) or 1 (int16).");
    if (mxIsComplex(prhs[1]) || mxGetClassID(prhs[1]) != (d.in_type == QDAS_PRE_I16 ? mxINT16_CLASS : mxSINGLE_CLASS))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "x must be real %s for this in_type.", d.in_type == QDAS_PRE_I16 ? "int16" : "single");
    const uint64_t Nf = d.Nfft ? d.Nfft : d.T;
    int dev = 0;
    const void *x = dev_in(prhs[1], (size_t)(d.T * d.K) * (d.in_type == QDAS_PRE_I16 ? 2 : 4), "x", &dev);
    const mwSize dims[2] = {(mwSize)Nf, (mwSize)d.K};
    const size_t bytes = (size_t)(Nf * d.K) * 8;
    mxArray *host;
    void *y = dev_out(2, dims, mxSINGLE_CLASS, 1, dev, bytes, &host);
    qdas_pre_plan *pl = NULL;
    int rc = qdas_pre_plan_create(&pl, &d);
    if (!rc) rc = qdas_pre_execute(pl, x, y, NULL);
    rc = fetch_out(rc, host, bytes);                    /* (host output: synchronises before the plan goes; gpuArray output: the plan's hipFree does) */
    if (pl) qdas_pre_plan_destroy(pl);
    return conclude(rc, host);
}

/* z = qdas_mex('slsc' | 'dmas' | 'cohfac' | 'pcf', ksz, x, ...) -- kern/slsc.m:187-223, kern/dmas.m:73-79, kern/cohfac.m:64, kern/pcf.m:80-107 */
static void cmd_coherence(const char *cmd, int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    const int slsc = !strcmp(cmd, "slsc"), dmas = !strcmp(cmd, "dmas"), pcf = !strcmp(cmd, "pcf");
    const int maxin = slsc ? 4 : (dmas || pcf ? 3 : 2);
    if (nrhs < 2 || nrhs > maxin) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('%s', ksz, x%s)", cmd, slsc ? ", L, method" : dmas ? ", L" : pcf ? ", gamma" : "");
    qdas_coherence_desc d;
    memset(&d, 0, sizeof d);
    d.device = -1;
    d.gamma = 1.0;
    d.method = slsc ? QDAS_COH_SLSC_AVERAGE : dmas ? QDAS_COH_DMAS : pcf ? QDAS_COH_PCF : QDAS_COH_COHFAC;
    const mxArray *k = prhs[0], *xa = prhs[1];
    const size_t nk = mxGetNumberOfElements(k);
    const uint64_t A = (uint64_t)num_at(k, 0, "ksz"), N = (uint64_t)num_at(k, 1, "ksz"), B = nk > 2 ? (uint64_t)num_at(k, 2, "ksz") : 1;
    const uint64_t K = nk > 3 ? (uint64_t)num_at(k, 3, "ksz") : 1, Cc = nk > 4 ? (uint64_t)num_at(k, 4, "ksz") : 1;
    const int kfirst = nk > 5 && num_at(k, 5, "ksz") != 0;
    const mxClassID cls = mxGetClassID(xa);
    if (cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s: x must be single or double.", cmd);
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32;
    d.cplx = mxIsComplex(xa) ? 1 : 0;
    if (pcf && !d.cplx) mexErrMsgIdAndTxt("QUPS:pcf:realInput", "Input must be complex.");
    const uint64_t R1 = kfirst ? K : N, R2 = kfirst ? N : K;            /* x is A x R1 x B x R2 x C */
    d.N = N; d.K = K;
    d.strideN = (int64_t)(kfirst ? A * R1 * B : A);
    d.strideK = (int64_t)(kfirst ? A : A * R1 * B);
    d.size[0] = A; d.stride[0] = 1;
    d.size[1] = B; d.stride[1] = (int64_t)(A * R1);
    d.size[2] = Cc; d.stride[2] = (int64_t)(A * R1 * B * R2);
    const mxArray *Ltab = NULL;                                        /* a lag vector: copied into a table right before the launch */
    if (slsc || dmas) {
        const mxArray *L = nrhs > 2 ? prhs[2] : NULL;
        if (!L || mxIsEmpty(L)) { d.lag_lo = 1; d.lag_hi = slsc ? (N / 4 > 1 ? N / 4 : 1) : N - 1; }
        else if (mxGetNumberOfElements(L) == 1) {
            const double l = num_at(L, 0, "L");
            if (l < 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s: lags must be non-negative.", cmd);
            d.lag_lo = 1; d.lag_hi = (uint64_t)l;
        } else {
            (void)num_at(L, 0, "L");                                   /* (raises here for a complex or non-numeric L, before anything is staged) */
            d.nlags = mxGetNumberOfElements(L);
            Ltab = L;
        }
    }
    if (slsc && nrhs > 3) {
        char m[16];
        if (!mxIsChar(prhs[3]) || mxGetString(prhs[3], m, sizeof m) || (strcmp(m, "average") && strcmp(m, "ensemble"))) {
            mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "slsc: method must be 'average' or 'ensemble'.");
        }
        if (!strcmp(m, "ensemble")) d.method = QDAS_COH_SLSC_ENSEMBLE;
    }
    if (pcf && nrhs > 2 && !mxIsEmpty(prhs[2])) d.gamma = num_at(prhs[2], 0, "gamma");
    const size_t es = d.dtype == QDAS_F64 ? 8 : 4, xs = es * (d.cplx ? 2 : 1);
    const int ycplx = d.cplx && (slsc || dmas);
    const uint64_t P = A * B * Cc;
    const mwSize dims[3] = {(mwSize)A, (mwSize)B, (mwSize)Cc};
    if (P == 0) {                                                      /* an empty image: empty results, nothing staged or launched */
        plhs[0] = mxCreateNumericArray(3, dims, cls, ycplx ? mxCOMPLEX : mxREAL);
        if (pcf && nlhs > 1) plhs[1] = mxCreateNumericArray(3, dims, cls, mxREAL);
        return;
    }
    int dev = 0;
    const void *x = dev_in(xa, (size_t)(A * N * B * K * Cc) * xs, "x", &dev);
    const size_t bytes = (size_t)P * es * (ycplx ? 2 : 1);
    mxArray *host;
    void *y = dev_out(3, dims, cls, ycplx, dev, bytes, &host);
    int64_t *tab = NULL;
    if (Ltab) {
        tab = (int64_t *)malloc(sizeof(int64_t) * d.nlags);
        if (!tab) { if (host) mxDestroyArray(host); CFAIL("out of host memory."); }
        for (uint64_t i = 0; i < d.nlags; ++i) tab[i] = (int64_t)num_at(Ltab, (mwSize)i, "L");
        d.lags = tab;
    }
    void *y2 = NULL;
    mxArray *host2 = NULL;
    int rc = 0;
    if (pcf) {
        host2 = mxCreateNumericArray(3, dims, cls, mxREAL);
        rc = qdas_device_malloc(&y2, (size_t)P * es, -1);
    }
    if (!rc) rc = qdas_coherence(&d, x, y, y2, NULL);
    free(tab);
    if (pcf) {
        if (!rc) rc = qdas_device_copy(mxGetData(host2), y2, (size_t)P * es, 1, -1);
        if (y2) qdas_device_free(y2, -1);
        if (rc || nlhs < 2) { mxDestroyArray(host2); host2 = NULL; }   /* (w = qdas_mex('pcf', ...): MATLAB provides one output slot) */
    }
    plhs[0] = finish(rc, host, bytes);
    if (host2) plhs[1] = host2;
}

/* y = qdas_mex('pwznxcorr', psz, xl, xr, w, lags) -- kern/pwznxcorr.m:241-299 (iflt = false, integer lags, U = 1, multi = false) */
static mxArray *cmd_pwznxcorr(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 5) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('pwznxcorr', psz, xl, xr, w, lags)");
    qdas_pwznxcorr_desc d;
    memset(&d, 0, sizeof d);
    const mxArray *p = prhs[0], *xl = prhs[1], *xr = prhs[2], *wa = prhs[3], *la = prhs[4];
    const size_t np = mxGetNumberOfElements(p);
    const uint64_t T = (uint64_t)num_at(p, 0, "psz"), N = (uint64_t)num_at(p, 1, "psz"), B = (uint64_t)num_at(p, 2, "psz");
    d.zero = num_at(p, 3, "psz") != 0; d.norm = num_at(p, 4, "psz") != 0; d.pad = num_at(p, 5, "psz") != 0;
    const int rN = np > 6 ? num_at(p, 6, "psz") != 0 : 1, rB = np > 7 ? num_at(p, 7, "psz") != 0 : 1;
    const mxClassID cls = mxGetClassID(xl);
    if (cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "pwznxcorr: x must be single or double.");
    if (mxGetClassID(xr) != cls || mxIsComplex(xr) != mxIsComplex(xl)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "pwznxcorr: xl and xr must have the same class and complexity.");
    if (mxGetClassID(wa) != cls || mxIsComplex(wa)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "pwznxcorr: the weights must be real and of x's class.");
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32;
    d.cplx = mxIsComplex(xl) ? 1 : 0;
    d.device = -1;
    d.T = T; d.N = N; d.W = (uint64_t)mxGetNumberOfElements(wa); d.nlags = (uint64_t)mxGetNumberOfElements(la);
    d.bsize[0] = B; d.bsize[1] = 1;
    const uint64_t xrN = rN ? N : 1;
    d.xl_strideN = (int64_t)T; d.xl_bstride[0] = (int64_t)(T * N);
    d.xr_strideN = rN ? (int64_t)T : 0; d.xr_bstride[0] = rB ? (int64_t)(T * xrN) : 0;
    d.y_strideN = (int64_t)T; d.y_bstride[0] = (int64_t)(T * N); d.y_strideL = (int64_t)(T * N * B);
    if (d.W == 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "pwznxcorr: the window is empty.");
    for (uint64_t i = 0; i < d.nlags; ++i) {                           /* (raises here for complex, non-numeric or non-integer lags, before anything is staged) */
        const double l = num_at(la, (mwSize)i, "lags");
        if ((double)(int64_t)l != l) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "pwznxcorr: lags must be integers.");
    }
#ifdef QDAS_MEX_GPU
    if (!mxIsGPUArray(wa))
#endif
    if (d.norm) for (uint64_t k = 0; k < d.W; ++k) if (num_at(wa, (mwSize)k, "w") < 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "pwznxcorr: a negative weight needs norm = false.");
    const size_t es = d.dtype == QDAS_F64 ? 8 : 4, xs = es * (d.cplx ? 2 : 1);
    const mwSize dims[4] = {(mwSize)T, (mwSize)N, (mwSize)B, (mwSize)d.nlags};
    if (T * N * B * d.nlags == 0) return mxCreateNumericArray(4, dims, cls, d.cplx ? mxCOMPLEX : mxREAL);   /* an empty result: nothing staged or launched */
    int dev = 0;
    const void *pl = dev_in(xl, (size_t)(T * N * B) * xs, "xl", &dev);
    const void *pr = dev_in(xr, (size_t)(T * xrN * (rB ? B : 1)) * xs, "xr", &dev);
    const void *pw = dev_in(wa, (size_t)d.W * es, "w", &dev);
    const size_t bytes = (size_t)(T * N * B * d.nlags) * xs;
    mxArray *host;
    void *y = dev_out(4, dims, cls, d.cplx, dev, bytes, &host);
    int64_t *tab = (int64_t *)malloc(sizeof(int64_t) * d.nlags);
    if (!tab) { if (host) mxDestroyArray(host); CFAIL("out of host memory."); }
    for (uint64_t i = 0; i < d.nlags; ++i) tab[i] = (int64_t)num_at(la, (mwSize)i, "lags");
    const int rc = qdas_pwznxcorr(&d, pl, pr, pw, tab, y, NULL);
    free(tab);
    return finish(rc, host, bytes);
}

/* T = qdas_mex('msfm', csz, F, src, first, max_passes) -- kern/msfm.m:93-113 (UseSecond = UseCross = false), one call for every source set */
static mxArray *cmd_msfm(int nrhs, const mxArray *prhs[]) {
    if (nrhs < 3 || nrhs > 5) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('msfm', csz, F, src, first, max_passes)");
    qdas_eikonal_desc d;
    memset(&d, 0, sizeof d);
    d.C1 = (uint64_t)num_at(prhs[0], 0, "csz"); d.C2 = (uint64_t)num_at(prhs[0], 1, "csz");
    d.dp = 1.0; d.base = 1; d.device = -1;
    const mxArray *sa = prhs[2], *fa = nrhs > 3 ? prhs[3] : NULL;
    if (!mxIsEmpty(sa) && (mxGetClassID(sa) != mxDOUBLE_CLASS || mxIsComplex(sa) || mxGetNumberOfElements(sa) % 2))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "msfm: SourcePoints must be a real double 2 x P array.");
    d.npts = (uint64_t)(mxGetNumberOfElements(sa) / 2);
    const int sets = fa && !mxIsEmpty(fa);
    d.K = sets ? (uint64_t)mxGetNumberOfElements(fa) - 1 : d.npts;
    if (nrhs > 4 && !mxIsEmpty(prhs[4])) d.max_passes = (uint32_t)num_at(prhs[4], 0, "max_passes");
    const mwSize dims[3] = {(mwSize)d.C1, (mwSize)d.C2, (mwSize)d.K};
    if (d.C1 * d.C2 == 0 || d.K == 0 || d.npts == 0)                   /* empty in, empty out */
        return mxCreateNumericArray(3, (const mwSize[3]){(mwSize)d.C1, (mwSize)d.C2, (mwSize)(d.C1 * d.C2 != 0 ? 0 : d.K)}, mxDOUBLE_CLASS, mxREAL);
    if (mxGetClassID(prhs[1]) != mxDOUBLE_CLASS || mxIsComplex(prhs[1])) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "msfm: the speed map must be real double.");
    /* the reference's range errors, its texts (kern/msfm.m:96-99) */
    const double *sp = (const double *)mxGetData(sa);
    for (uint64_t p = 0; p < 2 * d.npts; ++p) if (!(sp[p] >= 1.0)) mexErrMsgIdAndTxt("QUPS:msfm:sourceRange", "Source points must be >= 1 to be within the field.");
    for (int dim = 0; dim < 2; ++dim)
        for (uint64_t p = 0; p < d.npts; ++p)
            if (sp[2 * p + dim] > (double)(dim ? d.C2 : d.C1))
                mexErrMsgIdAndTxt("QUPS:msfm:sourceRange", "Source points must be <= %llu in dimension %d to be in the field.", (unsigned long long)(dim ? d.C2 : d.C1), dim + 1);
    uint64_t *first = NULL;
    if (sets) {
        first = (uint64_t *)malloc(sizeof(uint64_t) * (d.K + 1));
        if (!first) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "out of host memory.");
        for (uint64_t k = 0; k <= d.K; ++k) first[k] = (uint64_t)num_at(fa, (mwSize)k, "first");
        d.set_begin = first;
    }
    int dev = 0;
    const size_t bytes = (size_t)(d.C1 * d.C2 * d.K) * 8;
    const void *c = dev_in(prhs[1], (size_t)(d.C1 * d.C2) * 8, "F", &dev);
    mxArray *host;
    void *T = dev_out(3, dims, mxDOUBLE_CLASS, 0, dev, bytes, &host);
    const int rc = qdas_eikonal(&d, (const double *)c, sp, (double *)T, NULL);
    free(first);
    return finish(rc, host, bytes);
}

/* T = qdas_mex('msfm3d', csz, F, src, first, max_passes) -- kern/msfm.m:93-113 for a volume (UseSecond = UseCross = false), one call for every source set */
static mxArray *cmd_msfm3d(int nrhs, const mxArray *prhs[]) {
    if (nrhs < 3 || nrhs > 5) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('msfm3d', csz, F, src, first, max_passes)");
    qdas_eikonal3_desc d;
    memset(&d, 0, sizeof d);
    d.C1 = (uint64_t)num_at(prhs[0], 0, "csz"); d.C2 = (uint64_t)num_at(prhs[0], 1, "csz"); d.C3 = (uint64_t)num_at(prhs[0], 2, "csz");
    d.dp = 1.0; d.base = 1; d.device = -1;
    const mxArray *sa = prhs[2], *fa = nrhs > 3 ? prhs[3] : NULL;
    if (!mxIsEmpty(sa) && (mxGetClassID(sa) != mxDOUBLE_CLASS || mxIsComplex(sa) || mxGetNumberOfElements(sa) % 3))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "msfm3d: SourcePoints must be a real double 3 x P array.");
    d.npts = (uint64_t)(mxGetNumberOfElements(sa) / 3);
    const int sets = fa && !mxIsEmpty(fa);
    d.K = sets ? (uint64_t)mxGetNumberOfElements(fa) - 1 : d.npts;
    if (nrhs > 4 && !mxIsEmpty(prhs[4])) d.max_passes = (uint32_t)num_at(prhs[4], 0, "max_passes");
    const uint64_t csz[3] = {d.C1, d.C2, d.C3}, CC = d.C1 * d.C2 * d.C3;
    const mwSize dims[4] = {(mwSize)d.C1, (mwSize)d.C2, (mwSize)d.C3, (mwSize)d.K};
    if (CC == 0 || d.K == 0 || d.npts == 0)                            /* empty in, empty out */
        return mxCreateNumericArray(4, (const mwSize[4]){(mwSize)d.C1, (mwSize)d.C2, (mwSize)d.C3, (mwSize)(CC != 0 ? 0 : d.K)}, mxDOUBLE_CLASS, mxREAL);
    if (mxGetClassID(prhs[1]) != mxDOUBLE_CLASS || mxIsComplex(prhs[1])) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "msfm3d: the speed map must be real double.");
    /* the reference's range errors, its texts (kern/msfm.m:96-99) */
    const double *sp = (const double *)mxGetData(sa);
    for (uint64_t p = 0; p < 3 * d.npts; ++p) if (!(sp[p] >= 1.0)) mexErrMsgIdAndTxt("QUPS:msfm:sourceRange", "Source points must be >= 1 to be within the field.");
    for (int dim = 0; dim < 3; ++dim)
        for (uint64_t p = 0; p < d.npts; ++p)
            if (sp[3 * p + dim] > (double)csz[dim])
                mexErrMsgIdAndTxt("QUPS:msfm:sourceRange", "Source points must be <= %llu in dimension %d to be in the field.", (unsigned long long)csz[dim], dim + 1);
    uint64_t *first = NULL, wbytes = 0;
    if (sets) {
        first = (uint64_t *)malloc(sizeof(uint64_t) * (d.K + 1));
        if (!first) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "out of host memory.");
        for (uint64_t k = 0; k <= d.K; ++k) first[k] = (uint64_t)num_at(fa, (mwSize)k, "first");
        d.set_begin = first;
    }
    if (qdas_eikonal3_work_bytes(&d, &wbytes)) { free(first); mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s", qdas_last_error()); }
    int dev = 0;
    const size_t bytes = (size_t)(CC * d.K) * 8;
    const void *c = dev_in(prhs[1], (size_t)CC * 8, "F", &dev);
    if (g_nda >= QDAS_MEX_MAX_DEVARGS) { free(first); CFAIL("too many array arguments."); }
    devarg *w = &g_da[g_nda++];                                         /* the work space: owned, released with the inputs */
    memset(w, 0, sizeof *w);
    if (qdas_device_malloc(&w->owned, (size_t)wbytes, -1)) { free(first); CFAIL("%s", qdas_last_error()); }
    mxArray *host;
    void *T = dev_out(4, dims, mxDOUBLE_CLASS, 0, dev, bytes, &host);
    const int rc = qdas_eikonal3(&d, (const double *)c, sp, (double *)T, w->owned, wbytes, NULL);
    free(first);
    return finish(rc, host, bytes);
}

/* b = qdas_mex('adjoint', sizes, xk, f, Pi, Pr, Pt, cinv, del_tx, apod_tx, a_n, a_m, flags) -- the parfor of bfAdjoint (src/UltrasoundSystem.m:3997-4037).
 * xk: N x V x F single complex (the selected bins of the spectrum, a_mn applied), f: F doubles [Hz] (host), Pi / Pr / Pt: 3 x I / N / M single,
 * cinv: 1 or I single, del_tx: M x V double (t0Offset added), apod_tx: M x V single, a_n: I x N single or [], a_m: I x V single or [].
 * b: I x [N] x [V] single complex. */
static mxArray *cmd_adjoint(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 12) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('adjoint', sizes, xk, f, Pi, Pr, Pt, cinv, del_tx, apod_tx, a_n, a_m, flags)");
    qdas_adjoint_desc d;
    memset(&d, 0, sizeof d);
    d.I = (uint64_t)num_at(prhs[0], 0, "sizes"); d.N = (uint64_t)num_at(prhs[0], 1, "sizes"); d.M = (uint64_t)num_at(prhs[0], 2, "sizes");
    d.V = (uint64_t)num_at(prhs[0], 3, "sizes"); d.Ksel = (uint64_t)num_at(prhs[0], 4, "sizes");
    d.keep_rx = num_at(prhs[11], 0, "flags") != 0; d.keep_tx = num_at(prhs[11], 1, "flags") != 0;
    d.dtype = QDAS_F32; d.device = -1;
    const mxArray *xa = prhs[1], *fa = prhs[2];
    if (!mxIsEmpty(xa) && (mxGetClassID(xa) != mxSINGLE_CLASS || !mxIsComplex(xa)))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "adjoint: the spectrum must be single complex (half precision is insufficient for frequency-domain beamforming; there is no double path).");
    if (mxGetNumberOfElements(fa) != d.Ksel || (d.Ksel && (mxGetClassID(fa) != mxDOUBLE_CLASS || mxIsComplex(fa))))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "adjoint: f must hold one real double per frequency.");
    for (int k = 3; k <= 6; ++k) if (!mxIsEmpty(prhs[k]) && mxGetClassID(prhs[k]) != mxSINGLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "adjoint: Pi, Pr, Pt and cinv must be single.");
    if (!mxIsEmpty(prhs[7]) && mxGetClassID(prhs[7]) != mxDOUBLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "adjoint: del_tx must be double.");
    for (int k = 8; k <= 10; ++k) if (!mxIsEmpty(prhs[k]) && mxGetClassID(prhs[k]) != mxSINGLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "adjoint: apod_tx, a_n and a_m must be single.");
    d.cinv_count = (uint64_t)mxGetNumberOfElements(prhs[6]);
    d.freq = (const double *)mxGetData(fa);
    const mwSize dims[3] = {(mwSize)d.I, (mwSize)(d.keep_rx ? d.N : 1), (mwSize)(d.keep_tx ? d.V : 1)};
    const size_t bytes = (size_t)dims[0] * dims[1] * dims[2] * 8;
    if (!bytes) return mxCreateNumericArray(3, dims, mxSINGLE_CLASS, mxCOMPLEX);                    /* empty in, empty out */
    int dev = 0;
    const void *x = dev_in(xa, (size_t)(d.N * d.V * d.Ksel) * 8, "xk", &dev);
    d.Pi = (const float *)dev_in(prhs[3], 3 * (size_t)d.I * 4, "Pi", &dev);
    d.Pr = (const float *)dev_in(prhs[4], 3 * (size_t)d.N * 4, "Pr", &dev);
    d.Pt = (const float *)dev_in(prhs[5], 3 * (size_t)d.M * 4, "Pt", &dev);
    d.cinv = (const float *)dev_in(prhs[6], (size_t)d.cinv_count * 4, "cinv", &dev);
    d.del_tx = (const double *)dev_in(prhs[7], (size_t)(d.M * d.V) * 8, "del_tx", &dev);
    d.apod_tx = (const float *)dev_in(prhs[8], (size_t)(d.M * d.V) * 4, "apod_tx", &dev);
    d.a_n = mxIsEmpty(prhs[9]) ? NULL : (const float *)dev_in(prhs[9], (size_t)(d.I * d.N) * 4, "a_n", &dev);
    d.a_m = mxIsEmpty(prhs[10]) ? NULL : (const float *)dev_in(prhs[10], (size_t)(d.I * d.V) * 4, "a_m", &dev);
    mxArray *host;
    void *b = dev_out(3, dims, mxSINGLE_CLASS, 1, dev, bytes, &host);
    return finish(qdas_adjoint(&d, x, b, NULL), host, bytes);
}

/* b = qdas_mex('migration', sizes, x, tau, gamma, params, flags) -- bfMigration's loop over blocks of transmits (src/UltrasoundSystem.m:4801-4855).
 * x: T x N x M x frames single complex, tau: N x M double (delays(seq, xdc) at c0), gamma: M double, params = [fs fmod t0 c0 pitch],
 * flags = [interp keep_tx jacobian] (interp: 0 nearest, 1 linear, 2 cubic, 3 lanczos3, 5 cubic_dev).  b: min(T,F) x min(N,K) x [M] x frames single complex.
 * Transform lengths the in-LDS kernels do not take raise QUPS:das_spec:qdas with the library's text (the caller composes the image in MATLAB then). */
static mxArray *cmd_migration(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 6) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('migration', sizes, x, tau, gamma, params, flags)");
    qdas_migration_desc d;
    memset(&d, 0, sizeof d);
    d.T = (uint64_t)num_at(prhs[0], 0, "sizes"); d.N = (uint64_t)num_at(prhs[0], 1, "sizes"); d.M = (uint64_t)num_at(prhs[0], 2, "sizes");
    d.frames = (uint64_t)num_at(prhs[0], 3, "sizes"); d.F = (uint64_t)num_at(prhs[0], 4, "sizes"); d.K = (uint64_t)num_at(prhs[0], 5, "sizes");
    d.fs = num_at(prhs[4], 0, "params"); d.fmod = num_at(prhs[4], 1, "params"); d.t0 = num_at(prhs[4], 2, "params");
    d.c0 = num_at(prhs[4], 3, "params"); d.pitch = num_at(prhs[4], 4, "params");
    d.flag = (int32_t)num_at(prhs[5], 0, "flags"); d.keep_tx = num_at(prhs[5], 1, "flags") != 0; d.jacobian = num_at(prhs[5], 2, "flags") != 0;
    d.device = -1;
    const mxArray *xa = prhs[1];
    if (!mxIsEmpty(xa) && (mxGetClassID(xa) != mxSINGLE_CLASS || !mxIsComplex(xa)))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "migration: the data must be single complex.");
    for (int k = 2; k <= 3; ++k)
        if (!mxIsEmpty(prhs[k]) && (mxGetClassID(prhs[k]) != mxDOUBLE_CLASS || mxIsComplex(prhs[k]))) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "migration: tau and gamma must be real double.");
    const uint64_t Tn = d.T < d.F ? d.T : d.F, Nn = d.N < d.K ? d.N : d.K;
    const mwSize dims[4] = {(mwSize)Tn, (mwSize)Nn, (mwSize)(d.keep_tx ? d.M : 1), (mwSize)d.frames};
    const size_t bytes = (size_t)dims[0] * dims[1] * dims[2] * dims[3] * 8;
    if (!bytes || !d.M) return mxCreateNumericArray(4, dims, mxSINGLE_CLASS, mxCOMPLEX);           /* empty in, empty out */
    int dev = 0;
    const void *x = dev_in(xa, (size_t)(d.T * d.N * d.M * d.frames) * 8, "x", &dev);
    d.tau = (const double *)dev_in(prhs[2], (size_t)(d.N * d.M) * 8, "tau", &dev);
    d.gamma = (const double *)dev_in(prhs[3], (size_t)d.M * 8, "gamma", &dev);
    mxArray *host;
    void *b = dev_out(4, dims, mxSINGLE_CLASS, 1, dev, bytes, &host);
    return finish(qdas_migration(&d, x, b, NULL), host, bytes);
}

/* y = qdas_mex('refocus', sizes, x, Hi, t0, fs) -- lines 3735-3762 of the reference's refocus (src/UltrasoundSystem.m): fft, time-alignment phase, Hi applied over
 * the transmits, phase back, ifft.  sizes = [T N V M frames] (the gateway takes its extents from a sizes row like every other command); x: T x N x V x frames
 * single complex; Hi: M x V x T single complex, the reference's own array, unchanged; t0: one real double or one per pulse (V), a HOST array; fs: a real
 * scalar.  y: T x N x M x frames single complex; its time axis starts at min(t0).  A record length the in-LDS kernels do not take raises QUPS:das_spec:qdas
 * with the library's text (the caller runs the reference's lines in MATLAB then).  The work space is staged like an input and released with them. */
static mxArray *cmd_refocus(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 5) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('refocus', sizes, x, Hi, t0, fs)");
    qdas_refocus_desc d;
    memset(&d, 0, sizeof d);
    d.T = (uint64_t)num_at(prhs[0], 0, "sizes"); d.N = (uint64_t)num_at(prhs[0], 1, "sizes"); d.V = (uint64_t)num_at(prhs[0], 2, "sizes");
    d.M = (uint64_t)num_at(prhs[0], 3, "sizes"); d.frames = (uint64_t)num_at(prhs[0], 4, "sizes");
    d.fs = num_at(prhs[4], 0, "fs");
    d.device = -1;
    const mxArray *xa = prhs[1], *ha = prhs[2], *ta = prhs[3];
    if ((!mxIsEmpty(xa) && (mxGetClassID(xa) != mxSINGLE_CLASS || !mxIsComplex(xa))) || (!mxIsEmpty(ha) && (mxGetClassID(ha) != mxSINGLE_CLASS || !mxIsComplex(ha))))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "refocus: the data and Hi must be single complex.");
    const mwSize dims[4] = {(mwSize)d.T, (mwSize)d.N, (mwSize)d.M, (mwSize)d.frames};
    const size_t bytes = (size_t)dims[0] * dims[1] * dims[2] * dims[3] * 8;
    if (!bytes || !d.V) return mxCreateNumericArray(4, dims, mxSINGLE_CLASS, mxCOMPLEX);           /* empty in, or no pulses to sum: empty / zeros out */
    const size_t nt0 = (size_t)mxGetNumberOfElements(ta);
    if (mxGetClassID(ta) != mxDOUBLE_CLASS || mxIsComplex(ta) || (nt0 != 1 && nt0 != d.V)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "refocus: t0 must hold one real double, or one per pulse.");
    const double *t0 = (const double *)mxGetData(ta);
    d.one_t0 = nt0 == 1;
    d.t0_out = t0[0];
    for (size_t v = 1; v < nt0; ++v) if (t0[v] < d.t0_out) d.t0_out = t0[v];
    uint64_t wbytes = 0;
    if (qdas_refocus_work_bytes(&d, &wbytes)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s", qdas_last_error());
    int dev = 0;
    const void *x = dev_in(xa, (size_t)(d.T * d.N * d.V * d.frames) * 8, "x", &dev);
    const void *Hi = dev_in(ha, (size_t)(d.M * d.V * d.T) * 8, "Hi", &dev);
    if (!d.one_t0) d.t0 = (const double *)dev_in(ta, nt0 * 8, "t0", &dev);
    if (g_nda >= QDAS_MEX_MAX_DEVARGS) CFAIL("too many array arguments.");
    devarg *w = &g_da[g_nda++];                                                                     /* the work space: owned, released with the inputs */
    memset(w, 0, sizeof *w);
    if (qdas_device_malloc(&w->owned, (size_t)wbytes, -1)) CFAIL("%s", qdas_last_error());
    mxArray *host;
    void *y = dev_out(4, dims, mxSINGLE_CLASS, 1, dev, bytes, &host);
    return finish(qdas_refocus(&d, x, Hi, y, w->owned, wbytes), host, bytes);
}

/* the grid and the rays of the two straight-ray commands: gsz = [X Z J sa sb ...]; x, z: real vectors of one class (single | double) with X and Z values,
 * strictly increasing (the caller's promise, as in the C ABI: wbilerpg.m asserts it before it gets here); pa, pb: 2 x J arrays of that class, a column is
 * one point (x; z) -- or, with sa / sb = 0, 2 x 1: one point for every ray. */
static mxClassID ray_args(const char *who, const mxArray *prhs[], qdas_raypaths_desc *d, int *dev) {
    memset(d, 0, sizeof *d);
    d->X = (uint64_t)num_at(prhs[0], 0, "gsz"); d->Z = (uint64_t)num_at(prhs[0], 1, "gsz"); d->J = (uint64_t)num_at(prhs[0], 2, "gsz");
    d->pa_stride = num_at(prhs[0], 3, "gsz") != 0; d->pb_stride = num_at(prhs[0], 4, "gsz") != 0;
    d->device = -1;
    const mxClassID cls = mxGetClassID(prhs[1]);
    if (cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s: the grid vectors must be single or double.", who);
    for (int k = 1; k <= 4; ++k)
        if (mxGetClassID(prhs[k]) != cls || mxIsComplex(prhs[k])) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s: grid vectors and end points must be real and of one class.", who);
    d->dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32;
    if (d->J == 0) return cls;
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4;
    d->xg = dev_in(prhs[1], (size_t)d->X * es, "x", dev);
    d->zg = dev_in(prhs[2], (size_t)d->Z * es, "z", dev);
    d->pa = dev_in(prhs[3], (size_t)(d->pa_stride ? d->J : 1) * 2 * es, "pa", dev);
    d->pb = dev_in(prhs[4], (size_t)(d->pb_stride ? d->J : 1) * 2 * es, "pb", dev);
    return cls;
}

/* a further output of `bytes` bytes the command owns on the device: released with the inputs */
static void *dev_extra(size_t bytes) {
    if (g_nda >= QDAS_MEX_MAX_DEVARGS) CFAIL("too many array arguments.");
    devarg *w = &g_da[g_nda++];
    memset(w, 0, sizeof *w);
    if (qdas_device_malloc(&w->owned, bytes, -1)) CFAIL("%s", qdas_last_error());
    return w->owned;
}

/* [cxy, ixo, iyo] = qdas_mex('wbilerp', gsz, x, y, pa, pb) -- kern/wbilerpg.m without r: each output is 4 (X + Y + 1) x J; the indices are int32, 1-based and 0
 * where the slot is empty, as wbilerpg returns them (ixo and iyo come back as host arrays).  Rays outside the grid are clipped without the warning. */
static void cmd_wbilerp(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    if (nrhs != 5) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('wbilerp', gsz, x, y, pa, pb)");
    qdas_raypaths_desc d;
    int dev = 0;
    const mxClassID cls = ray_args("wbilerp", prhs, &d, &dev);
    const uint64_t K4 = 4 * qdas_raypaths_slots(d.X, d.Z);
    const mwSize dims[2] = {(mwSize)K4, (mwSize)d.J};
    if (d.J == 0) {
        plhs[0] = mxCreateNumericArray(2, dims, cls, mxREAL);
        for (int k = 1; k < nlhs && k < 3; ++k) plhs[k] = mxCreateNumericArray(2, dims, mxINT32_CLASS, mxREAL);
        return;
    }
    const size_t n = (size_t)(K4 * d.J), bytes = n * (cls == mxDOUBLE_CLASS ? 8 : 4);
    int32_t *ix = (int32_t *)dev_extra(n * 4), *iz = (int32_t *)dev_extra(n * 4);
    mxArray *host, *hi[2] = {mxCreateNumericArray(2, dims, mxINT32_CLASS, mxREAL), mxCreateNumericArray(2, dims, mxINT32_CLASS, mxREAL)};
    void *w = dev_out(2, dims, cls, 0, dev, bytes, &host);
    int rc = qdas_raypaths_weights(&d, w, ix, iz);
    rc = fetch_out(rc, host, bytes);
    if (!rc) rc = qdas_device_copy(mxGetData(hi[0]), ix, n * 4, 1, -1);
    if (!rc) rc = qdas_device_copy(mxGetData(hi[1]), iz, n * 4, 1, -1);
    for (int k = 0; k < 2; ++k) {
        int32_t *v = (int32_t *)mxGetData(hi[k]);
        for (size_t i = 0; i < n; ++i) v[i] += 1;
        if (rc || nlhs < k + 2) { mxDestroyArray(hi[k]); hi[k] = NULL; }
    }
    plhs[0] = conclude(rc, host);
    if (hi[0]) plhs[1] = hi[0];
    if (hi[1]) plhs[2] = hi[1];
}

/* [v, len] = qdas_mex('rayintegrals', gsz, x, z, pa, pb, maps) -- what globalAverageC.m and the product ``f(:)' * rayPaths(...)`` compute, without the triplets:
 * v(j, f) = the integral of the bilinear interpolant of map f along ray j (J x F), len(j) the length of the part of the ray inside the grid (a host array).
 * gsz = [X Z J sa sb F xstride zstride]: maps holds F maps of X Z values of the grid's class; node (ix, iz) of a map is element 1 + ix xstride + iz zstride --
 * a Z x X array: [Z 1], an X x Z array: [1 X]. */
static void cmd_rayintegrals(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    if (nrhs != 6) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('rayintegrals', gsz, x, z, pa, pb, maps)");
    qdas_raypaths_desc d;
    int dev = 0;
    const uint64_t F = (uint64_t)num_at(prhs[0], 5, "gsz");
    const int64_t xstride = (int64_t)num_at(prhs[0], 6, "gsz"), zstride = (int64_t)num_at(prhs[0], 7, "gsz");
    const mxClassID cls = mxGetClassID(prhs[1]);
    if (!mxIsEmpty(prhs[5]) && (mxGetClassID(prhs[5]) != cls || mxIsComplex(prhs[5]))) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "rayintegrals: the maps must be real and of the grid's class.");
    ray_args("rayintegrals", prhs, &d, &dev);
    d.F = F; d.xstride = xstride; d.zstride = zstride;
    const mwSize dims[2] = {(mwSize)d.J, (mwSize)F}, ldims[2] = {(mwSize)d.J, 1};
    if (d.J == 0 || F == 0) {
        release_devargs();
        plhs[0] = mxCreateNumericArray(2, dims, cls, mxREAL);
        if (nlhs > 1) plhs[1] = mxCreateNumericArray(2, ldims, cls, mxREAL);
        return;
    }
    if (xstride < 0 || zstride < 0 || (uint64_t)xstride * (d.X - 1) + (uint64_t)zstride * (d.Z - 1) >= d.X * d.Z) CFAIL("rayintegrals: the strides reach outside a map of X Z values.");
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4, bytes = (size_t)(d.J * F) * es;
    const void *maps = dev_in(prhs[5], (size_t)(d.X * d.Z * F) * es, "maps", &dev);
    void *len = dev_extra((size_t)d.J * es);
    mxArray *host, *hl = mxCreateNumericArray(2, ldims, cls, mxREAL);
    void *y = dev_out(2, dims, cls, 0, dev, bytes, &host);
    int rc = qdas_raypaths_integrate(&d, maps, y, len);
    rc = fetch_out(rc, host, bytes);
    if (!rc) rc = qdas_device_copy(mxGetData(hl), len, (size_t)d.J * es, 1, -1);
    if (rc || nlhs < 2) { mxDestroyArray(hl); hl = NULL; }
    plhs[0] = conclude(rc, host);
    if (hl) plhs[1] = hl;
}

/* [g, col] = qdas_mex('raybackproject', gsz, x, z, pa, pb, r) -- the product ``w' * r`` with w the matrix kern/rayPaths.m returns, without the triplets:
 * g(:, f) = sum_j w_j r(j, f), one map of X Z values per column of r (J x F, of the grid's class), and col = sum_j w_j, the matrix's column sums (a host array).
 * gsz = [X Z J sa sb F xstride zstride] as 'rayintegrals' takes it; node (ix, iz) of a map is element 1 + ix xstride + iz zstride, and because every element
 * of an output must be written the strides are those of a Z x X array, [Z 1], or of an X x Z array, [1 X].  F = 0 with two outputs computes col alone. */
static void cmd_raybackproject(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    if (nrhs != 6) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('raybackproject', gsz, x, z, pa, pb, r)");
    qdas_raypaths_desc d;
    int dev = 0;
    const uint64_t F = (uint64_t)num_at(prhs[0], 5, "gsz");
    const int64_t xstride = (int64_t)num_at(prhs[0], 6, "gsz"), zstride = (int64_t)num_at(prhs[0], 7, "gsz");
    const mxClassID cls = mxGetClassID(prhs[1]);
    ray_args("raybackproject", prhs, &d, &dev);
    if (!mxIsEmpty(prhs[5]) && (mxGetClassID(prhs[5]) != cls || mxIsComplex(prhs[5]))) CFAIL("raybackproject: r must be real and of the grid's class.");
    d.F = F; d.xstride = xstride; d.zstride = zstride;
    const mwSize dims[2] = {(mwSize)(d.X * d.Z), (mwSize)F}, cdims[2] = {(mwSize)(d.X * d.Z), 1};
    if (d.J == 0 || (F == 0 && nlhs < 2)) {                                                          /* zeros: nothing to sum */
        release_devargs();
        plhs[0] = mxCreateNumericArray(2, dims, cls, mxREAL);
        if (nlhs > 1) plhs[1] = mxCreateNumericArray(2, cdims, cls, mxREAL);
        return;
    }
    if (!((xstride == 1 && zstride == (int64_t)d.X) || (zstride == 1 && xstride == (int64_t)d.Z))) CFAIL("raybackproject: the strides must be [Z 1] or [1 X]: every element of a map of X Z values is written.");
    const size_t es = cls == mxDOUBLE_CLASS ? 8 : 4, bytes = (size_t)(d.X * d.Z * F) * es, cbytes_ = (size_t)(d.X * d.Z) * es;
    const void *r = F ? dev_in(prhs[5], (size_t)(d.J * F) * es, "r", &dev) : NULL;
    void *col = nlhs > 1 ? dev_extra(cbytes_) : NULL;
    mxArray *host = NULL, *hc = nlhs > 1 ? mxCreateNumericArray(2, cdims, cls, mxREAL) : NULL;
    void *g = F ? dev_out(2, dims, cls, 0, dev, bytes, &host) : NULL;
    int rc = qdas_raypaths_backproject(&d, r, g, col);
    if (F) rc = fetch_out(rc, host, bytes);
    if (!rc && hc) rc = qdas_device_copy(mxGetData(hc), col, cbytes_, 1, -1);
    if (rc && hc) { mxDestroyArray(hc); hc = NULL; }
    plhs[0] = F ? conclude(rc, host) : conclude(rc, mxCreateNumericArray(2, dims, cls, mxREAL));
    if (hc) plhs[1] = hc;
}

/* an axis of the scan conversion: a real host vector of any numeric class, as float64 on the device; angles arrive in degrees as the reference keeps them and
 * become radians here with a * pi / 180 ([] -> NULL, *n = 0) */
static const double *sc_axis(const mxArray *a, uint64_t *n, int degrees, const char *what) {
    *n = a ? (uint64_t)mxGetNumberOfElements(a) : 0;
    if (!*n) return NULL;
    (void)num_at(a, 0, what);                                                                        /* (raises on a complex or non-numeric array, before anything is held) */
    double *h = (double *)malloc((size_t)*n * sizeof(double));
    if (!h) CFAIL("%s: out of memory.", what);
    for (uint64_t i = 0; i < *n; ++i) h[i] = degrees ? num_at(a, (mwSize)i, what) * 3.14159265358979323846 / 180.0 : num_at(a, (mwSize)i, what);
    void *d = dev_extra((size_t)*n * sizeof(double));
    const int rc = qdas_device_copy(d, h, (size_t)*n * sizeof(double), 0, -1);
    free(h);
    if (rc) CFAIL("%s", qdas_last_error());
    return (const double *)d;
}

/* bc = qdas_mex('scanconvert', b, r, a, e, origin, x, y, z, opts) -- ScanPolar.scanConvert (src/ScanPolar.m:143-201) with e = [] and ScanSpherical.scanConvert
 * (src/ScanSpherical.m:121-188) otherwise.  b: single | double, real or complex, R x A x pages (R x A x E x pages) as MATLAB holds it (a host array or, in a GPU
 * build, a gpuArray); r [m], a, e [degrees], origin (3 values), x, y, z [m]: real host vectors, strictly increasing (y is not read for a polar scan and may be
 * []).  opts: [] | [pre db_floor fill] | a struct with those fields; pre = 0: none, 1: abs, 2: dB (mod2db applied to the samples BEFORE the interpolation),
 * defaults 0, -Inf, NaN.  bc: Z x X x pages (Z x X x Y x pages) of b's class -- real when pre is 1 or 2 --, fill outside the sector. */
static mxArray *cmd_scanconvert(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 9) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('scanconvert', b, r, a, e, origin, x, y, z, opts)");
    const mxArray *ba = prhs[0], *o = prhs[8];
    const mxClassID cls = mxGetClassID(ba);
    if (cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "scanconvert: b must be single or double (half-precision images are not built).");
    qdas_scanconvert_desc d;
    memset(&d, 0, sizeof d);
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32;
    d.cplx = mxIsComplex(ba) ? 1 : 0;
    d.device = -1;
    d.pre = QDAS_SC_PRE_NONE; d.db_floor = -INFINITY; d.fill = NAN;
    if (o && !mxIsEmpty(o)) {
        const mxArray *f;
        if (mxIsStruct(o)) {
            if ((f = mxGetField(o, 0, "pre"))) d.pre = (int32_t)num_at(f, 0, "opts.pre");
            if ((f = mxGetField(o, 0, "db_floor"))) d.db_floor = num_at(f, 0, "opts.db_floor");
            if ((f = mxGetField(o, 0, "fill"))) d.fill = num_at(f, 0, "opts.fill");
        } else {
            const size_t no = mxGetNumberOfElements(o);
            d.pre = (int32_t)num_at(o, 0, "opts");
            if (no > 1) d.db_floor = num_at(o, 1, "opts");
            if (no > 2) d.fill = num_at(o, 2, "opts");
        }
    }
    for (int k = 0; k < 3; ++k) d.origin[k] = num_at(prhs[4], (mwSize)k, "origin");
    d.r = sc_axis(prhs[1], &d.R, 0, "r");
    d.a = sc_axis(prhs[2], &d.A, 1, "a");
    d.e = sc_axis(prhs[3], &d.E, 1, "e");
    d.x = sc_axis(prhs[5], &d.X, 0, "x");
    uint64_t ny = 0;
    const double *yv = sc_axis(prhs[6], &ny, 0, "y");
    if (d.E) { d.y = yv; d.Y = ny; }
    d.z = sc_axis(prhs[7], &d.Z, 0, "z");
    const uint64_t per = d.R * d.A * (d.E ? d.E : 1), nb = (uint64_t)mxGetNumberOfElements(ba);
    if (!per || nb % per) CFAIL("scanconvert: b holds %llu samples, not pages of R x A%s = %llu.", (unsigned long long)nb, d.E ? " x E" : "", (unsigned long long)per);
    d.P = nb / per;
    d.sr = 1; d.sa = (int64_t)d.R; d.se = d.E ? (int64_t)(d.R * d.A) : 0; d.sp = (int64_t)per;
    const int ocplx = d.cplx && d.pre == QDAS_SC_PRE_NONE;
    const mwSize dims[4] = {(mwSize)d.Z, (mwSize)d.X, (mwSize)(d.E ? d.Y : d.P), (mwSize)d.P};
    const mwSize nd = d.E ? 4 : 3;
    const uint64_t nout = d.Z * d.X * (d.E ? d.Y : 1) * d.P;
    const size_t es = (cls == mxDOUBLE_CLASS ? 8 : 4), bytes = (size_t)nout * es * (ocplx ? 2 : 1);
    if (nout == 0) {
        const int rc = qdas_scanconvert(&d, NULL, NULL);                                             /* (an empty call is still validated) */
        if (rc) CFAIL("%s", qdas_last_error());
        release_devargs();
        return mxCreateNumericArray(nd, dims, cls, ocplx ? mxCOMPLEX : mxREAL);
    }
    int dev = 0;
    const void *b = dev_in(ba, (size_t)nb * es * (d.cplx ? 2 : 1), "b", &dev);
    mxArray *host;
    void *out = dev_out(nd, dims, cls, ocplx, dev, bytes, &host);
    return finish(qdas_scanconvert(&d, b, out), host, bytes);
}

/* y = qdas_mex('demod', x, b, prm, t0) -- downmix(chd, fc) -> filter(chd, D) -> downsample(chd, ratio) (src/ChannelData.m:757-807, :857-888, :1042-1058) in one
 * pass (qdas_demod).  x: int16 | single | double (single, double: real or complex), T x C (any trailing dimensions count as traces) as MATLAB holds it: time
 * fastest (a host array or, in a GPU build, a gpuArray).  b: the real FIR taps, a host vector of any numeric class (converted to the data's precision).
 * prm = [T fc fs ratio gdiv] (T = size(x, 1); gdiv optional, default 1); t0: one start time, or G of them -- trace c (0-based) starts at t0(1 + mod(floor(c / gdiv), G)), so
 * gdiv = N, G = M gives one start time per transmit of a T x N x M record.  y: ceil(T / ratio) x C complex single (double for double data); real data give half
 * the analytic amplitude, as the composition does.  The new time axis, t0 - (numel(b) - 1) / 2 / fs and fs / ratio, is the caller's bookkeeping.  Half output
 * is not offered here (MATLAB has no half class). */
static mxArray *cmd_demod(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 4) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('demod', x, b, prm, t0)");
    const mxArray *xa = prhs[0];
    const mxClassID cls = mxGetClassID(xa);
    const int cplx = mxIsComplex(xa) ? 1 : 0;
    if ((cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS && cls != mxINT16_CLASS) || (cls == mxINT16_CLASS && cplx))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "demod: x must be int16 (real), single or double.");
    qdas_demod_desc d;
    memset(&d, 0, sizeof d);
    d.in_type = cls == mxINT16_CLASS ? QDAS_DEMOD_I16 : cls == mxSINGLE_CLASS ? (cplx ? QDAS_DEMOD_C64 : QDAS_DEMOD_F32) : (cplx ? QDAS_DEMOD_C128 : QDAS_DEMOD_F64);
    d.device = -1;
    const size_t np = mxGetNumberOfElements(prhs[2]);
    const double Tn = num_at(prhs[2], 0, "prm"), fc = num_at(prhs[2], 1, "prm"), fs = num_at(prhs[2], 2, "prm"), ratio = num_at(prhs[2], 3, "prm");
    const double gdiv = np > 4 ? num_at(prhs[2], 4, "prm") : 1.0;
    if (!(Tn >= 0.0) || Tn != floor(Tn) || !(ratio >= 1.0) || ratio != floor(ratio) || !(gdiv >= 1.0) || gdiv != floor(gdiv) || !(fs > 0.0))
        CFAIL("demod: prm = [T fc fs ratio gdiv] with fs > 0, an integer T >= 0 and positive integers ratio, gdiv.");
    const uint64_t nx = (uint64_t)mxGetNumberOfElements(xa);
    d.T = (uint64_t)Tn; d.C = d.T ? nx / d.T : 0;
    if (d.T ? nx % d.T != 0 : nx != 0) CFAIL("demod: x holds %llu samples, not traces of T = %llu.", (unsigned long long)nx, (unsigned long long)d.T);
    d.K = (uint64_t)mxGetNumberOfElements(prhs[1]); d.R = (uint64_t)ratio;
    d.G = (uint64_t)mxGetNumberOfElements(prhs[3]); d.gdiv = (uint64_t)gdiv;
    const uint64_t J = qdas_demod_len(d.T, d.R);
    d.x_ld = d.T; d.out_ld = J;
    d.fc_over_fs = fc / fs; d.step = fc * ratio / fs;
    const int dbl = cls == mxDOUBLE_CLASS;
    const mxClassID ocls = dbl ? mxDOUBLE_CLASS : mxSINGLE_CLASS;
    const mwSize dims[2] = {(mwSize)J, (mwSize)d.C};
    if (d.K == 0 || d.G == 0) CFAIL("demod: b and t0 must not be empty.");
    if (J * d.C == 0) {
        const int rc = qdas_demod(&d, NULL, NULL, NULL);                                             /* (an empty call is still validated) */
        if (rc) CFAIL("%s", qdas_last_error());
        release_devargs();
        return mxCreateNumericArray(2, dims, ocls, mxCOMPLEX);
    }
    /* the taps in the data's precision and the start phases frac(fc t0), staged on the device */
    const size_t rs = dbl ? 8 : 4;
    (void)num_at(prhs[1], 0, "b"); (void)num_at(prhs[3], 0, "t0");      /* whatever raises (the class of b / t0, the device blocks) does so before the host blocks exist: */
    void *db = dev_extra((size_t)d.K * rs), *dc = dev_extra((size_t)d.G * sizeof(double));      /* num_at's refusals do not depend on the index below numel */
    void *hb = malloc((size_t)d.K * rs);
    double *hc = (double *)malloc((size_t)d.G * sizeof(double));
    if (!hb || !hc) { free(hb); free(hc); CFAIL("demod: out of memory."); }
    for (uint64_t k = 0; k < d.K; ++k) { const double v = num_at(prhs[1], (mwSize)k, "b"); if (dbl) ((double *)hb)[k] = v; else ((float *)hb)[k] = (float)v; }
    for (uint64_t k = 0; k < d.G; ++k) { const double c = fc * num_at(prhs[3], (mwSize)k, "t0"); hc[k] = c - floor(c); }
    int rc = qdas_device_copy(db, hb, (size_t)d.K * rs, 0, -1);
    if (!rc) rc = qdas_device_copy(dc, hc, (size_t)d.G * sizeof(double), 0, -1);
    free(hb); free(hc);
    if (rc) CFAIL("%s", qdas_last_error());
    d.cyc0 = (const double *)dc;
    int dev = 0;
    const size_t es = cls == mxINT16_CLASS ? 2 : (dbl ? 8 : 4) * (cplx ? 2 : 1), bytes = (size_t)(J * d.C) * rs * 2;
    const void *x = dev_in(xa, (size_t)nx * es, "x", &dev);
    mxArray *host;
    void *out = dev_out(2, dims, ocls, 1, dev, bytes, &host);
    return finish(qdas_demod(&d, x, db, out), host, bytes);
}

/* y = qdas_mex('resample', x, h, prm) -- the rational-rate polyphase FIR (qdas_resample): y(j) = sum_i h(off + j q - i p) X(i) (0-based) over the taps that
 * exist, J outputs per trace.  x: int16 | single | double (single, double: real or complex), T x C (any trailing dimensions count as traces) as MATLAB holds it:
 * time fastest (a host array or, in a GPU build, a gpuArray).  h: the real taps, a host vector of any numeric class (converted to the data's precision).
 * prm = [T p q off J edge], edge 0: zeros outside the record, 1: odd reflection (optional, default 0).  With h = resample's design (p h / sum(h), odd length K),
 * off = (K - 1) / 2 and J = ceil(T p / q) this is MATLAB's uniform resample(x, p, q); with p = q = 1, h = conv(b, flip(b)), off = numel(b) - 1, J = T and
 * edge = 1 it is filtfilt(b, 1, x); with off = 0 and J = ceil(((T - 1) p + K) / q), upfirdn(x, h, p, q).  y: J x C, single for int16 and single data, double
 * for double, complex for complex x. */
static mxArray *cmd_resample(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 3) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('resample', x, h, prm)");
    const mxArray *xa = prhs[0];
    const mxClassID cls = mxGetClassID(xa);
    const int cplx = mxIsComplex(xa) ? 1 : 0;
    if ((cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS && cls != mxINT16_CLASS) || (cls == mxINT16_CLASS && cplx))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "resample: x must be int16 (real), single or double.");
    qdas_resample_desc d;
    memset(&d, 0, sizeof d);
    d.in_type = cls == mxINT16_CLASS ? QDAS_RESAMPLE_I16 : cls == mxSINGLE_CLASS ? (cplx ? QDAS_RESAMPLE_C64 : QDAS_RESAMPLE_F32) : (cplx ? QDAS_RESAMPLE_C128 : QDAS_RESAMPLE_F64);
    d.device = -1;
    const size_t np = mxGetNumberOfElements(prhs[2]);
    const double Tn = num_at(prhs[2], 0, "prm"), pn = num_at(prhs[2], 1, "prm"), qn = num_at(prhs[2], 2, "prm"), on = num_at(prhs[2], 3, "prm"), Jn = num_at(prhs[2], 4, "prm");
    const double en = np > 5 ? num_at(prhs[2], 5, "prm") : 0.0;
    if (!(Tn >= 0.0) || Tn != floor(Tn) || !(pn >= 1.0) || pn != floor(pn) || !(qn >= 1.0) || qn != floor(qn) || !(on >= 0.0) || on != floor(on) ||
        !(Jn >= 0.0) || Jn != floor(Jn) || (en != 0.0 && en != 1.0) || Tn >= 1e15 || pn >= 1e15 || qn >= 1e15 || on >= 1e15 || Jn >= 1e15)
        CFAIL("resample: prm = [T p q off J edge] with integers T, off, J >= 0, p, q >= 1 and edge 0 | 1.");
    const uint64_t nx = (uint64_t)mxGetNumberOfElements(xa);
    d.T = (uint64_t)Tn; d.C = d.T ? nx / d.T : 0;
    if (d.T ? nx % d.T != 0 : nx != 0) CFAIL("resample: x holds %llu samples, not traces of T = %llu.", (unsigned long long)nx, (unsigned long long)d.T);
    d.K = (uint64_t)mxGetNumberOfElements(prhs[1]);
    d.p = (uint64_t)pn; d.q = (uint64_t)qn; d.off = (uint64_t)on; d.J = (uint64_t)Jn; d.edge = (int32_t)en;
    d.x_ld = d.T; d.out_ld = d.J;
    const int dbl = cls == mxDOUBLE_CLASS;
    const mxClassID ocls = dbl ? mxDOUBLE_CLASS : mxSINGLE_CLASS;
    const mwSize dims[2] = {(mwSize)d.J, (mwSize)d.C};
    if (d.K == 0) CFAIL("resample: h must not be empty.");
    if (d.J * d.C == 0) {
        const int rc = qdas_resample(&d, NULL, NULL, NULL);                                          /* (an empty call is still validated) */
        if (rc) CFAIL("%s", qdas_last_error());
        release_devargs();
        return mxCreateNumericArray(2, dims, ocls, cplx ? mxCOMPLEX : mxREAL);
    }
    const size_t rs = dbl ? 8 : 4;
    (void)num_at(prhs[1], 0, "h");                                      /* whatever raises (the class of h, the device block) does so before the host block exists */
    void *dh = dev_extra((size_t)d.K * rs);
    void *hh = malloc((size_t)d.K * rs);
    if (!hh) CFAIL("resample: out of memory.");
    for (uint64_t k = 0; k < d.K; ++k) { const double v = num_at(prhs[1], (mwSize)k, "h"); if (dbl) ((double *)hh)[k] = v; else ((float *)hh)[k] = (float)v; }
    const int rc = qdas_device_copy(dh, hh, (size_t)d.K * rs, 0, -1);
    free(hh);
    if (rc) CFAIL("%s", qdas_last_error());
    int dev = 0;
    const size_t es = cls == mxINT16_CLASS ? 2 : rs * (cplx ? 2 : 1), bytes = (size_t)(d.J * d.C) * rs * (cplx ? 2 : 1);
    const void *x = dev_in(xa, (size_t)nx * es, "x", &dev);
    mxArray *host;
    void *out = dev_out(2, dims, ocls, cplx, dev, bytes, &host);
    return finish(qdas_resample(&d, x, dh, out), host, bytes);
}

/* rec = qdas_mex('fdtd', med, pml, s, src, sen, prm) -- Nt steps of the 2-D acoustic FDTD scheme (qdas_fdtd, include/qdas.h) from rest, on tables the caller
 * prepared (qups_amd/fdtd.py `prepare` is the recipe: the medium extended into the PML by edge replication, staggered densities, PML factors).
 * med: Nz x Nx x 4, single or double (every real array follows its class): c^2, rho, dt / rho_sgz, dt / rho_sgx, z fastest (a host array or, in a GPU build,
 * a gpuArray).  pml: [az; azs; ax; axs], 2 Nz + 2 Nx values.  s: V x M x T' (pulse fastest: the kernel's order), the source table.  src: 3 x M host array, per
 * source [node; wz; wx] with node = j Nz + i (0-based) and wz = nz 2 c dt / h.  sen: N host values, the sensors' nodes (0-based).
 * prm = [Nz Nx V Nt dt_h inv_h order], order 2, 4 or 8 (optional, default 8).  rec: Nt x N x V of the class of med (time first, as ChannelData holds it).
 * The states are the gateway's own scratch, cleared on the device (QDAS_FDTD_ZERO); sources and sensors must sit on distinct nodes.  M = 0 (src empty) is
 * allowed: the record is then all zeros.
 * rec = qdas_mex('fdtdloss', med, pml, s, src, sen, prm, kap, loss) -- the same with absorption (qdas_fdtd_lossy).  kap: Nz x Nx of the class of med, the loss
 * map extended like the medium (2 c a under relaxation, 2 c a / dt under Stokes; qups_amd/fdtd.py `loss_model` is the recipe).  loss: host values
 * [mode g(1 .. L) E(1 .. L)], mode 1 = Stokes (L = 0) | 2 = relaxation (L = 1 .. 4).  The L memory variables per pulse are scratch of the call like the states.
 * rec = qdas_mex('fdtdnl', med, pml, s, src, sen, prm, bq, flags[, kap, loss]) -- the same with nonlinear propagation (qdas_fdtd_nonlinear).  bq: Nz x Nx of
 * the class of med, B/A / (2 rho) extended like the medium (qups_amd/fdtd.py `nl_model` is the recipe); flags: one host value, 0 | 1 (no convective term);
 * kap and loss as for 'fdtdloss', both or neither.  The source table is in m/s. */
static mxArray *cmd_fdtd(int nrhs, const mxArray *prhs[], int kind) {                                   /* kind 0: 'fdtd', 1: 'fdtdloss', 2: 'fdtdnl' */
    const int nonlin = kind == 2, lossy = kind == 1 || (nonlin && nrhs == 10), ki = nonlin ? 8 : 6;     /* ki: where kap sits; loss follows it */
    if (nonlin ? (nrhs != 8 && nrhs != 10) : nrhs != (lossy ? 8 : 6))
        mexErrMsgIdAndTxt("QUPS:das_spec:nargin", nonlin ? "qdas_mex('fdtdnl', med, pml, s, src, sen, prm, bq, flags[, kap, loss])" :
                          lossy ? "qdas_mex('fdtdloss', med, pml, s, src, sen, prm, kap, loss)" : "qdas_mex('fdtd', med, pml, s, src, sen, prm)");
    const mxClassID cls = mxGetClassID(prhs[0]);
    if ((cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS) || mxIsComplex(prhs[0])) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: med must be real single or double.");
    if (mxGetClassID(prhs[1]) != cls || mxGetClassID(prhs[2]) != cls || mxIsComplex(prhs[1]) || mxIsComplex(prhs[2]))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: pml and s must be real and of the class of med.");
    const size_t np = mxGetNumberOfElements(prhs[5]);
    const double zn = num_at(prhs[5], 0, "prm"), xn = num_at(prhs[5], 1, "prm"), vn = num_at(prhs[5], 2, "prm"), tn = num_at(prhs[5], 3, "prm");
    const double on = np > 6 ? num_at(prhs[5], 6, "prm") : 8.0;
    if (!(zn >= 1.0) || zn != floor(zn) || !(xn >= 1.0) || xn != floor(xn) || !(vn >= 0.0) || vn != floor(vn) || !(tn >= 0.0) || tn != floor(tn) ||
        on != floor(on) || zn * xn >= 2147483648.0 || vn > 65535.0 || tn >= 1e12 || !(fabs(on) < 1e6))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: prm = [Nz Nx V Nt dt_h inv_h order] with integers Nz, Nx >= 1, Nz Nx < 2^31, 0 <= V <= 65535, Nt >= 0.");
    qdas_fdtd_desc d;
    memset(&d, 0, sizeof d);
    d.Nz = (uint64_t)zn; d.Nx = (uint64_t)xn; d.V = (uint64_t)vn; d.Nt = (uint64_t)tn;
    d.dt_h = num_at(prhs[5], 4, "prm"); d.inv_h = num_at(prhs[5], 5, "prm");
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32; d.order = (int32_t)on; d.device = -1;
    d.flags = QDAS_FDTD_ZERO;                                                                       /* the states are scratch of this call: the entry clears them on the device */
    d.ld = d.Nz; d.vstride = d.Nz * d.Nx;
    const size_t cells = (size_t)(d.Nz * d.Nx), rs = cls == mxDOUBLE_CLASS ? 8 : 4;
    d.M = (uint64_t)(mxGetNumberOfElements(prhs[3]) / 3); d.N = (uint64_t)mxGetNumberOfElements(prhs[4]);
    if (mxGetNumberOfElements(prhs[3]) % 3) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: src is 3 x M: [node; wz; wx] per source.");
    if (mxGetNumberOfElements(prhs[0]) != 4 * cells) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: med holds %llu values, not Nz x Nx x 4.", (unsigned long long)mxGetNumberOfElements(prhs[0]));
    if (mxGetNumberOfElements(prhs[1]) != 2 * (size_t)(d.Nz + d.Nx)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: pml holds %llu values, not 2 Nz + 2 Nx.", (unsigned long long)mxGetNumberOfElements(prhs[1]));
    const uint64_t ns = (uint64_t)mxGetNumberOfElements(prhs[2]), MV = d.M * d.V;
    d.Ts = MV ? ns / MV : 0;
    if (MV ? ns % MV != 0 : ns != 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd: s holds %llu values, not V x M x T' with V = %llu, M = %llu.", (unsigned long long)ns, (unsigned long long)d.V, (unsigned long long)d.M);
    d.rec_st = 1; d.rec_sn = d.Nt; d.rec_sv = d.Nt * d.N;
    qdas_fdtd_loss q;
    memset(&q, 0, sizeof q);
    if (lossy) {
        if (mxGetClassID(prhs[ki]) != cls || mxIsComplex(prhs[ki]) || mxGetNumberOfElements(prhs[ki]) != cells)
            mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtdloss: kap must be Nz x Nx, real and of the class of med.");
        const size_t nl = mxGetNumberOfElements(prhs[ki + 1]);
        if (nl < 1 || nl % 2 != 1 || nl > 1 + 2 * QDAS_FDTD_MAX_L) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtdloss: loss = [mode g(1 .. L) E(1 .. L)] with L <= 4.");
        const double mn = num_at(prhs[ki + 1], 0, "loss");
        q.mode = (mn == floor(mn) && fabs(mn) < 1e6) ? (int32_t)mn : -1;
        q.L = (int32_t)(nl / 2);
        for (int k = 0; k < q.L; ++k) { q.g[k] = num_at(prhs[ki + 1], (mwSize)(1 + k), "loss"); q.E[k] = num_at(prhs[ki + 1], (mwSize)(1 + q.L + k), "loss"); }
    }
    qdas_fdtd_nl w;
    memset(&w, 0, sizeof w);
    if (nonlin) {
        if (mxGetClassID(prhs[6]) != cls || mxIsComplex(prhs[6]) || mxGetNumberOfElements(prhs[6]) != cells)
            mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtdnl: bq must be Nz x Nx, real and of the class of med.");
        if (mxGetNumberOfElements(prhs[7]) != 1) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtdnl: flags is one value, 0 or 1 (no convective term).");
        const double fn = num_at(prhs[7], 0, "flags");
        w.flags = (fn == floor(fn) && fabs(fn) < 1e6) ? (int32_t)fn : -1;
    }
    const mwSize dims[3] = {(mwSize)d.Nt, (mwSize)d.N, (mwSize)d.V};
    if (d.Nt * d.V == 0 || d.N == 0) {
        const uint64_t keep = d.Nt;
        if (d.N == 0) d.Nt = 0;                                                                       /* no sensors: nothing to run, but the call is still validated */
        const int rc = nonlin ? qdas_fdtd_nonlinear(&d, NULL, lossy ? &q : NULL, &w) : lossy ? qdas_fdtd_lossy(&d, NULL, &q) : (d.N == 0 ? QDAS_OK : qdas_fdtd(&d, NULL));
        d.Nt = keep;
        if (rc) CFAIL("%s", qdas_last_error());
        release_devargs();
        return mxCreateNumericArray(3, dims, cls, mxREAL);
    }
    /* the host side: node lists, per-tile lists and the weights, in one integer and one real block */
    const uint64_t nt = qdas_fdtd_tiles(d.Nz, d.Nx);
    const size_t ni = (size_t)(2 * d.M + 2 * d.N + 2 * (nt + 1)), nr = (size_t)(2 * d.M);
    if (d.M) (void)num_at(prhs[3], 0, "src");
    (void)num_at(prhs[4], 0, "sen");                   /* whatever raises does so before the host blocks exist */
    int32_t *hi = (int32_t *)calloc(ni ? ni : 1, sizeof(int32_t));
    void *hr = calloc(nr ? nr : 1, rs);
    if (!hi || !hr) { free(hi); free(hr); CFAIL("fdtd: out of memory."); }
    int32_t *src_node = hi, *src_start = src_node + d.M, *src_list = src_start + nt + 1, *sen_node = src_list + d.M, *sen_start = sen_node + d.N, *sen_list = sen_start + nt + 1;
    int bad = 0;
    for (uint64_t m = 0; m < d.M; ++m) {
        const double nd = num_at(prhs[3], (mwSize)(3 * m), "src");
        if (!(nd >= 0.0) || nd != floor(nd) || nd >= (double)cells) bad = 1; else src_node[m] = (int32_t)nd;
        for (int r = 0; r < 2; ++r) {
            const double w = num_at(prhs[3], (mwSize)(3 * m + 1 + (uint64_t)r), "src");
            if (rs == 8) ((double *)hr)[(size_t)r * d.M + m] = w; else ((float *)hr)[(size_t)r * d.M + m] = (float)w;
        }
    }
    for (uint64_t j = 0; j < d.N; ++j) {
        const double nd = num_at(prhs[4], (mwSize)j, "sen");
        if (!(nd >= 0.0) || nd != floor(nd) || nd >= (double)cells) bad = 1; else sen_node[j] = (int32_t)nd;
    }
    if (bad || qdas_fdtd_tile_lists(d.Nz, d.Nx, d.M, src_node, src_start, src_list) || qdas_fdtd_tile_lists(d.Nz, d.Nx, d.N, sen_node, sen_start, sen_list)) {
        free(hi); free(hr);
        CFAIL("fdtd: the nodes of src and sen are integers in [0, Nz Nx).");
    }
    const size_t sbytes = (size_t)(5 + q.L) * cells * (size_t)d.V * rs;                                 /* the five states, then the V L memory variables */
    char *di = (char *)dev_extra(ni * sizeof(int32_t)), *dr = (char *)dev_extra((nr ? nr : 1) * rs), *ds = (char *)dev_extra(sbytes);
    int rc = qdas_device_copy(di, hi, ni * sizeof(int32_t), 0, -1);
    if (!rc && nr) rc = qdas_device_copy(dr, hr, nr * rs, 0, -1);
    free(hi); free(hr);
    if (rc) CFAIL("%s", qdas_last_error());
    int dev = 0;
    const char *med = (const char *)dev_in(prhs[0], 4 * cells * rs, "med", &dev), *pml = (const char *)dev_in(prhs[1], 2 * (size_t)(d.Nz + d.Nx) * rs, "pml", &dev);
    const void *sp = dev_in(prhs[2], (size_t)ns * rs, "s", &dev);
    qdas_fdtd_args a;
    memset(&a, 0, sizeof a);
    const size_t sb = cells * (size_t)d.V * rs;
    a.p = ds; a.uz = ds + sb; a.ux = ds + 2 * sb; a.rz = ds + 3 * sb; a.rx = ds + 4 * sb;
    a.c2 = med; a.rho = med + cells * rs; a.dtrz = med + 2 * cells * rs; a.dtrx = med + 3 * cells * rs;
    a.az = pml; a.azs = pml + d.Nz * rs; a.ax = pml + 2 * d.Nz * rs; a.axs = pml + (2 * d.Nz + d.Nx) * rs;
    a.s = sp; a.src_wz = dr; a.src_wx = dr + d.M * rs;
    const int32_t *dii = (const int32_t *)di;
    a.src_node = dii; a.src_start = dii + d.M; a.src_list = a.src_start + nt + 1; a.sen_node = a.src_list + d.M; a.sen_start = a.sen_node + d.N; a.sen_list = a.sen_start + nt + 1;
    const size_t bytes = (size_t)(d.Nt * d.N * d.V) * rs;
    mxArray *host;
    if (lossy) {
        q.kap = dev_in(prhs[ki], cells * rs, "kap", &dev);
        q.e = q.L ? ds + 5 * sb : NULL;
    }
    if (nonlin) w.bq = dev_in(prhs[6], cells * rs, "bq", &dev);
    a.rec = dev_out(3, dims, cls, 0, dev, bytes, &host);
    return finish(nonlin ? qdas_fdtd_nonlinear(&d, &a, lossy ? &q : NULL, &w) : lossy ? qdas_fdtd_lossy(&d, &a, &q) : qdas_fdtd(&d, &a), host, bytes);
}

/* rec = qdas_mex('fdtd3', med, pml, s, src, sen, prm) -- Nt steps of the 3-D acoustic FDTD scheme (qdas_fdtd3, include/qdas.h) from rest, on tables the caller
 * prepared (qups_amd/fdtd3.py `prepare` is the recipe).  The 'fdtd' command with a third axis:
 * med: Nz x Nx x Ny x 5, single or double (every real array follows its class): c^2, rho, dt / rho_sgz, dt / rho_sgx, dt / rho_sgy, z fastest, then x, then y
 * (a host array or, in a GPU build, a gpuArray).  pml: [az; azs; ax; axs; ay; ays], 2 Nz + 2 Nx + 2 Ny values.  s: V x M x T' (pulse fastest), the source
 * table.  src: 4 x M host array, per source [node; wz; wx; wy] with node = (k Nx + j) Nz + i (0-based) and wz = nz 2 c dt / h.  sen: N host values, the
 * sensors' nodes (0-based).  prm = [Nz Nx Ny V Nt dt_h inv_h order], order 2, 4 or 8 (optional, default 8).  rec: Nt x N x V of the class of med.
 * The states are the gateway's own scratch, cleared on the device (QDAS_FDTD3_ZERO: the gateway has no device fill); sources and sensors must sit on distinct
 * nodes.  M = 0 (src empty) is allowed: the record is then all zeros. */
static mxArray *cmd_fdtd3(int nrhs, const mxArray *prhs[]) {
    if (nrhs != 6) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('fdtd3', med, pml, s, src, sen, prm)");
    const mxClassID cls = mxGetClassID(prhs[0]);
    if ((cls != mxDOUBLE_CLASS && cls != mxSINGLE_CLASS) || mxIsComplex(prhs[0])) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: med must be real single or double.");
    if (mxGetClassID(prhs[1]) != cls || mxGetClassID(prhs[2]) != cls || mxIsComplex(prhs[1]) || mxIsComplex(prhs[2]))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: pml and s must be real and of the class of med.");
    const size_t np = mxGetNumberOfElements(prhs[5]);
    const double zn = num_at(prhs[5], 0, "prm"), xn = num_at(prhs[5], 1, "prm"), yn = num_at(prhs[5], 2, "prm"), vn = num_at(prhs[5], 3, "prm"), tn = num_at(prhs[5], 4, "prm");
    const double on = np > 7 ? num_at(prhs[5], 7, "prm") : 8.0;
    if (!(zn >= 1.0) || zn != floor(zn) || !(xn >= 1.0) || xn != floor(xn) || !(yn >= 1.0) || yn != floor(yn) || !(vn >= 0.0) || vn != floor(vn) || !(tn >= 0.0) ||
        tn != floor(tn) || on != floor(on) || zn * xn * yn >= 2147483648.0 || vn > 65535.0 || tn >= 1e12 || !(fabs(on) < 1e6))
        mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: prm = [Nz Nx Ny V Nt dt_h inv_h order] with integers Nz, Nx, Ny >= 1, Nz Nx Ny < 2^31, 0 <= V <= 65535, Nt >= 0.");
    qdas_fdtd3_desc d;
    memset(&d, 0, sizeof d);
    d.Nz = (uint64_t)zn; d.Nx = (uint64_t)xn; d.Ny = (uint64_t)yn; d.V = (uint64_t)vn; d.Nt = (uint64_t)tn;
    d.dt_h = num_at(prhs[5], 5, "prm"); d.inv_h = num_at(prhs[5], 6, "prm");
    d.dtype = cls == mxDOUBLE_CLASS ? QDAS_F64 : QDAS_F32; d.order = (int32_t)on; d.device = -1;
    d.flags = QDAS_FDTD3_ZERO;                                                                      /* the states are scratch of this call: the entry clears them on the device */
    d.ld = d.Nz; d.pstride = d.Nz * d.Nx; d.vstride = d.pstride * d.Ny;
    const size_t cells = (size_t)d.vstride, npml = 2 * (size_t)(d.Nz + d.Nx + d.Ny), rs = cls == mxDOUBLE_CLASS ? 8 : 4;
    d.M = (uint64_t)(mxGetNumberOfElements(prhs[3]) / 4); d.N = (uint64_t)mxGetNumberOfElements(prhs[4]);
    if (mxGetNumberOfElements(prhs[3]) % 4) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: src is 4 x M: [node; wz; wx; wy] per source.");
    if (mxGetNumberOfElements(prhs[0]) != 5 * cells) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: med holds %llu values, not Nz x Nx x Ny x 5.", (unsigned long long)mxGetNumberOfElements(prhs[0]));
    if (mxGetNumberOfElements(prhs[1]) != npml) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: pml holds %llu values, not 2 Nz + 2 Nx + 2 Ny.", (unsigned long long)mxGetNumberOfElements(prhs[1]));
    const uint64_t ns = (uint64_t)mxGetNumberOfElements(prhs[2]), MV = d.M * d.V;
    d.Ts = MV ? ns / MV : 0;
    if (MV ? ns % MV != 0 : ns != 0) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "fdtd3: s holds %llu values, not V x M x T' with V = %llu, M = %llu.", (unsigned long long)ns, (unsigned long long)d.V, (unsigned long long)d.M);
    d.rec_st = 1; d.rec_sn = d.Nt; d.rec_sv = d.Nt * d.N;
    const mwSize dims[3] = {(mwSize)d.Nt, (mwSize)d.N, (mwSize)d.V};
    if (d.Nt * d.V == 0 || d.N == 0) {
        const int rc = d.N == 0 ? QDAS_OK : qdas_fdtd3(&d, NULL);                                     /* (an empty call is still validated) */
        if (rc) CFAIL("%s", qdas_last_error());
        release_devargs();
        return mxCreateNumericArray(3, dims, cls, mxREAL);
    }
    /* the host side: node lists, per-brick lists and the weights, in one integer and one real block */
    const uint64_t nb = qdas_fdtd3_bricks(d.Nz, d.Nx, d.Ny);
    const size_t ni = (size_t)(2 * d.M + 2 * d.N + 2 * (nb + 1)), nr = (size_t)(3 * d.M);
    if (d.M) (void)num_at(prhs[3], 0, "src");
    (void)num_at(prhs[4], 0, "sen");                   /* whatever raises does so before the host blocks exist */
    int32_t *hi = (int32_t *)calloc(ni ? ni : 1, sizeof(int32_t));
    void *hr = calloc(nr ? nr : 1, rs);
    if (!hi || !hr) { free(hi); free(hr); CFAIL("fdtd3: out of memory."); }
    int32_t *src_node = hi, *src_start = src_node + d.M, *src_list = src_start + nb + 1, *sen_node = src_list + d.M, *sen_start = sen_node + d.N, *sen_list = sen_start + nb + 1;
    int bad = 0;
    for (uint64_t m = 0; m < d.M; ++m) {
        const double nd = num_at(prhs[3], (mwSize)(4 * m), "src");
        if (!(nd >= 0.0) || nd != floor(nd) || nd >= (double)cells) bad = 1; else src_node[m] = (int32_t)nd;
        for (int r = 0; r < 3; ++r) {
            const double w = num_at(prhs[3], (mwSize)(4 * m + 1 + (uint64_t)r), "src");
            if (rs == 8) ((double *)hr)[(size_t)r * d.M + m] = w; else ((float *)hr)[(size_t)r * d.M + m] = (float)w;
        }
    }
    for (uint64_t j = 0; j < d.N; ++j) {
        const double nd = num_at(prhs[4], (mwSize)j, "sen");
        if (!(nd >= 0.0) || nd != floor(nd) || nd >= (double)cells) bad = 1; else sen_node[j] = (int32_t)nd;
    }
    if (bad || qdas_fdtd3_brick_lists(d.Nz, d.Nx, d.Ny, d.M, src_node, src_start, src_list) || qdas_fdtd3_brick_lists(d.Nz, d.Nx, d.Ny, d.N, sen_node, sen_start, sen_list)) {
        free(hi); free(hr);
        CFAIL("fdtd3: the nodes of src and sen are integers in [0, Nz Nx Ny).");
    }
    const size_t sb = cells * (size_t)d.V * rs;
    char *di = (char *)dev_extra(ni * sizeof(int32_t)), *dr = (char *)dev_extra((nr ? nr : 1) * rs), *ds = (char *)dev_extra(7 * sb);
    int rc = qdas_device_copy(di, hi, ni * sizeof(int32_t), 0, -1);
    if (!rc && nr) rc = qdas_device_copy(dr, hr, nr * rs, 0, -1);
    free(hi); free(hr);
    if (rc) CFAIL("%s", qdas_last_error());
    int dev = 0;
    const char *med = (const char *)dev_in(prhs[0], 5 * cells * rs, "med", &dev), *pml = (const char *)dev_in(prhs[1], npml * rs, "pml", &dev);
    const void *sp = dev_in(prhs[2], (size_t)ns * rs, "s", &dev);
    qdas_fdtd3_args a;
    memset(&a, 0, sizeof a);
    a.p = ds; a.uz = ds + sb; a.ux = ds + 2 * sb; a.uy = ds + 3 * sb; a.rz = ds + 4 * sb; a.rx = ds + 5 * sb; a.ry = ds + 6 * sb;
    a.c2 = med; a.rho = med + cells * rs; a.dtrz = med + 2 * cells * rs; a.dtrx = med + 3 * cells * rs; a.dtry = med + 4 * cells * rs;
    a.az = pml; a.azs = pml + d.Nz * rs; a.ax = pml + 2 * d.Nz * rs; a.axs = pml + (2 * d.Nz + d.Nx) * rs;
    a.ay = pml + 2 * (d.Nz + d.Nx) * rs; a.ays = pml + (2 * (d.Nz + d.Nx) + d.Ny) * rs;
    a.s = sp; a.src_wz = dr; a.src_wx = dr + d.M * rs; a.src_wy = dr + 2 * d.M * rs;
    const int32_t *dii = (const int32_t *)di;
    a.src_node = dii; a.src_start = dii + d.M; a.src_list = a.src_start + nb + 1; a.sen_node = a.src_list + d.M; a.sen_start = a.sen_node + d.N; a.sen_list = a.sen_start + nb + 1;
    const size_t bytes = (size_t)(d.Nt * d.N * d.V) * rs;
    mxArray *host;
    a.rec = dev_out(3, dims, cls, 0, dev, bytes, &host);
    return finish(qdas_fdtd3(&d, &a), host, bytes);
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
#ifdef QDAS_MEX_GPU
    mxInitGPU();
#endif
    char cmd[32] = "";
    if (nrhs >= 1 && mxIsChar(prhs[0]) && mxGetString(prhs[0], cmd, sizeof cmd)) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "unreadable command.");
    if (nlhs > (!strcmp(cmd, "wbilerp") ? 3 : (!strcmp(cmd, "pcf") || !strcmp(cmd, "rayintegrals") || !strcmp(cmd, "raybackproject")) ? 2 : 1))
        mexErrMsgIdAndTxt("QUPS:das_spec:nargout", "qdas_mex returns at most one output ('pcf', 'rayintegrals', 'raybackproject': two; 'wbilerp': three).");
    if (nrhs >= 1 && mxIsChar(prhs[0])) {
        if (!strcmp(cmd, "create")) {
            const int slot = create_plan(nrhs - 1, prhs + 1);
            plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
            *(uint64_t *)mxGetData(plhs[0]) = (uint64_t)(slot + 1);
        } else if (!strcmp(cmd, "execute")) {
            if (nrhs != 3) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('execute', h, x)");
            const char *err = execute_plan(slot_of(prhs[1]), prhs[2], 0, &plhs[0]);
            if (err) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s", err);
        } else if (!strcmp(cmd, "prepare")) {
            if (nrhs != 3) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('prepare', h, F)");
            plan_slot *s = slot_of(prhs[1]);
            if (s->plan && qdas_plan_prepare_frames(s->plan, (uint64_t)num_at(prhs[2], 0, "F"))) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s", qdas_last_error());
        } else if (!strcmp(cmd, "info")) {
            if (nrhs != 2) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex('info', h)");
            plan_slot *s = slot_of(prhs[1]);
            char buf[512];
            if (s->plan) {
                char kn[256];
                qdas_plan_kernel_name(s->plan, kn, sizeof kn);
                snprintf(buf, sizeof buf, "%s; reciprocal=%d", kn, qdas_plan_reciprocal(s->plan));
            } else {
                int n = 0;
                qdas_plan_sharded_info(s->splan, -1, &n, NULL, NULL, NULL);
                snprintf(buf, sizeof buf, "sharded over %d device slab(s)", n);
            }
            plhs[0] = mxCreateString(buf);
        } else if (!strcmp(cmd, "delays")) { plhs[0] = cmd_delays(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "lut")) { plhs[0] = cmd_lut(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "wsinterpd")) { plhs[0] = cmd_wsinterpd(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "shiftsum")) { plhs[0] = cmd_shiftsum(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "greens")) { plhs[0] = cmd_greens(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "convd")) { plhs[0] = cmd_convd(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "hilbert")) { plhs[0] = cmd_hilbert(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "slsc") || !strcmp(cmd, "dmas") || !strcmp(cmd, "cohfac") || !strcmp(cmd, "pcf")) { cmd_coherence(cmd, nlhs, plhs, nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "pwznxcorr")) { plhs[0] = cmd_pwznxcorr(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "msfm")) { plhs[0] = cmd_msfm(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "msfm3d")) { plhs[0] = cmd_msfm3d(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "adjoint")) { plhs[0] = cmd_adjoint(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "migration")) { plhs[0] = cmd_migration(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "refocus")) { plhs[0] = cmd_refocus(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "wbilerp")) { cmd_wbilerp(nlhs, plhs, nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "rayintegrals")) { cmd_rayintegrals(nlhs, plhs, nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "raybackproject")) { cmd_raybackproject(nlhs, plhs, nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "scanconvert")) { plhs[0] = cmd_scanconvert(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "demod")) { plhs[0] = cmd_demod(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "resample")) { plhs[0] = cmd_resample(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "fdtd")) { plhs[0] = cmd_fdtd(nrhs - 1, prhs + 1, 0);
        } else if (!strcmp(cmd, "fdtdloss")) { plhs[0] = cmd_fdtd(nrhs - 1, prhs + 1, 1);
        } else if (!strcmp(cmd, "fdtdnl")) { plhs[0] = cmd_fdtd(nrhs - 1, prhs + 1, 2);
        } else if (!strcmp(cmd, "fdtd3")) { plhs[0] = cmd_fdtd3(nrhs - 1, prhs + 1);
        } else if (!strcmp(cmd, "destroy")) {
            if (nrhs >= 2) destroy_slot(slot_of(prhs[1])); else destroy_all();
        } else mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "unknown command '%s'.", cmd);
        return;
    }
    /* one call: create + execute + destroy */
    if (nrhs != 10) mexErrMsgIdAndTxt("QUPS:das_spec:nargin", "qdas_mex expects 10 inputs (or a command string first).");
    qdas_sizes z;
    uint64_t F = 1;
    read_sizes(prhs[0], &z, &F);
    const mxArray *cargs[9] = {prhs[0], prhs[1], prhs[2], prhs[3], prhs[4], prhs[5], prhs[6], prhs[7], prhs[9]};
    const int slot = create_plan(9, cargs);
    const char *err = execute_plan(&g_slots[slot], prhs[8], F, &plhs[0]);
    destroy_slot(&g_slots[slot]);
    if (err) mexErrMsgIdAndTxt("QUPS:das_spec:qdas", "%s", err);
}
