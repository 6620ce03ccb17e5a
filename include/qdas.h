/* qdas.h -- C ABI of libqdas.so: MI355X-native delay-and-sum beamforming engine.
 *
 * Drop-in boundary for ONE reference call site: the device launch inside
 * `das_spec` (reference kern/das_spec.m:279-306 builds the kernel object and
 * uploads the size constants; kern/das_spec.m:372 is the per-frame launch
 *
 *     y{f} = k.feval(yg, Pi, Pr, Pv, Nv, apod, cinv, [cstride, astride],
 *                    x(:,:,:,f), [fs, fmod]);
 *
 * of `DAS` / `DASf` / `DASh`, reference src/bf.cu:144-172), plus the `delays`
 * variant (kern/das_spec.m:377, src/bf.cu:209-298) and -- as the "next" row --
 * the split-delay launch of `wsinterpd2[f|h]` (kern/wsinterpd2.m:236,
 * src/interpd.cu:449-476) used by bfDAS/bfDASLUT.  The steps either side of
 * the path have their own entry points further down: `qdas_greens`
 * (src/greens.cu), `qdas_shift_sum` (UltrasoundSystem.focusTx), `qdas_pre_*` (ChannelData.hilbert / downmix), `qdas_convd`
 * (src/convd.cu), and `qdas_permute3` for row-major hosts.
 *
 * Everything is plain C: pointers, sizes, no torch / HIP types in signatures
 * (`stream` is a `hipStream_t` passed as `void*`; NULL = the default stream).
 * All arrays use MATLAB (column-major) memory order exactly as the reference
 * kernel ABI does.  Functions return 0 on success, a QDAS_E* code otherwise;
 * `qdas_last_error()` returns a thread-local message (the MEX shim maps it to
 * mexErrMsgIdAndTxt("QUPS:das_spec:...")).  The library never frees or keeps
 * caller memory beyond a call, except device copies it makes itself.
 */
#ifndef QDAS_H
#define QDAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100: rounds 1-3.  101 (round 5): qdas_wsinterpd_desc carries ystride[8] / lane_dim / reserved (added in round 4 without a bump), QDAS_PLAN_PREFOLDED rejects
 * apodization arrays.  102 (round 5): the device staging entries recycle their buffers (qdas_device_trim), one-shot entries take temporaries from kept arenas.
 * 103 (round 6): qdas_device_free waits for the device before a buffer can be handed out again (it used to be caller's business, unstated).  EVERY descriptor of this header must be ZERO-INITIALISED by the caller (memset / `= {0}`) before its fields are set: fields added by
 * later versions then read as "default", and a caller compiled against an older header must check qdas_version() against the QDAS_VERSION it was built with. */
#define QDAS_VERSION 103

/* ---- data precision: the reference's kernel postfix (kern/das_spec.m:218-222) */
#define QDAS_F64 0 /* 'DAS'  : double2 data/apod/y, double geometry + time            */
#define QDAS_F32 1 /* 'DASf' : float2  data/apod/y, float  geometry + time            */
#define QDAS_F16 2 /* 'DASh' : half2   data/apod/y (passed as ushort2), float geometry */

/* ---- QUPS_BF_FLAG bit layout (reference kern/das_spec.m:198-213, src/bf.cu:100,126,129) */
#define QDAS_INTERP_NEAREST  0
#define QDAS_INTERP_LINEAR   1
#define QDAS_INTERP_CUBIC    2 /* Catmull-Rom = MATLAB interp1 'cubic' (the CPU path)   */
#define QDAS_INTERP_LANCZOS3 3 /* window a = 2, 4 taps (src/interpd.cu:116-150)          */
#define QDAS_INTERP_LINEAR4  4 /* alias of linear (src/interpd.cu:163)                   */
#define QDAS_INTERP_CUBIC_DEV 5 /* extension: the Horner lines the CUDA/OpenCL code executes
                                   (src/interpd.cu:103-106) -- NOT Catmull-Rom; see DESIGN.md */
#define QDAS_FLAG_INTERP_MASK 7
#define QDAS_FLAG_KEEP_RX 8   /* 'SYN' | 'BF' : keep the receive dimension   */
#define QDAS_FLAG_KEEP_TX 16  /* 'MUL' | 'BF' : keep the transmit dimension  */
#define QDAS_FLAG_TPOSE   32  /* data is T x M x N instead of T x N x M      */

/* ---- where caller pointers live */
#define QDAS_MEM_HOST   0
#define QDAS_MEM_DEVICE 1

/* ---- kernel selection (QDAS_KERNEL_AUTO picks the tiled kernel when eligible)
 * Eligible: 'DAS' with any data precision -- fp64 data: pixel-independent apodization and / or one pixel x receiver (pixel-only) array, scalar sound speed --,
 * 'SYN' / 'MUL' / 'BF' with fp32 data; scalar sound speed or a full per-pixel map; any number of pixel-independent apodization arrays
 * (folded into an N x M table) plus pixel-dependent arrays of ONE side: I x N (pixel x receiver), or I x 1 x M (pixel x transmit: 'DAS' / 'MUL';
 * the roles of the two apertures are swapped), with any I-only arrays (spatial weights / region-of-interest masks) -- several of them, or arrays
 * that broadcast over a pixel dimension (I1 x 1 x 1 x N), are multiplied into one plan-owned array at plan creation --, or one generated receive
 * rule (rx_apod_kind); fp32 data with real weights and no remodulation also takes a transmit-side AND a receive-side pixel array together
 * (the receive-side product is applied per pair);
 * N and M up to about 1000 each.  Everything else runs the generic kernel with identical semantics; qdas_last_error() after a
 * QDAS_KERNEL_TILED request says why a plan is not eligible. */
#define QDAS_KERNEL_AUTO    0
#define QDAS_KERNEL_GENERIC 1 /* one pixel per lane, any mode / broadcast shape        */
#define QDAS_KERNEL_TILED   2 /* LDS-staged pixel tiles; error if the case is ineligible */

/* ---- generated receive apodization w(pixel, receiver), r = Pi - Pr(n), nhat = element normal:
 *  ACCEPTANCE     (reference src/UltrasoundSystem.m:5355-5373 apAcceptanceAngle): w = [ r.nhat/|r| >= p[0] ],  p[0] = cosd(theta)
 *  COSINE         (:5414-5428 apCosineAngle): w = cos(min(pi/2, p[0]*acos(clip(r.nhat/|r|, -1, 1)))),        p[0] = 90/theta
 *  FNUMBER_PLANAR (:5251-5256 apApertureGrowth, planar array): d = x_n - x_i, z = z_i: w = [z > p[0]*|2d|]*[|2d| < p[1]],  p = {f, Dmax}
 *  FNUMBER_ORIENTED (:5244-5250,5255-5256, non-planar array, elements rotated about y): d = r_x*n_z - r_z*n_x, z = |r_x*n_x + r_z*n_z| */
#define QDAS_RXAPOD_NONE             0
#define QDAS_RXAPOD_ACCEPTANCE       1
#define QDAS_RXAPOD_COSINE           2
#define QDAS_RXAPOD_FNUMBER_PLANAR   3
#define QDAS_RXAPOD_FNUMBER_ORIENTED 4

/* ---- plan flags (qdas_desc.plan_flags) */
#define QDAS_PLAN_NO_RECIPROCAL 1 /* never use the reciprocal mode of the tiled kernel (transmit elements == receive elements):
                                     the general kernel that every apodized / non-FSA acquisition runs                        */
#define QDAS_PLAN_JIT           2 /* compile the tiled kernel for THIS plan's sizes with hiprtc: N, M, T, strides, delay kinds,
                                     tile shape and modes become constants, the reference's const-compile specialisation
                                     (src/UltrasoundSystem.m:5626-5748 getDASConstCudaDef, src/sizes.cu:17-52).  Cached on disk
                                     (QDAS_CACHE_DIR, default ~/.cache/qdas); falls back to the prebuilt kernel with a message
                                     in qdas_last_error() if hiprtc is unavailable                                            */

#define QDAS_PLAN_COPY_INPUTS   4 /* desc.mem == QDAS_MEM_DEVICE: copy Pi, Pr, Pv, Nv, apod, cinv, rx_normals into plan-owned device
                                     buffers instead of reading the caller's arrays in place.  For hosts whose arrays do not
                                     outlive the call that created the plan (the MEX gateway's persistent handles: MATLAB frees
                                     the gpuArrays of das_spec's workspace when it returns)                                  */

#define QDAS_PLAN_NO_MIRROR     8 /* never use the lateral-mirror mode of the tiled kernel (scan, array and sequence mirror-symmetric
                                     about x = 0, detected from the geometry: tap index and weights are shared by a pixel and its
                                     mirror image)                                                                            */

#define QDAS_PLAN_MIRROR_SLAB   16 /* a pixel slab AND its mirror image in one plan (multi-GPU jobs that keep the lateral-mirror mode):
                                     i_begin / i_count describe slab A -- whole columns [c0, c1) of the FIRST half of an even number of
                                     columns I2 (I3 == 1) --; the plan also beamforms the mirror-image columns [I2 - c1, I2 - c0) and
                                     writes them behind slab A: y[0 .. i_count) = slab A, y[i_count .. 2 i_count) = slab B, both in
                                     natural pixel order ('DAS' only; y holds 2 i_count pixels).  QDAS_EUNSUPPORTED when the geometry
                                     is not mirror-symmetric or the mode is not available for the problem: use plain slabs then.  */

#define QDAS_PLAN_NO_FOLD       32 /* reciprocal plans with fp32 data: do NOT fold the frame (qdas_plan_folded) -- gather both traces of every
                                     unordered pair per pixel and share only tap index and weights between them, as rounds 1-3 did.  The fold
                                     costs a plan-owned copy of the frame (T x N x M complex64) and one streaming pass per frame            */

#define QDAS_PLAN_APPROX_SYMMETRY 64 /* take the reciprocal / lateral-mirror modes also when the geometry is symmetric only WITHIN A TOLERANCE: element and
                                     pixel POSITIONS may deviate from their partners' (mirror) images as long as the bound on the delay error this commits,
                                     cinv fs (2 max|M(p') - p| + max|M(r') - r| + max|M(v') - v|) resp. 2 cinv fs max|r_m - v_m|, stays <= 1e-5 sample
                                     (QDAS_SYM_TOL=<samples> overrides; normals and start times must match exactly).  Off by default: the modes then need
                                     bit-exact symmetry.  1e-5 sample is 0.8 nm of path at 20 MHz / 1540 m/s -- sub-ulp deviations of coordinates of a
                                     few mm; a delay error d sample shows up as a relative image error of about 2 pi (fc / fs) d: the image tolerance
                                     of 1e-4 allows ~6e-5 sample, i.e. ~5 nm, NOT micrometres -- a calibrated probe is simply not symmetric.
                                     qdas_plan_symmetry_bound reports the bounds of the modes in use                                          */

#define QDAS_PLAN_PREFOLDED     128 /* the frames handed to execute ARE folded frames (qdas_fold: complex64, upper triangle n <= m; weights applied there): the plan
                                     runs no fold pass and owns no folded copy.  For hosts that fold once per acquisition and replicate the folded frame (half
                                     the bytes) to several devices.  Needs a reciprocal fp32 'DAS' problem without apodization arrays whose tiles all fit the
                                     staging windows, else QDAS_EUNSUPPORTED                                                                       */

/* ---- LIFETIME of caller memory.  Host arrays (QDAS_MEM_HOST) are copied at qdas_plan_create and never touched again.  Device
 *      arrays (QDAS_MEM_DEVICE) are used IN PLACE: Pi, Pr, Pv, Nv, apod, cinv and rx_normals must stay allocated and unchanged
 *      until qdas_plan_destroy -- unless the plan was created with QDAS_PLAN_COPY_INPUTS.  acstride is read at creation only.
 *      x / y belong to the caller and are only accessed by the execute call they are passed to (asynchronously on `stream` for
 *      device memory: keep them alive until the stream has passed the call).  Every entry restores the calling thread's
 *      current HIP device before it returns. */

/* ---- error codes */
#define QDAS_OK            0
#define QDAS_EINVAL        1 /* bad argument / inconsistent sizes (message says which)  */
#define QDAS_EUNSUPPORTED  2 /* valid request the build cannot serve                    */
#define QDAS_EHIP          3 /* HIP runtime error (message carries hipGetErrorString)   */
#define QDAS_ENOMEM        4
#define QDAS_ENOCONV       5 /* an iteration reached its pass cap without a fixed point  */
#define QDAS_ENOTLDS       6 /* qdas_migration, qdas_refocus: a transform length the in-LDS kernels do not take (the caller composes the result instead) */

/* Size/flag constants: the reference's constant-memory symbols QUPS_{T,N,M,I,I1,I2,I3,S},
 * QUPS_{VS,DV}, QUPS_BF_FLAG (reference src/sizes.cu:17-52, src/bf.cu:45-47;
 * uploaded at kern/das_spec.m:294-298). */
typedef struct qdas_sizes {
    uint64_t T;          /* fast-time samples per trace                                  */
    uint64_t N, M;       /* receivers, transmits                                         */
    uint64_t I1, I2, I3; /* image size; I = I1*I2*I3, I1 fastest                         */
    uint64_t S;          /* number of apodization arrays (0 = none; reference passes {1}) */
    int32_t  flag;       /* QUPS_BF_FLAG                                                  */
    int32_t  VS;         /* 1: virtual-source model, 0: plane-wave model                  */
    int32_t  DV;         /* 1: diverging wave (distance always positive)                  */
    int32_t  dtype;      /* QDAS_F64 | QDAS_F32 | QDAS_F16                                */
} qdas_sizes;

/* Full description of one beamforming problem (everything except the data). */
typedef struct qdas_desc {
    qdas_sizes sz;
    double fs, fmod;      /* [fs, fmod] == tvars (src/bf.cu:57-58)                        */
    /* geometry, real(prec) -- float for QDAS_F16 (kern/das_spec.m:356) */
    const void *Pi;       /* 3 x I    pixel positions                                      */
    const void *Pr;       /* 3 x N    receiver positions                                   */
    const void *Pv;       /* 4 x M    (virtual) source positions, row 4 = t0 (das_spec.m:361) */
    const void *Nv;       /* 3 x M    transmit normals                                     */
    const void *apod;     /* concatenated apodization arrays (das_spec.m:344-345); complex(prec)
                             unless apod_real != 0; may be NULL iff S == 0                 */
    const void *cinv;     /* 1/c, real(prec), broadcastable I1 x I2 x I3 x N x M           */
    const uint64_t *acstride; /* HOST pointer, 6*(1+S) entries: [cstride(6), astride(6 x S)]
                             element strides for dims (I1,I2,I3,N,M) -- 0 where singleton -- and
                             the array's base offset in entry 6 (reference das_spec.m:257-260) */
    int32_t mem;          /* QDAS_MEM_*: where Pi..cinv AND x / y of execute() live        */
    int32_t apod_real;    /* extension: apod buffer holds real(prec) weights               */
    int32_t kernel;       /* QDAS_KERNEL_*                                                 */
    int32_t device;       /* HIP device ordinal, -1 = current device                       */
    /* pixel shard (multi-GPU: every rank builds the same desc with its own slab;
       single GPU: i_begin = 0, i_count = 0 meaning "all I") */
    uint64_t i_begin;     /* first linear pixel index of this plan                         */
    uint64_t i_count;     /* number of pixels (0 = I - i_begin)                            */
    uint64_t y_ld;        /* pixels between consecutive [n|m] planes of y (0 = i_count): lets a
                             shard write straight into a full-size I x [N] x [M] buffer    */
    /* extension: receive apodization GENERATED in the kernel from the geometry instead of a
       materialised I1 x I2 x I3 x N array; multiplies the apodization arrays.  rx_normals: 3 x N element
       normals, real(prec) like Pr (float for QDAS_F16); same memory kind as Pr.                            */
    int32_t  rx_apod_kind;   /* QDAS_RXAPOD_*                                                             */
    int32_t  plan_flags;     /* QDAS_PLAN_* bits (0 = defaults)                                           */
    double   rx_apod_p[2];   /* parameters, see QDAS_RXAPOD_*                                             */
    const void *rx_normals;  /* may be NULL for QDAS_RXAPOD_NONE / QDAS_RXAPOD_FNUMBER_PLANAR             */
} qdas_desc;

typedef struct qdas_plan qdas_plan; /* opaque: device copies of geometry + strides + kernel choice */

/* ---- plan API: the reusable [k, PRE_ARGS, POST_ARGS] handle of the reference
 *      (kern/das_spec.m:72-81,387-390) */
int  qdas_plan_create(qdas_plan **plan, const qdas_desc *desc);
/* Beamform ONE frame: x is T x N x M (or T x M x N with QDAS_FLAG_TPOSE) complex(prec);
 * y is i_count x [1|N] x [1|M] complex(prec) with plane stride y_ld; y is fully
 * overwritten.  Asynchronous on `stream` when desc.mem == QDAS_MEM_DEVICE.  A plan owns device scratch (fold buffer, misfit-tile list, partial images):
 * two streams may use one plan only one after the other, with an event (or a synchronisation) between the calls; concurrent use is not supported. */
int  qdas_plan_execute(qdas_plan *plan, const void *x, void *y, void *stream);
/* F frames in one call (kern/das_spec.m:371-373 host loop): frame f uses
 * x + f*x_stride and y + f*y_stride (strides in complex elements).  Device-resident frames of a tiled plan share launches
 * (four / two per launch: tap index and interpolation weights are evaluated once per group), so a frame's image equals
 * qdas_plan_execute's to fp32 re-association, not bit for bit, and every frame of ONE call is summed in the same order.
 * A general-mode lateral-mirror plan streams F >= 4 frames through a twin plan without the mode, created at the first such
 * call (device allocations and probe launches of a plan creation, synchronous, ~plan memory x2): that first call is not
 * asynchronous and not graph-capturable; set QDAS_NO_FRAMES_TWIN=1 to keep streams on the plan's own kernel. */
int  qdas_plan_execute_frames(qdas_plan *plan, const void *x, void *y, uint64_t F,
                              uint64_t x_stride, uint64_t y_stride, void *stream);
/* Everything a stream of F frames does ONCE per plan -- the twin plan above; for a reciprocity-folded plan the second folded copy of a frame (T x N x M
 * complex64) that lets two frames share a launch; the frame-sharing kernel instantiations libqdas.so does not carry (built through hiprtc, ~2 s each);
 * the second staging set of host-resident frames -- done now, synchronously.  Optional: qdas_plan_execute_frames does the same at the plan's first
 * stream, which makes THAT call synchronous and not graph-capturable; after qdas_plan_prepare_frames(plan, F) every stream of up to F frames only enqueues. */
int  qdas_plan_prepare_frames(qdas_plan *plan, uint64_t F);
/* 'delays' (src/bf.cu:209-298, kern/das_spec.m:377): tau is i_count x N x M real(prec),
 * tau = cinv(1) * (dv + dr); no t0, like the reference. */
int  qdas_plan_delays(qdas_plan *plan, void *tau, void *stream);
void qdas_plan_destroy(qdas_plan *plan);
/* which kernel a plan resolved to (QDAS_KERNEL_GENERIC | QDAS_KERNEL_TILED) and, after an
 * execute, how many pixel tiles fell back to the generic kernel (oversize delay window) */
int  qdas_plan_kernel(const qdas_plan *plan);
int  qdas_plan_fallback_tiles(const qdas_plan *plan, uint64_t *ntiles);
/* shapes a QDAS_KERNEL_TILED plan chose from the scan's delay gradient and size: a workgroup tile of
 * tile_z pixels of I1 (64 | 32 | 16 | 8) x tile_cols columns of I2*I3, made of waves of wave_z x
 * (64 / wave_z) pixels, and ksplit workgroups per tile that each sum a slice of the aperture (> 1 when the
 * image or pixel slab has too few tiles to fill the GPU); wave_z / ksplit may be NULL; all 0 for a
 * generic-kernel plan */
int  qdas_plan_tile_shape(const qdas_plan *plan, int *tile_z, int *tile_cols, int *wave_z, int *ksplit);
/* 1 when a QDAS_KERNEL_TILED plan runs in reciprocal mode (transmit elements == receive elements, one t0: every unordered
 * transmit/receive pair is indexed and weighted once), else 0 */
int  qdas_plan_reciprocal(const qdas_plan *plan);
/* 1 when a reciprocal plan beamforms the RECIPROCITY-FOLDED frame (fp32 data; QDAS_PLAN_NO_FOLD): every execute first adds the two traces of
 * each unordered transmit/receive pair, xs[:,n,m] = w[n,m] x[:,n,m] + w[m,n] x[:,m,n] (n <= m; one pass over HBM into a plan-owned copy of the
 * frame, pixel-independent apodization applied on the way), and the fused kernel then walks the upper triangle only */
int  qdas_plan_folded(const qdas_plan *plan);
/* The reciprocity fold on its own: xs[:,n,m] = w[n,m] x[:,n,m] + w[m,n] x[:,m,n] for n < m, xs[:,n,n] = w[n,n] x[:,n,n]; traces of T samples at (n strN + m strM)
 * samples in x AND xs (0: T, T N); x complex64 (QDAS_F32) or complex32 (QDAS_F16), xs complex64 always; wtab: device N x N complex64 [n + N m] or NULL (ones);
 * only the upper triangle of xs is written (zero-fill it once).  Device pointers; asynchronous on `stream`. */
typedef struct qdas_fold_desc {
    uint64_t T, N;
    uint64_t strN, strM;
    int32_t  dtype;       /* QDAS_F32 | QDAS_F16: type of x */
    int32_t  device;      /* HIP device ordinal, -1 = current */
    const void *wtab;
} qdas_fold_desc;
int  qdas_fold(const qdas_fold_desc *d, const void *x, void *xs, void *stream);
/* bounds [samples] of the delay error committed by the lateral-mirror / reciprocal mode of the plan: 0 = exact symmetry, > 0 = accepted within
 * the tolerance of QDAS_PLAN_APPROX_SYMMETRY, -1 = that mode is not in use (either pointer may be NULL) */
int  qdas_plan_symmetry_bound(const qdas_plan *plan, double *mirror_samples, double *reciprocal_samples);
/* 1 when a QDAS_KERNEL_TILED plan runs in lateral-mirror mode (QDAS_PLAN_NO_MIRROR), else 0 */
int  qdas_plan_mirror(const qdas_plan *plan);
/* human-readable name of the kernel a plan launches for one frame, e.g.
 *   "das_tile_kernel<interp=3,f32,sym,mb=16,W=128> [prebuilt]"   |   "... [jit 5f0c...]"  (QDAS_PLAN_JIT, hiprtc build)   |
 *   "das_generic_kernel<interp=2,f64>"
 * Written NUL-terminated into buf (truncated to len). */
int  qdas_plan_kernel_name(const qdas_plan *plan, char *buf, size_t len);
/* time of the last execute()'s kernels in ms measured with hipEvents on its stream
 * (enabled by qdas_plan_set_timing(plan, 1); synchronises the stream) */
int  qdas_plan_set_timing(qdas_plan *plan, int enable);
int  qdas_plan_last_kernel_ms(const qdas_plan *plan, float *ms);

/* ---- one host thread, several devices: the image is split into ndev contiguous slabs of the linear pixel
 *      index, one per entry of devices[] (NULL: 0 .. ndev-1; an ordinal may repeat: several streams on one device); geometry and
 *      channel data are replicated, every device beamforms its slab with an ordinary plan, the slabs are concatenated into y.
 *      desc->mem == QDAS_MEM_DEVICE: the constant inputs and x / y live on devices[0]; x is replicated with peer copies over the xGMI mesh --
 *      scatter (device u pulls piece u of the frame from devices[0]) + all-gather (every device pulls the other pieces from their holders:
 *      all links carry 1/(U-1) of the frame at once) --, slabs (mirror slabs when the geometry allows: a slab of the first half of the
 *      columns AND its mirror image per device) come back with peer copies; asynchronous on `stream` (a stream of devices[0]).
 *      desc->mem == QDAS_MEM_HOST: x is uploaded once to devices[0] and replicated from there; y is downloaded; synchronous.
 *      desc->i_begin / i_count / y_ld must be 0; y is I x [1|N] x [1|M].  The reference has no multi-device path (one gpuDevice
 *      per MATLAB process, README.md:232): this is what lets its single-process host reach a whole node. */
typedef struct qdas_sharded_plan qdas_sharded_plan;
int  qdas_plan_create_sharded(qdas_sharded_plan **plan, const qdas_desc *desc, int ndev, const int *devices);
int  qdas_plan_execute_sharded(qdas_sharded_plan *plan, const void *x, void *y, void *stream);
/* shard < 0: the number of shards in *device.  Else the shard's device, pixel slab and kernel (QDAS_KERNEL_*; 0: empty slab). */
int  qdas_plan_sharded_info(const qdas_sharded_plan *plan, int shard, int *device, uint64_t *i_begin, uint64_t *i_count, int *kernel);
/* 1 when the plan runs MIRROR SLABS: shard g then owns the slab qdas_plan_sharded_info reports (whole columns of the first half of the image)
 * AND its mirror image, the pixels [I - i_begin - i_count, I - i_begin); 0: plain contiguous slabs */
int  qdas_plan_sharded_mirror(const qdas_sharded_plan *plan);
void qdas_plan_destroy_sharded(qdas_sharded_plan *plan);

/* ---- one-shot entries shaped like the reference kernels' argument lists
 *      (device pointers; sizes struct replaces the constant-memory symbols).
 *      DAS  <-> src/bf.cu:144-151, DASf <-> :153-161, DASh <-> :164-171.  The arrays may still be in the making on `stream`: the call waits for `stream`
 *      before it reads the geometry (a plan is created, executed and destroyed inside the call) and again before it returns. */
int qdas_DAS (const qdas_sizes *sz, void *y, const double *Pi, const double *Pr, const double *Pv,
              const double *Nv, const void *a, const double *cinv, const uint64_t *acstride_host,
              const void *x, const double tvars[2], void *stream);
int qdas_DASf(const qdas_sizes *sz, void *y, const float *Pi, const float *Pr, const float *Pv,
              const float *Nv, const void *a, const float *cinv, const uint64_t *acstride_host,
              const void *x, const float tvars[2], void *stream);
int qdas_DASh(const qdas_sizes *sz, void *y, const float *Pi, const float *Pr, const float *Pv,
              const float *Nv, const void *a, const float *cinv, const uint64_t *acstride_host,
              const void *x, const float tvars[2], void *stream);
/* delays <-> src/bf.cu:255-298, delaysf <-> :209-252 (tau is I x N x M) */
int qdas_delays (const qdas_sizes *sz, double *tau, const double *Pi, const double *Pr,
                 const double *Pv, const double *Nv, double cinv, void *stream);
int qdas_delaysf(const qdas_sizes *sz, float *tau, const float *Pi, const float *Pr,
                 const float *Pv, const float *Nv, float cinv, void *stream);

/* ---- split-delay flavour ("next" row): what bfDASLUT ->
 *      ChannelData.sample2sep -> wsinterpd2 computes (reference src/UltrasoundSystem.m:4641-4660,
 *      src/ChannelData.m:1431-1445, kern/wsinterpd2.m:236, src/interpd.cu:344-396) with owned
 *      outputs instead of float atomics:
 *        y[i,(n),(m)] = sum w[i,n,m] * exp(j*omega*s) * sample(x[:,n,m], s),
 *        s = tau_rx[i,n] + tau_tx[i,m]        (sample units, already (tau - t0)*fs)
 *      non-finite s are skipped (src/interpd.cu:390). */
typedef struct qdas_lut_desc {
    uint64_t T, N, M, I;      /* I pixels (any shape, flattened)                            */
    int32_t  flag;            /* interp bits + QDAS_FLAG_KEEP_RX/TX (+ TPOSE for the data)   */
    int32_t  dtype;           /* QDAS_F64 | QDAS_F32 | QDAS_F16 (delays: double|float|float) */
    double   omega;           /* imag(omega) = 2*pi*fmod/fs (src/ChannelData.m:1439)         */
    const void *tau_rx;       /* I x N real, device                                          */
    const void *tau_tx;       /* I x M real, device                                          */
    const void *w;            /* complex(prec) weights or NULL; strides below               */
    uint64_t wstride[3];      /* element strides of w for (i, n, m); 0 where singleton       */
    int32_t  w_real;          /* weights are real(prec)                                      */
    int32_t  reserved;
    uint64_t I1;              /* size of the fastest pixel dimension (the image is I1 x I/I1; 0: unknown) -- lets fp32 full-sum
                                 calls run on the fused tiled kernel, whose tiles must be compact in depth */
} qdas_lut_desc;
int qdas_das_lut(const qdas_lut_desc *d, const void *x, void *y, void *stream);
/* which kernel served the calling thread's last qdas_das_lut (diagnostic, like qdas_plan_kernel_name): "tiled,mirror [jit <key>]" (tables that are their own
 * lateral mirror images, checked bit for bit per call: a pixel and its image share tap index and weights -- fp32 full sums without weights), "tiled", "generic" */
int qdas_das_lut_last_kernel(char *buf, size_t len);

/* ---- General single-delay flavour: weighted, phase-rotated sampling over an N-D broadcast index space.  Replaces the launches of
 *      wsinterpd[f|h] (reference kern/wsinterpd.m:221-236, kernel src/interpd.cu:295-342) and interpd[f|h] (kern/interpd.m,
 *      src/interpd.cu:169-192) -- what ChannelData.sample (src/ChannelData.m:1230-1336) and focusTx run on:
 *        y[kept] = sum over summed dims of  w[j] * exp(i*omega*t[j]) * sample(x[:, j], t[j])        (t in samples, 0-based)
 *      The index space has ndim <= 8 dimensions of sizes size[]; dimension 0 is the sampling dimension (size[0] samples of t
 *      against T samples of x).  t, w and the trace bases of x address it through element strides (0 = broadcast): the reference's
 *      matching / outer dimension classification (kern/wsinterpd.m:70-93) reduces to these.  y is dense, column-major over the kept
 *      dimensions (summed ones have size 1).  Infinite t are skipped; samples outside the record give `extrap` (NaN allowed; sums
 *      omit NaN like the reference's sum(..., 'omitnan')).  All pointers are device pointers of `dtype` (t: double | float | float). */
typedef struct qdas_wsinterpd_desc {
    uint64_t T;               /* samples per trace of x                                             */
    uint64_t x_tstride;       /* element stride between consecutive samples of a trace (1: contiguous) */
    int32_t  ndim;            /* 1..8                                                               */
    int32_t  flag;            /* QDAS_INTERP_*                                                      */
    int32_t  dtype;           /* QDAS_F64 | QDAS_F32 | QDAS_F16                                     */
    int32_t  w_real;          /* weights are real(prec)                                             */
    uint64_t size[8];
    int64_t  tstride[8], xstride[8], wstride[8];   /* xstride[0] must be 0 (the sampling dimension indexes t, not x) */
    uint8_t  sum[8];          /* 1: summed dimension                                                */
    double   omega;           /* imag(omega)                                                        */
    double   extrap;          /* value of out-of-record samples                                     */
    const void *t, *w, *x;    /* w may be NULL                                                      */
    /* extension (round 4): the layout of y.  ystride all 0: dense column-major over the kept dimensions (the reference's output).  Else element
       strides per dimension (summed dimensions ignored): lets a row-major / arbitrarily strided x be sampled IN PLACE into a y of the same layout
       -- together with x_tstride / xstride no layout pass is needed.  `lane_dim`: the kept dimension the lanes of a wave run along (choose the
       one along which x -- or, where x broadcasts, t -- is contiguous); -1, a summed dimension or a dimension of one element (so also the 0 of a
       zero-initialised descriptor whose first dimension is a singleton): the first kept dimension with more than one element.                   */
    int64_t  ystride[8];
    int32_t  lane_dim;
    int32_t  reserved;
} qdas_wsinterpd_desc;
int qdas_wsinterpd(const qdas_wsinterpd_desc *d, void *y, void *stream);

/* ---- misc */
/* ---- Point-scatterer channel-data simulator: replaces the kernels greens / greensf
 * (reference src/greens.cu:88-121, body :8-86) launched by UltrasoundSystem.greens
 * (src/UltrasoundSystem.m:681-718: k.feval(x, ps, as, pn, pv, kn, sb, blocks, [t0k t0x fso fsr cinv R0], [E E], flagnum)).
 *   y[s,n,m] = 1/fsr * sum_i sum_ne sum_me a_i * sample(x, fsr*(s - (cinv*(r1+r2) + t0 - s0)*fs)) / (max(r1,R0)*max(r2,R0))
 * All pointers are DEVICE pointers; real = double (QDAS_F64) or float (QDAS_F32), complex = interleaved pairs.
 * The reference's `sb` / `blocks` arguments (per-scatterer sample windows for culling) are not needed: the kernel
 * derives the windows itself.  R0 == 0: no propagation loss (the reference's CPU branch, :797-803).
 * Two kernels, the same sum: per (entry, sample), and -- fp32 data, an integer fsr, at least QDAS_GREENS_TRAIN_MIN (1024) entries per trace -- impulse
 * trains: the interpolation fraction is one per entry, so every entry adds its K weighted amplitudes to K fixed-point trains (64-bit integer LDS atomics:
 * the result does not depend on the order of arrival, bit-reproducible) and one dense convolution with the waveform per block of samples follows.  The two
 * agree to fp32 re-association (~1e-6 of the peak); an entry whose fp32 delay lies on a tap boundary may land on either side (csrc/greens.hip). */
typedef struct qdas_greens_desc {
    uint64_t S;            /* output samples per trace                          (QUPS_S) */
    uint64_t T;            /* samples of the waveform x                          (QUPS_T) */
    uint64_t N, M, I;      /* receivers, transmitters, scatterers                         */
    int32_t  En, Em;       /* sub-apertures per receive / transmit element       (E)      */
    int32_t  interp;       /* QDAS_INTERP_*                                      (iflag)  */
    int32_t  dtype;        /* QDAS_F64 | QDAS_F32                                         */
    double   s0;           /* time of output sample 0 [s]                        (t0k)    */
    double   t0;           /* time of waveform sample 0 [s]                      (t0x)    */
    double   fs;           /* output sampling frequency [Hz]                     (fso)    */
    double   fsr;          /* waveform sampling frequency / fs                            */
    double   cinv;         /* 1 / sound speed                                             */
    double   R0;           /* minimum distance of the 1/(r1 r2) loss; 0 = no loss         */
    const void *Ps;        /* 3 x I   scatterer positions, real                           */
    const void *a;         /* I       scatterer amplitudes, complex                       */
    const void *Pr;        /* 3 x N x En receive (sub-)element positions, real            */
    const void *Pv;        /* 3 x M x Em transmit (sub-)element positions, real           */
    const void *x;         /* T       waveform samples, complex                           */
    int32_t  device;       /* HIP device ordinal, -1 = current                            */
    int32_t  reserved;
} qdas_greens_desc;
int qdas_greens(const qdas_greens_desc *desc, void *y /* S x N x M complex */, void *stream);

/* ---- Transmit synthesis (UltrasoundSystem.focusTx, reference src/UltrasoundSystem.m:3374-3503): delay-and-sum over the transmit ELEMENTS of a
 * full-synthetic-aperture record,
 *     y[t', n, m'] = sum_m  w[m, m'] * x(t' + shift[m, m'],  n, m),      t' = 0 .. To-1,
 * the call the reference makes as sample2sep(chd.time, -tau, interp, apd, mdim) (:3498 -> kern/wsinterpd2.m -> src/interpd.cu:344-396) with the
 * positions written as the record's own time grid plus one offset per (element, synthesised transmit) [samples; shift = -tau * fs after the
 * reference's re-basing of the time axis, :3457-3463].  qdas_wsinterpd computes the same numbers from a materialised position array; this entry
 * uses the structure (per-pair tap offset and weights, LDS-staged windows, uniform skips of zero weights; csrc/shiftsum.hip).
 * x: T x N x M x F, y: To x N x Mo x F column-major DEVICE arrays of `dtype` (QDAS_F64 | QDAS_F32), complex or real; shift: M x Mo real(dtype),
 * w: M x Mo real(dtype) or complex(dtype) or NULL (ones) -- DEVICE arrays, m fastest.  Real data take real weights.
 * Edge rule as in every kernel: a term counts iff all its taps lie in [0, T) and its position is >= 0. */
typedef struct qdas_shift_desc {
    uint64_t T, To, N, M, Mo, F;
    int32_t  flag;      /* interpolation, bits 0-2 of QUPS_BF_FLAG */
    int32_t  dtype;     /* QDAS_F64 | QDAS_F32                     */
    int32_t  cplx;      /* samples are interleaved complex         */
    int32_t  w_real;    /* w holds real(dtype) weights             */
    int32_t  device;    /* HIP device ordinal, -1 = current        */
    int32_t  tpad;      /* the last tpad of the T samples of a trace are ZEROS that are not stored: x holds T - tpad samples per trace (that is its stride);
                         * a tap in the tail counts as an in-range zero -- ChannelData.zeropad in front of the sampling (src/UltrasoundSystem.m:3479) without the copy */
    const void *shift;
    const void *w;
} qdas_shift_desc;
int qdas_shift_sum(const qdas_shift_desc *desc, const void *x, void *y, void *stream);

/* ---- Batched 1-D convolution along one dimension (band-pass / matched filtering of the traces in front of DAS).
 * Replaces the kernels conv / convf / convc / convcf (reference src/convd.cu:95-127,130-146) launched by kern/convd.m:150-199
 * (kern.feval(x, y, z, sizes) with the constant L0).  x: C x M x S, y: C x N x S, z: C x L x S, column-major, all DEVICE pointers,
 * real or interleaved complex of `dtype`; C = product of the dimensions in front of the convolved one, S = of those behind it:
 *   z[c,l,s] = sum_i x[c,i,s] * y[c, l + off - i, s]
 * 'full': L = M+N-1, off = 0; 'same': L = M, off = N-1 - floor((N-1)/2); 'valid': L = max(M-N+1, 0), off = N-1
 * (kern/convd.m:103-114).  A singleton column / slice dimension of x or y is broadcast (bits of `bcast`) instead of being
 * replicated as the reference does (kern/convd.m:75-84).  QDAS_F16: the half-precision twins convh / convch (src/convd.cu:141,153) --
 * products and sums in fp32, rounded once at the store (the reference accumulates in half).
 * Long filters: complex64 traces with C == 1 (time contiguous), one filter for all slices, N >= QDAS_CONV_FFT_MIN_TAPS (128) and M + N - 1 <= 8192 take an
 * FFT convolution with the trace resident in LDS (csrc/pre.hip): the same outputs to fp32 rounding (a few 1e-6 of the largest), O(L log L) per trace. */
#define QDAS_CONV_FULL  0
#define QDAS_CONV_SAME  1
#define QDAS_CONV_VALID 2
#define QDAS_CONV_CAUSAL 3         /* extension: L = M, off = 0 -- the first M samples of the full convolution = MATLAB filter(b, 1, x), what
                                      ChannelData.filter applies with an FIR digitalFilter (reference src/ChannelData.m:857-880)            */
#define QDAS_CONV_X_ONE_COLUMN 1   /* x is 1 x M x (S | 1) */
#define QDAS_CONV_X_ONE_SLICE  2   /* x is (C | 1) x M x 1 */
#define QDAS_CONV_Y_ONE_COLUMN 4
#define QDAS_CONV_Y_ONE_SLICE  8
typedef struct qdas_convd_desc {
    uint64_t C, M, N, S;
    int32_t  dtype;    /* QDAS_F64 | QDAS_F32 | QDAS_F16         */
    int32_t  cplx;     /* 0: real data, 1: interleaved complex   */
    int32_t  shape;    /* QDAS_CONV_*                            */
    int32_t  bcast;    /* QDAS_CONV_{X,Y}_ONE_{COLUMN,SLICE}     */
    int32_t  device;   /* HIP device ordinal, -1 = current       */
    int32_t  y_real;   /* extension (cplx == 1): y holds REAL taps of `dtype` -- a real filter on complex traces costs half the multiplies
                          of the promoted product the reference forms (kern/convd.m:259-268 makes both operands complex) */
} qdas_convd_desc;
uint64_t qdas_convd_len(uint64_t M, uint64_t N, int shape);    /* L */
int qdas_convd(const qdas_convd_desc *desc, const void *x, const void *y, void *z, void *stream);

/* ---- Recursive (IIR) filtering along time: what ChannelData.filter applies with an IIR digitalFilter (reference src/ChannelData.m:857-888:
 * filter(D, x) -- a cascade of second-order sections, each the direct-form II transposed recursion -- then t0 -= filtord(D) / fs).
 * x, y: T x K DEVICE arrays of `dtype` (QDAS_F64 | QDAS_F32), real or interleaved complex, time contiguous (K = every other dimension flattened); y may be x.
 * sos: HOST array, nsec x 6 row-major [b0 b1 b2 a0 a1 a2] per section (MATLAB's D.Coefficients / scipy's sos); gain: overall scale (0 = 1).
 * One read and one write of the record whatever the order (iir.hip); the state is kept in double. */
typedef struct qdas_iir_desc {
    uint64_t T, K;
    int32_t  nsec;     /* 1 .. 16 second-order sections */
    int32_t  dtype;    /* QDAS_F64 | QDAS_F32           */
    int32_t  cplx;     /* samples are interleaved complex */
    int32_t  device;   /* HIP device ordinal, -1 = current */
    double   gain;
    const double *sos;
} qdas_iir_desc;
int qdas_iir(const qdas_iir_desc *desc, const void *x, void *y, void *stream);

/* ---- Aperture-reduction images of a receive-kept image (SYN output of DAS, I1 x I2 x I3 x ... x N): the MATLAB branches of the reference's
 * kern/slsc.m (average / ensemble estimator, optional time-kernel dimension), kern/dmas.m, kern/cohfac.m and kern/pcf.m (coherence.hip).
 * x: DEVICE array of `dtype` (QDAS_F64 | QDAS_F32), real or interleaved complex, in a strided layout: the output pixels are up to three
 * (size, stride) groups, group 0 the fastest; the reduced aperture has N elements at stride strideN, an optional second reduced dimension K at
 * strideK (SLSC: the time kernel `kdim`; cohfac: its second `dim`; K = 0 reads as 1).  Strides count elements (complex samples when cplx).
 * Pixels should be the fastest dimension (coalesced loads); any strides are computed correctly.
 * y: DEVICE array of P = size[0] size[1] size[2] outputs, group 0 fastest: SLSC / DMAS: `dtype`, complex when cplx (SLSC's imaginary part is 0 in
 * exact arithmetic and is written as such, except NaN where the reference gives NaN); cohfac, pcf: real `dtype` (pcf's w).  y2: pcf's sf (real),
 * NULL otherwise.  The sizes are taken as given: an unused group is (1, 0), and a size of 0 is an empty image -- the arguments are validated,
 * nothing is launched, x / y / y2 may be NULL.  Lags (SLSC, DMAS): the range lag_lo .. lag_hi when lags == NULL (a scalar L of the reference is 1 .. L), else the host
 * table lags[0 .. nlags-1] (the reference's vector L; read during the call only; lags above 2047 that have pairs: QDAS_EUNSUPPORTED).  SLSC
 * normalises by L = the number of lags as given (duplicates and lags >= N included, kern/slsc.m:136-139) and counts lag 0 once (the MATLAB branch,
 * not src/slsc.cl); an empty set is QDAS_EINVAL.  DMAS uses the lags in 1 .. N-1 (an empty set gives 0).  gamma: pcf's gamma (the reference's default
 * is 1; 0 is taken as given).  One kernel launch on `stream`, no temporaries, no host synchronisation. */
#define QDAS_COH_SLSC_AVERAGE  1
#define QDAS_COH_SLSC_ENSEMBLE 2
#define QDAS_COH_DMAS          3
#define QDAS_COH_COHFAC        4
#define QDAS_COH_PCF           5
typedef struct qdas_coherence_desc {
    int32_t  method;              /* QDAS_COH_*                                  */
    int32_t  dtype;               /* QDAS_F64 | QDAS_F32                         */
    int32_t  cplx;                /* samples are interleaved complex             */
    int32_t  device;              /* HIP device ordinal, -1 = current            */
    uint64_t N, K;                /* reduced aperture; second reduced dimension  */
    int64_t  strideN, strideK;
    uint64_t size[3];             /* pixel groups, fastest first; unused: (1, 0) */
    int64_t  stride[3];
    uint64_t lag_lo, lag_hi;      /* lag range when lags == NULL                 */
    const int64_t *lags;          /* host lag table, or NULL                     */
    uint64_t nlags;
    double   gamma;               /* pcf                                         */
} qdas_coherence_desc;
int qdas_coherence(const qdas_coherence_desc *desc, const void *x, void *y, void *y2, void *stream);

/* ---- Travel times through a sound-speed map, and the delay tables sampled from them (eikonal.hip): what the reference's bfEikonal computes with
 * kern/msfm.m (two arguments: first order, four neighbours) and griddedInterpolant(grd, T, 'cubic', 'none') (src/UltrasoundSystem.m:4283-4321).
 * c: DEVICE C1 x C2 doubles, C1 fastest (a MATLAB matrix as it lies in memory): the speed; c / dp is msfm's F in cells per second (dp = 1: c is F).
 * src: HOST 2 x npts doubles, one (first, second) grid coordinate per point in the index base `base` (1: msfm's own), floored to a node as the
 * reference does; source set k owns the points set_begin[k] .. set_begin[k+1]-1 (a host table of K + 1 entries; NULL: one point per set, npts == K).
 * A point outside the grid is QDAS_EINVAL.  T: DEVICE C1 x C2 x K doubles, seconds (0 at the source nodes).
 * qdas_eikonal solves all K sets with the same launches, in double precision, by a block-based fast iterative method that ends at the FIXED POINT of the
 * update rule (a pass in which no node changes) -- the numbers fast marching produces, to rounding.  It WAITS for the stream (the host ends the iteration).
 * The number of passes is capped: max_passes, or with 0 qdas_eikonal_pass_cap(C1, C2) = 8 (C1 + C2) + 64.  Reaching the cap returns QDAS_ENOCONV,
 * the maps are set to NaN.  qdas_eikonal_last_passes: the passes the calling thread's last solve took.  C1 C2 = 0 or K = 0: nothing is launched.
 * Limits of one call: fewer than 2^24 tiles of 16 x 16 nodes per map, K <= 65535, I <= 2^32 - 256 (QDAS_EUNSUPPORTED beyond).  Work space comes from the stream's arena (below).
 * qdas_eikonal_tables: tau[i + I k] = map k at pixel i, for I pixels given as DEVICE 2 x I grid coordinates Pi (same base): separable cubic convolution
 * (Keys, a = -1/2; ghost nodes outside the border by Keys' rule f(-1) = 3 f(0) - 3 f(1) + f(2)), NaN for a pixel outside the grid; a pixel on a node gets the
 * node's value.  One launch on `stream`, no synchronisation.  tau is the I1 x I2 x I3 x N layout of qdas_das_lut's tables. */
typedef struct qdas_eikonal_desc {
    uint64_t C1, C2;              /* grid nodes, C1 fastest                          */
    uint64_t K;                   /* source sets = maps (at most 65535 per call)     */
    uint64_t npts;                /* source points in all (qdas_eikonal)             */
    const uint64_t *set_begin;    /* host, K + 1 entries, or NULL                    */
    double   dp;                  /* grid step (qdas_eikonal)                        */
    int32_t  base;                /* index base of src / Pi: 0 | 1                   */
    int32_t  device;              /* HIP device ordinal, -1 = current                */
    uint32_t max_passes;          /* 0 = qdas_eikonal_pass_cap(C1, C2)               */
    uint32_t reserved;
    uint64_t I;                   /* pixels (qdas_eikonal_tables)                    */
} qdas_eikonal_desc;
int qdas_eikonal(const qdas_eikonal_desc *desc, const double *c, const double *src, double *T, void *stream);
int qdas_eikonal_tables(const qdas_eikonal_desc *desc, const double *T, const double *Pi, double *tau, void *stream);
int qdas_eikonal_last_passes(void);
uint32_t qdas_eikonal_pass_cap(uint64_t C1, uint64_t C2);

/* ---- Travel times through a sound-speed VOLUME, and the delay tables sampled from them (eikonal3.hip): what the reference's bfEikonal computes when the
 * grid has three non-singleton dimensions -- msfm3d with two arguments (first order, six neighbours) and griddedInterpolant({g1, g2, g3}, T, 'cubic', 'none')
 * (src/UltrasoundSystem.m:4251-4321).  The 2-D entries' contract above holds with a third coordinate; what differs is stated here.
 * c: DEVICE C1 x C2 x C3 doubles, C1 fastest (a MATLAB array as it lies in memory); c / dp is msfm's F in cells per second.  src: HOST 3 x npts doubles, one
 * (first, second, third) grid coordinate per point in the index base `base`, floored to a node; source set k owns the points set_begin[k] ..
 * set_begin[k+1]-1 (NULL: one point per set, npts == K).  T: DEVICE C1 x C2 x C3 x K doubles, seconds (0 at the source nodes).
 * qdas_eikonal3 solves all K sets with the same launches, in double precision: tiles of 8 x 8 x 8 nodes, worked off an ACTIVE LIST of (set, tile) pairs, one
 * launch per pass, to the FIXED POINT of the classical first-order upwind update (a pass that enlists nothing) -- the numbers heap fast marching with
 * msfm3d's rule produces, to rounding.  No floating-point atomics.
 * STREAM.  The hipStream_t travels in the descriptor's `queue` field (as qdas_refocus, and for its reason).  qdas_eikonal3 WAITS for that stream: the host
 * reads the list lengths back every few passes and ends the iteration.  qdas_eikonal3_tables is one launch on `queue`, no synchronisation.
 * WORK SPACE.  The caller provides it: DEVICE memory of at least qdas_eikonal3_work_bytes(desc) bytes (the same C1, C2, C3, K, npts), aligned to 16 bytes;
 * the library's per-stream arenas are not used and nothing the work space held before the call is read.  On return its first 8 bytes hold, as a uint64, the
 * number of tile visits of the solve (the sum of the list lengths over the passes): K tiles passes of them would be a solver without the list.
 * The number of passes is capped: max_passes, or with 0 qdas_eikonal3_pass_cap(C1, C2, C3) = 8 (C1 + C2 + C3) + 64.  Reaching the cap returns QDAS_ENOCONV and
 * the maps are set to NaN.  *passes (unless NULL) receives the passes taken; it replaces the 2-D entry's thread-local.
 * All validation happens on the host before any HIP call: a null descriptor or data pointer, dp <= 0, a base other than 0 | 1, npts != K without set_begin, a
 * set_begin that does not ascend to npts, an empty set, a point outside the grid, a work space that is too small or misaligned are QDAS_EINVAL;
 * C1 C2 C3 = 0 or K = 0 is QDAS_OK, nothing is launched, no device needed (work_bytes gives 0); K > 65535, 2^24 or more tiles per map, 2^31 or more nodes in
 * a dimension, I > 2^32 - 256 are QDAS_EUNSUPPORTED.
 * qdas_eikonal3_tables: tau[i + I k] = map k at pixel i, for I pixels given as DEVICE 3 x I grid coordinates Pi (same base): separable cubic convolution
 * (Keys, a = -1/2) along dimension 1, then 2, then 3, the 2-D sampler's ghost nodes dimension by dimension in that order, NaN for a pixel outside the grid; a
 * zero weight reads nothing, so a pixel on a node gets the node's value bit for bit.  tau is the I1 x I2 x I3 x N layout of qdas_das_lut's tables. */
typedef struct qdas_eikonal3_desc {
    uint64_t C1, C2, C3;          /* grid nodes, C1 fastest (a MATLAB C1 x C2 x C3 array as it lies in memory) */
    uint64_t K, npts;             /* source sets = maps; source points in all                                  */
    const uint64_t *set_begin;    /* host, K + 1 entries, or NULL (one point per set)                          */
    double   dp;                  /* grid step                                                                  */
    int32_t  base, device;        /* index base of src / Pi: 0 | 1; HIP ordinal, -1 = current                   */
    uint32_t max_passes, reserved;/* 0 = qdas_eikonal3_pass_cap(C1, C2, C3)                                     */
    uint64_t I;                   /* pixels (tables)                                                            */
    void    *queue;               /* a hipStream_t                                                              */
} qdas_eikonal3_desc;
uint32_t qdas_eikonal3_pass_cap(uint64_t C1, uint64_t C2, uint64_t C3);
int qdas_eikonal3_work_bytes(const qdas_eikonal3_desc *d, uint64_t *bytes);
int qdas_eikonal3(const qdas_eikonal3_desc *d, const double *c, const double *src /* HOST 3 x npts */, double *T,
                  void *work, uint64_t work_bytes, uint32_t *passes /* out, may be NULL */);
int qdas_eikonal3_tables(const qdas_eikonal3_desc *d, const double *T, const double *Pi /* DEVICE 3 x I */, double *tau);

/* ---- Frequency-domain adjoint beamformer (adjoint.hip): the frequency loop of the reference's bfAdjoint (src/UltrasoundSystem.m:3997-4037) as ONE call.
 * For every pixel i and selected frequency f_k, with tau_rx(i,n) = |Pr_n - Pi| cinv(i), tau_tx(i,m) = |Pt_m - Pi| cinv(i):
 *   S[m,v,k] = apod_tx[m,v] exp(-2 pi i f_k del_tx[m,v])
 *   A[i,v,k] = sum_m exp(-2 pi i f_k tau_tx(i,m)) S[m,v,k],   Ahat = A / ||A[i,:,k]||_2 (norm over v; a zero norm divides, as the reference does)
 *   R[i,v,k] = sum_n a_n(i,n) exp(+2 pi i f_k tau_rx(i,n)) X[k,v,n]
 *   b[i]     = sum_k sum_v a_m(i,v) R[i,v,k] conj(Ahat[i,v,k])               keep_tx: no sum over v, b[i,v]
 *   keep_rx: b[i,n] = sum_k sum_v a_m a_n exp(+2 pi i f_k tau_rx) X[k,v,n] conj(Ahat[i,v,k])           with keep_tx: b[i,n,v]
 * X: DEVICE complex64 Ksel x V x N, n fastest (MATLAB's N x V x F block as it lies in memory); b: DEVICE complex64 I x [N] x [V], pixel fastest.
 * Without keep_rx the two contractions run on the f32 matrix cores (v_mfma_f32_32x32x2_f32; the phasor operand is generated per lane, phases formed in
 * fp64 and reduced to a fractional cycle first); with keep_rx plain vector kernels.  No floating-point atomics: results are bit-reproducible.
 * Every pointer but `freq` is a DEVICE pointer; freq is a HOST table.  dtype: QDAS_F32 only (QDAS_F16 / QDAS_F64: QDAS_EUNSUPPORTED).
 * An image without elements (I = 0, N = 0 with keep_rx, V = 0 with keep_tx): nothing is launched.  Otherwise N, V or Ksel = 0 is an empty sum: b is set
 * to zero by a memset, no kernel runs.  M = 0 with everything else positive is QDAS_EINVAL (the transmit field has no norm).
 * Work space: the steering matrix S (Ksel V M complex64), the partial images of split frequencies, and -- keep_tx / keep_rx -- per-pixel tables, for
 * which the pixels are processed in blocks of at most 256 MiB.  It is taken through the stream's arena (below), so the call MAY BLOCK the host: any
 * single piece above 64 MiB (S at Ksel V M > 2^23, e.g. 1024 x 128 x 128; a full pixel block) is a hipMalloc of its own that is freed, after a
 * stream synchronisation, before the call returns.  Smaller calls only enqueue work. */
typedef struct qdas_adjoint_desc {
    uint64_t I, N, M, V, Ksel;    /* pixels, receivers, transmit elements, transmits, selected frequencies */
    const float *Pi, *Pr, *Pt;    /* 3 x I, 3 x N, 3 x M positions                    */
    const float *cinv;            /* 1 / sound speed: cinv_count values               */
    uint64_t cinv_count;          /* 1 | I                                            */
    const double *freq;           /* HOST: Ksel frequencies [Hz]                      */
    const double *del_tx;         /* M x V, m fastest: delays(seq, tx) + t0Offset [s] */
    const float *apod_tx;         /* M x V, m fastest                                 */
    const float *a_n;             /* I x N, pixel fastest, or NULL = 1                */
    const float *a_m;             /* I x V, pixel fastest, or NULL = 1                */
    int32_t  keep_rx, keep_tx;    /* 0 | 1                                            */
    int32_t  dtype;               /* QDAS_F32                                         */
    int32_t  device;              /* HIP device ordinal, -1 = current                 */
} qdas_adjoint_desc;
int qdas_adjoint(const qdas_adjoint_desc *desc, const void *X, void *b, void *stream);

/* ---- Plane-wave Stolt f-k migration (migration.hip): the reference's bfMigration (src/UltrasoundSystem.m:4675-4887) as ONE call.
 * Per transmit m of x[t, n, m, frame] (complex64, T x N x M x frames, time fastest), with transform lengths F (time) and K (lateral),
 * f_j = (j - floor(F/2)) fs / F, kx_k = (k - floor(K/2)) / K / pitch, cs = c0 / sqrt(2):
 *   1. x *= exp(2 pi i fmod (t0 + t / fs));  X = fftshift(FFT_t(x, F))            (zero-padded or truncated to F)
 *   2. X *= exp(-2 pi i f (t0 + tau[n, m]))
 *   3. X  = fftshift(FFT_n(X, K))                                                  (zero-padded or truncated to K)
 *   4. y[j, k] = interp(X[:, k], kkz[j, k]),  kkz = sign(j0) sqrt(a^2 + j0^2) + floor(F/2),  j0 = j - floor(F/2),  a = kx cs F / fs
 *      (fp64; the interpolators and the support rule of qdas_wsinterpd: all taps in [0, F) and kkz >= 0, else 0)
 *   5. jacobian: y *= (f / cs) / (fkz + eps),  fkz = cs sign(f) sqrt(kx^2 + f^2 / cs^2)
 *   6. y *= exp(+2 pi i f t0);  b = IFFT_t(ifftshift(y))
 *   7. b *= exp(2 pi i kx gamma[m] z),  z = c0 / 2 (t0 + (0 : F-1) / fs)
 *   8. b = IFFT_k(ifftshift(b));  9. crop to min(T, F) x min(N, K);  10. sum over m unless keep_tx (the sum is taken in front of step 8)
 * b: DEVICE complex64 min(T,F) x min(N,K) x [M] x frames, time fastest.  tau (N x M, n fastest) and gamma (M) are DEVICE doubles.
 * Four passes over an F x K x (block of transmits) work buffer, FFTs resident in LDS, no atomics: results are bit-reproducible.
 * F and K must be lengths the in-LDS transforms take -- products of 2, 3, 5, 7, 11, 13 from 2 to 8192 whose stages fit a workgroup, and K <= 600 (two
 * 16 x K tiles in LDS) -- otherwise QDAS_ENOTLDS and nothing is launched.  T, N, M or frames = 0: QDAS_OK, nothing is launched, no device needed.
 * All validation happens on the host before any launch.  Work space comes from the stream's arena (below): the transmits are taken in blocks
 * of at most 64 MiB (QDAS_MIGRATION_BLOCK_BYTES), so that no single piece is a hipMalloc of its own. */
typedef struct qdas_migration_desc {
    uint64_t T, N, M, frames;     /* samples, receivers, transmits, frames                          */
    uint64_t F, K;                /* transform lengths in time and laterally                        */
    double   fs, fmod, t0;        /* sampling frequency, modulation frequency, time of sample 0    */
    double   c0, pitch;           /* sound speed, element pitch                                     */
    int32_t  flag;                /* interpolator: 0 nearest, 1 linear, 2 cubic, 3 lanczos3, 5 cubic_dev */
    int32_t  keep_tx, jacobian;   /* 0 | 1                                                          */
    int32_t  device;              /* HIP device ordinal, -1 = current                               */
    const double *tau;            /* N x M, n fastest: the sequence's delays at c0 [s]              */
    const double *gamma;          /* M: sin(theta) / (2 - cos(theta))                               */
} qdas_migration_desc;
int qdas_migration(const qdas_migration_desc *desc, const void *x, void *b, void *stream);

/* ---- REFoCUS (refocus.hip): the reference's UltrasoundSystem.refocus (src/UltrasoundSystem.m:3505-3768) with the decoder given -- channel data of V
 * transmit pulses x[t, n, v, frame] (complex64, T x N x V x frames, time fastest) back to the full-synthetic-aperture data of M transmit elements.
 * With f_k = k fs / T for k = 0 .. T-1 (ChannelData.fftaxis: NOT wrapped to negative frequencies) and the decoder pages Hi_k (M x V):
 *   1. X = FFT_t(x) exp(-2 pi i f_k t0[v])
 *   2. Y_k[n, m] = sum_v Hi_k[m, v] X_k[n, v]
 *   3. Y *= exp(+2 pi i f_k t0_out),  t0_out = min(t0);   y = IFFT_t(Y)
 * y: DEVICE complex64 T x N x M x frames, time fastest; its sample 0 is at t0_out.  Hi: DEVICE complex64 M x V x T, m fastest -- the reference's order, so a
 * MATLAB caller passes its own Hi unchanged; how the pages are built from the sequence's delays and apodization (adjoint, tikhonov, pinv) is the
 * caller's business (qups_amd/refocus.py builds them on the host in float64, once per sequence).  With one_t0 the two phases cancel and neither is applied.
 * Three passes of complex64 (time FFT in LDS, the per-frequency products on the f32 matrix cores, inverse FFT in LDS), no atomics: results are
 * bit-reproducible.
 * STREAM.  The call is asynchronous on the hipStream_t in the descriptor's `queue` field: no synchronisation, no allocation.  It travels in the descriptor and
 * not as a trailing parameter because the census of the entries that take one (tests/test_streams_host.py) is a pinned list; the entry's stream case
 * lives in tests/test_gpu_refocus.py until that list may change.
 * WORK SPACE.  The caller provides it (the work_bytes entry tells how much: T twiddles, then T x V x N frames and T x M x N frames complex64); the library's
 * per-stream arenas are not used and nothing the work space held before the call is read.
 * All validation happens on the host before any HIP call: null pointers and a work space that is too small are QDAS_EINVAL; T, N, V, M or frames = 0 is
 * QDAS_OK, nothing is launched (y is not written), no device needed; a T the in-LDS transforms do not take (qdas_migration's rule: products of 2, 3, 5, 7, 11, 13 from 2 to
 * 8192 whose stages fit a workgroup) is QDAS_ENOTLDS, nothing is launched (the caller composes the result instead); more than 65535 pulses or elements,
 * or N * frames beyond 2^31 - 256, QDAS_EUNSUPPORTED. */
typedef struct qdas_refocus_desc {
    uint64_t T, N, V, M, frames;  /* samples, receivers, transmit pulses, transmit elements, frames */
    double   fs, t0_out;          /* sampling frequency; min(t0): the time of sample 0 of y         */
    int32_t  device, one_t0;      /* HIP device ordinal, -1 = current; 1: t0 is one value           */
    const double *t0;             /* DEVICE, V or 1 values (not read when one_t0)                   */
    void    *queue;               /* a hipStream_t                                                  */
} qdas_refocus_desc;
int qdas_refocus_work_bytes(const qdas_refocus_desc *desc, uint64_t *bytes);
int qdas_refocus(const qdas_refocus_desc *desc, const void *x, const void *Hi, void *y, void *work, uint64_t work_bytes);

/* ---- Straight-ray integrals over a rectilinear grid (raypaths.hip): the reference's kern/wbilerpg.m (bilinear ray weights), kern/rayPaths.m (the tomography
 * system matrix) and kern/globalAverageC.m (the integral of a slowness map along straight rays).  The grid vectors xg (X values) and zg (Z values) are strictly
 * increasing and need not be uniform -- the caller's promise, not checked here.  Ray j runs from pa[j] to pb[j]; it is cut at every crossing with a grid line and
 * at its end points, and only the part inside [xg[0], xg[X-1]] x [zg[0], zg[Z-1]] counts (end points outside are clipped).  A segment of length l inside one
 * cell gives each of the cell's four corners l times the mean of that corner's bilinear hat function along the segment: the four weights sum to l, the weights
 * of a ray to its clipped length, and sum(w f) is the exact line integral of the bilinear interpolant of f.  No weight is negative.  A ray of zero length, one
 * that misses the grid and one with a non-finite coordinate give nothing.  One lane per ray, in the order given; the crossings are merged on the fly from the
 * grid vectors (kept in LDS, less their first value), never listed or sorted; the walk takes at most K = X + Z + 1 steps whatever the data holds.
 *   qdas_raypaths_weights    w, ix, iz: DEVICE, 4 x K x J (the 4 corners (ix, iz), (ix+1, iz), (ix, iz+1), (ix+1, iz+1) of a slot together, then the slot, then
 *                            the ray), w of `dtype`, each aligned to 4 of its elements.  EVERY slot is written: one that holds nothing gets w = 0,
 *                            ix = iz = -1; indices are 0-based.  Which slot a segment lands in is not part of the contract, the dense sum is.
 *   qdas_raypaths_integrate  y[j + J f] = sum w map_f[iz zstride + ix xstride] for the F maps (DEVICE, of `dtype`, X Z elements apart), in path order, and
 *                            -- unless NULL -- len[j] = sum w, the clipped length.  The triplets are never formed.
 * Sums run in the data's precision, no atomics: results are bit-reproducible.
 * STREAM.  Both calls are asynchronous on the hipStream_t in the descriptor's `queue` field (as qdas_refocus, and for its reason): no synchronisation, no
 * allocation, no work space of the library's.  All validation happens on the host before any HIP call: a null descriptor or pointer, X < 2, Z < 2, a point
 * stride other than 0 | 1 is QDAS_EINVAL; J = 0 (F = 0) is QDAS_OK, nothing is launched, the pointers may be NULL; grid vectors beyond 64 KiB of LDS
 * (X + Z > 8192 doubles, 16384 singles), more than 65535 maps, more than 2^31 - 1 workgroups of 256 rays or element counts beyond 2^60: QDAS_EUNSUPPORTED. */
typedef struct qdas_raypaths_desc {
    uint64_t X, Z, J, F;          /* grid nodes, rays, maps (integrate) | vectors (backproject) */
    int64_t  xstride, zstride;    /* map / dense-index strides in elements ('ZX': Z, 1; 'XZ': 1, X) */
    int64_t  pa_stride, pb_stride;/* rays: 1, or 0 = one point for every ray                    */
    int32_t  dtype, device;       /* QDAS_F32 | QDAS_F64; HIP ordinal, -1 = current             */
    const void *xg, *zg, *pa, *pb;/* DEVICE: X, Z values; 2 x J (or 2) points, (x, z) pairs     */
    void    *queue;               /* a hipStream_t                                              */
} qdas_raypaths_desc;
uint64_t qdas_raypaths_slots(uint64_t X, uint64_t Z);                       /* X + Z + 1 */
int qdas_raypaths_weights(const qdas_raypaths_desc *d, void *w, int32_t *ix, int32_t *iz);
int qdas_raypaths_integrate(const qdas_raypaths_desc *d, const void *maps, void *y, void *len /* may be NULL */);
/* The transposed product -- back-projection onto the grid, MATLAB's w' * r on the matrix rayPaths returns: with w the weights of qdas_raypaths_weights,
 *   g_f[iz zstride + ix xstride] = sum_j w_j(ix, iz) r[j + J f]     for the F residual vectors r (DEVICE, of `dtype`), the maps g_f X Z elements apart, and
 *   colsum[iz zstride + ix xstride] = sum_j w_j(ix, iz)             -- unless NULL -- the column sums of the matrix.
 * A gather: a lane owns a node and asks every ray for its weight (the node's two hat functions are piecewise linear along the ray: at most three pieces), a
 * wave a tile of 8 x 8 nodes, and the sum runs in ray order in the data's precision -- no atomics, bit-reproducible, whatever the launch geometry.  EVERY
 * addressed element of every map is stored exactly once (a node no ray reaches gets 0): the caller need not clear.  A ray that gives nothing in the forward
 * entries gives nothing here and its r[j] is not looked at: a NaN in r[j] reaches exactly the nodes ray j weighs.  The weights agree with those of the forward
 * entries to rounding, not bit for bit.
 * F = 0: a non-NULL colsum is the whole job (r and g may be NULL); with colsum NULL too nothing is launched.  J = 0 writes zeros to the F maps and to colsum
 * (pa, pb and r may be NULL).  Stream, validation and limits as the two calls above (the same grids are taken both ways), F <= 65535. */
int qdas_raypaths_backproject(const qdas_raypaths_desc *d, const void *r, void *g, void *colsum /* may be NULL */);

/* ---- Scan conversion (scanconvert.hip): the reference's ScanPolar.scanConvert (src/ScanPolar.m:143-201: cart2pol, then interp2 per page, NaN outside) and
 * ScanSpherical.scanConvert (src/ScanSpherical.m:121-188: cart2sph, then interp3) -- an image on a polar grid, b[R x A x pages], or a volume on a spherical
 * grid, b[R x A x E x pages], onto the Cartesian axes z[Z], x[X] (and y[Y]): out is Z x X x pages (Z x X x Y x pages), dense, Z fastest ('ZXY').  Pages of a
 * volume are this library's extension.  The source is read in place through its strides (the view DAS returns; complex samples count as one element).
 * GEOMETRY is float64 whatever the data; the angle axes a, e are in RADIANS (the Python layer and the gateway take degrees as the reference does and convert
 * with a * pi / 180).  For output pixel (i, j[, y]) with dz = z[i] - origin[2], dx = x[j] - origin[0], dy = y[.] - origin[1]:
 *   polar      rho = hypot(dz, dx),                alpha = atan2(dx, dz)                                      (cart2pol(Z - oz, X - ox))
 *   spherical  rho = sqrt(dx^2 + dy^2 + dz^2),     alpha = atan2(dx, dz),   eps = atan2(dy, hypot(dz, dx))    (cart2sph(Z - oz, X - ox, Y - oy))
 * The pixel is INSIDE iff r[0] <= rho <= r[R-1] and a[0] <= alpha <= a[A-1] (and e[0] <= eps <= e[E-1]): both ends closed, as interp2; a non-finite coordinate
 * is outside; there is no angle wrap, because the reference has none.  The range cell is the largest k <= R - 2 with r[k] <= rho and
 * u = (rho - r[k]) / (r[k+1] - r[k]); the angle cells l (m) and weights v (w) follow the same rule: a point on the last node has the last cell and weight 1.
 * With u, v, w rounded to the data's real type and the arithmetic in that type (contraction to FMA allowed):
 *   lo = b[k,l] + u (b[k+1,l] - b[k,l]);   hi = b[k,l+1] + u (b[k+1,l+1] - b[k,l+1]);   out = lo + v (hi - lo)
 * and for a volume the same in the sheet m + 1, then one lerp along e with w: seven lerps, along r, then a, then e.  OUTSIDE, out = fill (the reference: NaN;
 * pass the canonical quiet NaN); for complex output the real part is fill and the imaginary part 0 -- this library's decision.  Non-finite samples go through
 * the lerps by IEEE rules: a NaN corner gives NaN even under a zero weight.
 * PRE acts on the corner samples BEFORE the lerps -- the reference's scanConvert(scan, mod2db(b)), not mod2db of the result.  QDAS_SC_PRE_NONE: out has
 * the data's type; QDAS_SC_PRE_ABS: |b|; QDAS_SC_PRE_DB: 20 log10 |b|, and a value below db_floor becomes db_floor (-inf: the reference's behaviour, an exact zero
 * then gives -inf corners and IEEE results around them; a NaN stays a NaN).  With ABS and DB out is REAL, of the data's precision.
 * The axes are strictly increasing and need not be uniform (the caller's promise, not checked here: they are device vectors).  A workgroup keeps r, a, e in LDS
 * and finds out for itself whether an axis has a constant pitch (every node within a quarter of it of its place): then the cell is guessed in O(1) and corrected
 * against the nodes, otherwise it is bisected (QDAS_SCANCONVERT_BISECT=1 in the environment, read per call: always; tests).  Either way the cell is the one named
 * above on the actual vector.  One lane per output z, looping over the pages; every output element is written exactly once, no atomics: results are bit-reproducible.
 * STREAM.  The call is asynchronous on the hipStream_t in the descriptor's `queue` field (as qdas_refocus, and for its reason): no synchronisation, no
 * allocation, no work space of the library's.  All validation happens on the host before any HIP call: a null descriptor, R < 2, A < 2, E = 1, E = 0 with
 * Y != 0, E >= 2 with Y = 0, an unknown dtype / pre, cplx other than 0 | 1, a non-finite origin, a NaN db_floor, and -- for a call that has work -- a null
 * pointer is QDAS_EINVAL; Z X max(Y, 1) P = 0 is QDAS_OK, nothing is launched, the pointers may be NULL; R + A + E > 8192 (source axes beyond 64 KiB of LDS),
 * more than 2^31 - 1 workgroups (256 values of z each) or element counts beyond 2^60: QDAS_EUNSUPPORTED.  Half-precision images are not built. */
#define QDAS_SC_PRE_NONE 0
#define QDAS_SC_PRE_ABS  1
#define QDAS_SC_PRE_DB   2
typedef struct qdas_scanconvert_desc {
    uint64_t R, A, E;            /* source nodes; E = 0: polar, E >= 2: spherical            */
    uint64_t Z, X, Y;            /* output nodes; polar: Y = 0 (there is no y axis)           */
    uint64_t P;                  /* pages                                                      */
    int64_t  sr, sa, se, sp;     /* SOURCE strides in elements (the DAS view is read in place) */
    int32_t  dtype, cplx, pre, device;   /* QDAS_F32 | QDAS_F64; 0 | 1; QDAS_SC_PRE_*; -1 = current */
    double   origin[3], fill, db_floor;
    const double *r, *a, *e, *x, *y, *z; /* DEVICE; angles in radians, strictly increasing: the caller's promise */
    void    *queue;              /* a hipStream_t                                              */
} qdas_scanconvert_desc;
int qdas_scanconvert(const qdas_scanconvert_desc *d, const void *b, void *out);  /* out: dense, Z fastest, then X, [Y], pages */

/* ---- Demodulation (demod.hip): the reference's recipe for baseband imaging, downmix(chd, fc) -> filter(chd, D) -> downsample(chd, ratio)
 * (src/ChannelData.m:757-807, :857-888, :1042-1058), in ONE pass over the record.  For x of T samples x C traces (time contiguous, trace c at x + c x_ld), real
 * taps b[0 .. K-1], an integer ratio R >= 1 and J = ceil(T / R) = qdas_demod_len(T, R):
 *   out[j + c out_ld] = sum_{k=0}^{K-1} b[k] x[jR - k, c] exp(-2 pi i frac(fc (t0_c + (jR - k) / fs))),   j = 0 .. J-1,
 * terms with jR - k < 0 omitted (the causal start of `filter`).  The new time axis is t0' = t0 - (K - 1) / 2 / fs, fs' = fs / R -- the caller's bookkeeping;
 * the phase uses the ORIGINAL t0, as the composition does.  For real x the result carries half the analytic amplitude, exactly as the composition does
 * (taps 2 b restore it); there is no gain field.  The kernel evaluates
 *   out[j] = exp(-2 pi i frac(cyc0_c + frac(j step))) sum_k (b[k] exp(+2 pi i frac(k fc_over_fs))) x[jR - k],   fc_over_fs = fc / fs,  step = fc R / fs,
 * with the three frac() in float64, sincos and the sums in the data's precision (fp32 accumulators for int16 / float32 / complex64 input, fp64 for double
 * data), one rounding at the store.  cyc0: DEVICE vector of G >= 1 doubles, frac(fc t0) per start time; trace c uses cyc0[(c / gdiv) % G] (gdiv = N, G = M: one
 * start time per transmit of a T x N x M record; G = 1: one for all).
 * TYPES.  in_type QDAS_DEMOD_I16 | _F32 | _C64: out is complex64, or with out_half interleaved half pairs (what qdas_DASh takes); b is float32.
 * QDAS_DEMOD_F64 | _C128: out is complex128, b is float64; out_half is refused.  b: DEVICE vector of K real taps.
 * A sample no output reads (K < R: indices with (-i) mod R >= K) is never loaded, and no sample is multiplied by a zero coefficient: a NaN at x[i] reaches
 * exactly the outputs with 0 <= jR - i < K.  Every output element is written exactly once, out_ld padding is not touched, no atomics: bit-reproducible.
 * STREAM.  Asynchronous on the hipStream_t in the descriptor's `queue` field (as qdas_scanconvert): no synchronisation, no allocation, no work space.
 * All validation happens on the host before any HIP call: a null descriptor, R = 0, K = 0, x_ld < T, out_ld < J, an unknown in_type, out_half other than
 * 0 | 1 or with double data, G = 0, gdiv = 0, a non-finite fc_over_fs / step and -- for a call that has work -- a null x, b, out or cyc0: QDAS_EINVAL.
 * T C = 0: QDAS_OK, nothing is launched, the pointers may be NULL.  LIMITS: K <= QDAS_DEMOD_MAX_K = 1024 taps and R <= QDAS_DEMOD_MAX_R = 4096 (the modulated
 * taps and the span of one tile live in at most 64 KiB of LDS), C ceil(J / QDAS_DEMOD_TILE) < 2^31 workgroups, T, C, x_ld, out_ld < 2^40: QDAS_EUNSUPPORTED beyond. */
#define QDAS_DEMOD_I16  0
#define QDAS_DEMOD_F32  1
#define QDAS_DEMOD_C64  2
#define QDAS_DEMOD_F64  3
#define QDAS_DEMOD_C128 4
#define QDAS_DEMOD_MAX_K 1024
#define QDAS_DEMOD_MAX_R 4096
#define QDAS_DEMOD_TILE  256    /* outputs of one trace per workgroup */
typedef struct qdas_demod_desc {
    uint64_t T, C, K, R;         /* samples per trace, traces, taps, decimation ratio           */
    uint64_t x_ld, out_ld;       /* trace strides in elements (x_ld >= T, out_ld >= J)          */
    int32_t  in_type, out_half;  /* QDAS_DEMOD_*; 0 | 1                                         */
    int32_t  device, reserved;   /* HIP ordinal, -1 = current                                   */
    double   fc_over_fs, step;   /* fc / fs; fc R / fs  (cycles per input / per output sample)  */
    const double *cyc0;          /* DEVICE, G values of frac(fc t0)                             */
    uint64_t gdiv, G;            /* trace c uses cyc0[(c / gdiv) % G]                           */
    void    *queue;              /* a hipStream_t                                               */
} qdas_demod_desc;
uint64_t qdas_demod_len(uint64_t T, uint64_t R);   /* J = ceil(T / R); 0 for R = 0 */
int qdas_demod(const qdas_demod_desc *d, const void *x, const void *b, void *out);

/* ---- Rational-rate polyphase FIR (resample.hip): the reference's resample, filtfilt and the FIR part of its time-axis DSP (src/ChannelData.m:1059-1094,
 * :890-909) as ONE formula.  For x of T samples x C traces (time contiguous, trace c at x + c x_ld), real taps h[0 .. K-1], integers p, q >= 1 (they need not
 * be coprime), an offset off >= 0 and an output count J:
 *   out[j + c out_ld] = sum_i h[off + j q - i p] X_c[i],   j = 0 .. J-1,   over every integer i with 0 <= off + j q - i p < K.
 * X[i] = x[i] for 0 <= i < T.  Outside the record edge = QDAS_RESAMPLE_ZERO gives X[i] = 0; edge = QDAS_RESAMPLE_ODD gives the odd reflection
 * X[-i] = 2 x[0] - x[i], X[T-1+i] = 2 x[T-1] - x[T-1-i], and the call is refused (QDAS_EINVAL) unless every index an output reads lies in [-(T-1), 2(T-1)].
 *   upfirdn(h, x, p, q):  off = 0, J = qdas_upfirdn_len(T, K, p, q) = ceil(((T-1) p + K) / q)            (scipy.signal.upfirdn)
 *   resample(x, p, q):    K odd, off = (K-1)/2, J = qdas_resample_len(T, p, q) = ceil(T p / q), ZERO      (MATLAB's uniform syntax, scipy's resample_poly)
 *   filtfilt(b, x):       p = q = 1, h = b * flip(b) (2 K_b - 1 taps), off = K_b - 1, J = T, ODD           (MATLAB's and scipy's filtfilt for an FIR b)
 *   a plain FIR at any integer offset: p = q = 1.
 * TYPES.  in_type QDAS_RESAMPLE_I16 | _F32 | _C64: fp32 products and sums, h is float32, out is float32 (I16, F32: int16 is widened while staging) or complex64.
 * QDAS_RESAMPLE_F64 | _C128: fp64, h is float64, out is float64 or complex128.  h: DEVICE vector of K real taps.  One accumulator per output, taps of a phase
 * in ascending order, no rounding but the FMAs' (and the one of a reflected sample).
 * A sample no output reads is never multiplied, and no sample meets a zero coefficient: a NaN at x[i] reaches exactly the outputs with
 * 0 <= off + j q - i p < K.  Every output element is written exactly once, out_ld padding is not touched, no atomics, no work space: bit-reproducible.
 * `queue` is a hipStream_t; the call is asynchronous on it and synchronises nothing.
 * All validation happens on the host before any HIP call: a null descriptor, an unknown in_type or edge, p = 0, q = 0, K = 0, x_ld < T, out_ld < J, and -- for
 * a call that has work -- T = 0, a null x, h or out, and the ODD reach rule: QDAS_EINVAL.  J C = 0: QDAS_OK, nothing is launched, the pointers may be NULL.
 * LIMITS: K <= QDAS_RESAMPLE_MAX_K = 8192, p, q <= QDAS_RESAMPLE_MAX_PQ = 4096; the K taps and the span of one output ((K-1)/p + 1 samples) within 64 KiB of
 * LDS -- every K <= 2730 fits in every type at every p, more with p >= 2 or narrower data (int16 and float32: K = 8192 at every p); a workgroup
 * takes the largest power of two of outputs, 1024 at most, whose span ceil((TJ-1) q / p) + (K-1)/p + 1 fits beside the taps (40 KiB down to 64 outputs, 64 KiB
 * below); C ceil(J / TJ) < 2^31; T, C, J, off, x_ld, out_ld < 2^40: QDAS_EUNSUPPORTED beyond. */
#define QDAS_RESAMPLE_I16  0
#define QDAS_RESAMPLE_F32  1
#define QDAS_RESAMPLE_C64  2
#define QDAS_RESAMPLE_F64  3
#define QDAS_RESAMPLE_C128 4
#define QDAS_RESAMPLE_ZERO 0
#define QDAS_RESAMPLE_ODD  1
#define QDAS_RESAMPLE_MAX_K  8192
#define QDAS_RESAMPLE_MAX_PQ 4096
typedef struct qdas_resample_desc {
    uint64_t T, C, K, J;         /* samples per trace, traces, taps, outputs per trace          */
    uint64_t p, q, off;          /* up, down, tap offset of output 0                            */
    uint64_t x_ld, out_ld;       /* trace strides in elements (x_ld >= T, out_ld >= J)          */
    int32_t  in_type, edge;      /* QDAS_RESAMPLE_I16 .. _C128; QDAS_RESAMPLE_ZERO | _ODD       */
    int32_t  device, reserved;   /* HIP ordinal, -1 = current                                   */
    void    *queue;              /* a hipStream_t                                               */
} qdas_resample_desc;
uint64_t qdas_resample_len(uint64_t T, uint64_t p, uint64_t q);              /* ceil(T p / q); 0 for q = 0            */
uint64_t qdas_upfirdn_len(uint64_t T, uint64_t K, uint64_t p, uint64_t q);   /* ceil(((T-1) p + K) / q); 0 for q T = 0 */
int qdas_resample(const qdas_resample_desc *d, const void *x, const void *h, void *out);

/* ---- 2-D acoustic FDTD (fdtd.hip): a linear, lossless, first-order solver on a staggered grid, the part the reference delegates to external solvers
 * (src/UltrasoundSystem.m:2458-3170 kspaceFirstOrder, :1042-1460 fullwaveSim).  FDTD of order 2R in space, NOT k-space pseudospectral.  Nz x Nx nodes (the
 * PML included), z fastest, spacing h in both directions, V pulses stepped together.  p, rz, rx at (i, j); uz at (i + 1/2, j), ux at (i, j + 1/2).
 *   D+f[i] = (1/h) sum_{k=1..R} a_k (f[i+k] - f[i-k+1])  (at i + 1/2),   D-g[i] = (1/h) sum_{k=1..R} a_k (g[i+k-1] - g[i-k])  (at i),
 * anything outside the array reads as 0; a = (1), (9/8, -1/24), (1225/1024, -245/3072, 49/5120, -5/7168) for R = 1, 2, 4.  One step n = 0 .. Nt-1:
 *   1. uz <- azs (azs uz - (dtrz / h) h D+z p),   ux <- axs (axs ux - (dtrx / h) h D+x p)         dtrz = dt / rho_sgz, dtrx = dt / rho_sgx
 *   2. uz[src m] += src_wz[m] s[n, m, v],  ux[src m] += src_wx[m] s[n, m, v]   for n < Ts           src_wz = nz 2 c[src] dt / h (additive velocity source)
 *   3. rz <- az (az rz - (dt / h) rho h D-z uz),  rx <- ax (ax rx - (dt / h) rho h D-x ux)
 *   4. p = c2 (rz + rx)
 *   5. rec[n rec_st + j rec_sn + v rec_sv] = p[sensor j]
 * az, azs (Nz) and ax, axs (Nx) are the PML factors exp(-alpha dt / 2) at the nodes and at the staggered points, 1 inside.
 * MEMORY.  The caller owns every byte; every pointer of qdas_fdtd_args is a DEVICE pointer.  States: element (i, j) of pulse v at v vstride + j ld + i
 * (ld >= Nz, vstride >= Nx ld); the padding is not touched.  The medium maps are Nx x Nz dense.  s is Ts x M x V (pulse fastest).  src_node / sen_node hold
 * j Nz + i; src_start / src_list and sen_start / sen_list are the per-tile lists qdas_fdtd_tile_lists makes on the host (a workgroup owns a tile of
 * QDAS_FDTD_TZ x QDAS_FDTD_TX nodes and injects and records the points inside it behind its own update: two launches per step, no atomics, no flags;
 * points must sit on distinct nodes).  The entry allocates nothing, synchronises nothing, captures no graph: it enqueues 2 Nt launches on `queue`
 * (a hipStream_t).  Two runs give the same bits; pulses never mix (a NaN in pulse v stays there).
 * dtype QDAS_F32 | QDAS_F64 (every array of that type); order = 2R in {2, 4, 8}.
 * All validation happens on the host before any HIP call: a null descriptor or argument block, a dtype other than QDAS_F32 / QDAS_F64, Nz = 0 or Nx = 0,
 * ld < Nz, vstride < Nx ld, dt_h or inv_h not finite and positive, and -- for a call that has work -- a null state, medium or PML pointer, M > 0 and Ts > 0
 * with a null source pointer, N > 0 with a null sensor pointer, unknown flags: QDAS_EINVAL.  An order other than 2, 4, 8, Nz or Nx >= 2^31, ld >= 2^40,
 * Nz Nx >= 2^31, V > 65535, M or N >= 2^31, Nt, Ts or a stride >= 2^40: QDAS_EUNSUPPORTED.  Nt = 0 or V = 0: QDAS_OK, nothing is launched, the pointers may
 * be NULL.
 * flags: QDAS_FDTD_ZERO -- the entry clears the Nz x Nx x V elements of each state array (not the padding) on `queue` before the first step: a start from
 * rest for a caller without a device fill of its own (the MEX gateway). */
#define QDAS_FDTD_TZ 64
#define QDAS_FDTD_TX 16
#define QDAS_FDTD_ZERO 1
typedef struct qdas_fdtd_desc {
    uint64_t Nz, Nx, V, Nt;            /* nodes with the PML, pulses, steps                          */
    uint64_t ld, vstride;              /* state strides in elements: row (>= Nz), pulse (>= Nx ld)   */
    uint64_t M, Ts, N;                 /* sources, rows of the source table, sensors                 */
    uint64_t rec_st, rec_sn, rec_sv;   /* record strides in elements: step, sensor, pulse            */
    double   dt_h, inv_h;              /* dt / h and 1 / h                                           */
    int32_t  dtype, order;             /* QDAS_F32 | QDAS_F64; 2R: 2, 4 or 8                         */
    int32_t  device, flags;            /* HIP ordinal, -1 = current; 0 | QDAS_FDTD_ZERO              */
    void    *queue;                    /* a hipStream_t                                              */
} qdas_fdtd_desc;
typedef struct qdas_fdtd_args {
    void *p, *uz, *ux, *rz, *rx;                       /* states, V x Nx x Nz (strided), updated in place */
    const void *c2, *rho, *dtrz, *dtrx;                /* c^2, rho, dt / rho_sgz, dt / rho_sgx            */
    const void *az, *azs, *ax, *axs;                   /* PML factors                                     */
    const void *s, *src_wz, *src_wx;                   /* source table and per-source weights             */
    const int32_t *src_node, *src_start, *src_list;
    const int32_t *sen_node, *sen_start, *sen_list;
    void *rec;
} qdas_fdtd_args;
uint64_t qdas_fdtd_tiles(uint64_t Nz, uint64_t Nx);      /* ceil(Nz / TZ) ceil(Nx / TX)                                                      */
/* HOST helper: start[0 .. tiles] and list[0 .. n) from n HOST node indices; QDAS_EINVAL for a node outside the grid. Tile (tz, tx) is tx ceil(Nz / TZ) + tz. */
int qdas_fdtd_tile_lists(uint64_t Nz, uint64_t Nx, uint64_t n, const int32_t *node, int32_t *start, int32_t *list);
int qdas_fdtd(const qdas_fdtd_desc *d, const qdas_fdtd_args *a);

/* ---- qdas_fdtd with power-law absorption: the scheme, the descriptor, the argument block and every rule of qdas_fdtd, with step 4 replaced.  A relaxation
 * FDTD of the Fullwave kind (memory variables), NOT k-Wave's fractional Laplacian.  With rn = rz + rx after step 3:
 *   QDAS_FDTD_LOSS_RELAX  (1 <= y < 2, L = 1 .. 4 mechanisms):   e_l <- e_l + E[l] (rn - e_l),   p = c2 (rn + kap sum_l g[l] (rn - e_l))   (the updated e_l)
 *   QDAS_FDTD_LOSS_STOKES (y = 2, L = 0, no extra state):        p = c2 (rn + kap (rn - ro)),    ro = rz + rx before step 3
 * and p = c2 rn exactly where kap is 0.  kap is an Nx x Nz dense map like the medium's: 2 c a under relaxation (a in Np (rad/s)^-y m^-1), mud = 2 c a / dt
 * under Stokes.  E[l] = 1 - exp(-dt / tau_l); for small loss alpha(w) = (w / 2c) kap sum_l g[l] (-Im D_l(w)) with the update's own discrete response
 * D_l = 1 - E_l / (1 - (1 - E_l) e^{i w dt}) (qups_amd/fdtd.py relaxation_fit makes tau, E, g); Stokes gives a w^2 less the (w dt)^2 / 6 of its backward
 * difference.  The unrelaxed speed c sqrt(1 + kap sum g) is what the caller's time step must respect.
 * e holds the memory variables, in the states' type and layout: mechanism l of pulse v starts at (v L + l) vstride, rows of ld.  QDAS_FDTD_ZERO clears e too.
 * Still two launches per step (the velocity pass is qdas_fdtd's kernel), no atomics, two runs give the same bits, pulses never mix.
 * Validation, on the host before any HIP call: every row of qdas_fdtd, and a null loss block, an unknown mode, L > 4, L = 0 with RELAX or L > 0 with STOKES,
 * a g that is not finite or negative, an E outside (0, 1], and -- for a call that has work -- a null kap, or a null e with L > 0: QDAS_EINVAL.  Nt = 0 or
 * V = 0: QDAS_OK, nothing is launched. */
#define QDAS_FDTD_LOSS_STOKES 1
#define QDAS_FDTD_LOSS_RELAX 2
#define QDAS_FDTD_MAX_L 4
typedef struct qdas_fdtd_loss {
    int32_t mode, L;                   /* QDAS_FDTD_LOSS_STOKES (L = 0) | QDAS_FDTD_LOSS_RELAX (L = 1 .. 4) */
    double g[4], E[4];                 /* weights and 1 - exp(-dt / tau_l) of the mechanisms 0 .. L-1         */
    const void *kap;                   /* Nx x Nz: 2 c a (RELAX) or 2 c a / dt (STOKES)                        */
    void *e;                           /* V L arrays of the states' layout, updated in place                   */
} qdas_fdtd_loss;
int qdas_fdtd_lossy(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l);

/* ---- qdas_fdtd with nonlinear propagation (B/A), with or without absorption: k-Wave's nonlinear first-order equations on the staggered grid of qdas_fdtd.
 * Steps 1, 2 and 5 are qdas_fdtd's.  With ro = rz + rx before step 3 and rn = rz + rx after it:
 *   3'. r_a <- A_a (A_a r_a - (dt / h) (rho + K ro) h D-_a u_a)      a in {z, x};  K = 2 (the convective term), 0 with QDAS_FDTD_NL_NO_CONVECTIVE
 *   4'. p = c2 (rn + [the absorption term of qdas_fdtd_lossy, if l is given] + bq rn^2)
 * bq = BoA / (2 rho) is an Nx x Nz dense map like the medium's; a node with bq = 0 takes the linear value itself.  For a progressive plane wave this is
 * Westervelt's equation with beta = 1 + B/2A (the convective term alone: beta = 1, the quadratic term alone: beta = B/2A).  The source samples are particle
 * velocities in m/s (a line of additive sources s = v0 radiates rho c v0 each way): their absolute size matters here.  There is no shock capturing: without
 * absorption a wave that reaches the shock distance (sigma = 1) rings at the grid scale.
 * l = NULL: no absorption; otherwise the loss block of qdas_fdtd_lossy with all its rules.  With QDAS_FDTD_NL_NO_CONVECTIVE and an all-zero bq the entry
 * gives the bits of qdas_fdtd (l = NULL) and of qdas_fdtd_lossy (l given).  Still two launches per step (the velocity pass is qdas_fdtd's kernel), no
 * atomics, two runs give the same bits, pulses never mix.
 * Validation, on the host before any HIP call: every row of qdas_fdtd and, with l, of qdas_fdtd_lossy; a null nonlinear block, unknown flags in it, and --
 * for a call that has work -- a null bq: QDAS_EINVAL.  Nt = 0 or V = 0: QDAS_OK, nothing is launched. */
#define QDAS_FDTD_NL_NO_CONVECTIVE 1
typedef struct qdas_fdtd_nl {
    const void *bq;                    /* Nx x Nz: BoA / (2 rho)                                              */
    int32_t flags;                     /* 0 | QDAS_FDTD_NL_NO_CONVECTIVE                                      */
} qdas_fdtd_nl;
int qdas_fdtd_nonlinear(const qdas_fdtd_desc *d, const qdas_fdtd_args *a, const qdas_fdtd_loss *l /* NULL: lossless */, const qdas_fdtd_nl *q);

/* ---- 3-D acoustic FDTD (fdtd3.hip): the scheme of qdas_fdtd with a third axis -- linear, lossless, first order in time, of order 2R in space (R = 1, 2, 4)
 * on a staggered grid -- for channel data through volumes (the reference's kspaceFirstOrder picks kspaceFirstOrder3D for a grid of three dimensions,
 * src/UltrasoundSystem.m:2929-2948).  FDTD, NOT k-space pseudospectral.
 * GRID.  Nz x Nx x Ny nodes of spacing h in every direction, the P PML cells on all six faces included (the medium extended by edge replication); z is
 * fastest, then x, then y: node (k Nx + j) Nz + i, the memory order of a Scan.cartesian(x, z, y) grid ('ZXY').  V pulses are stepped together.
 * FIELDS.  p, rz, rx, ry at (i, j, k); uz at (i + 1/2, j, k), ux at (i, j + 1/2, k), uy at (i, j, k + 1/2).  The staggered density of an axis is the mean of
 * the two neighbours along it, the last one kept.  Along an axis, with anything outside the array read as 0,
 *   D+f[i] = (1/h) sum_{k=1..R} a_k (f[i+k] - f[i-k+1])  (at i + 1/2),   D-g[i] = (1/h) sum_{k=1..R} a_k (g[i+k-1] - g[i-k])  (at i),
 * a = (1), (9/8, -1/24), (1225/1024, -245/3072, 49/5120, -5/7168) for R = 1, 2, 4 (the sums run k = 1 .. R in this order).  One step n = 0 .. Nt-1:
 *   1. u_a <- A+_a (A+_a u_a - (dtr_a / h) h D+_a p)         for a in {z, x, y}; dtr_a = dt / rho_sg,a; A+_a = azs | axs | ays
 *   2. u_a[src m] += src_w_a[m] s[n, m, v]   for n < Ts        src_w_a = n_a 2 c[src] dt / h (additive velocity source along the normal (nz, nx, ny))
 *   3. r_a <- A_a (A_a r_a - (dt / h) rho h D-_a u_a)          A_a = az | ax | ay
 *   4. p = c2 ((rz + rx) + ry), in this order of addition
 *   5. rec[n rec_st + j rec_sn + v rec_sv] = p[sensor j]
 * The PML factors are A = exp(-alpha dt / 2), alpha = 2 (c_max / h) (xi / P)^4, xi the depth into the layer in cells, at the nodes (A) and at the staggered
 * points (A+), 1 inside.  Every table is made in float64 on the host and rounded once to `dtype`.
 * STABILITY.  c_max dt / h <= 1 / (sqrt(3) sum|a_k|) = 0.5774, 0.4949, 0.4488 for R = 1, 2, 4 (the callers check; the entry does not know c_max).
 * MEMORY.  The caller owns every byte; every pointer of qdas_fdtd3_args is a DEVICE pointer.  States: element (i, j, k) of pulse v at
 * v vstride + k pstride + j ld + i (ld >= Nz, pstride >= Nx ld, vstride >= Ny pstride); the padding is not touched.  The medium maps are Ny x Nx x Nz dense.
 * s is Ts x M x V (pulse fastest).  src_node / sen_node hold (k Nx + j) Nz + i; src_start / src_list and sen_start / sen_list are the per-brick lists
 * qdas_fdtd3_brick_lists makes on the host.  A workgroup owns a brick of QDAS_FDTD3_TZ x QDAS_FDTD3_TX x QDAS_FDTD3_TY nodes of one pulse, marches through it
 * along y, and injects and records the points inside it behind its own update: two launches per step, no atomics, no flags; points must sit on distinct
 * nodes.  The entry allocates nothing, uses no work space, synchronises nothing, captures no graph: it enqueues 2 Nt launches on `queue` (a hipStream_t).
 * Two runs give the same bits; pulses never mix (a NaN in pulse v stays there).
 * dtype QDAS_F32 | QDAS_F64 (every array of that type); order = 2R in {2, 4, 8}.
 * All validation happens on the host before any HIP call: a null descriptor or argument block, a dtype other than QDAS_F32 / QDAS_F64, an extent of 0,
 * ld < Nz, pstride < Nx ld, vstride < Ny pstride, dt_h or inv_h not finite and positive, unknown flags, and -- for a call that has work -- a null state,
 * medium or PML pointer, M > 0 and Ts > 0 with a null source pointer, N > 0 with a null sensor pointer: QDAS_EINVAL.  An order other than 2, 4, 8, an extent
 * >= 2^31, Nz Nx Ny >= 2^31 (node indices are int32), ld >= 2^40, pstride >= 2^44, vstride >= 2^46, V > 65535, M or N >= 2^31, Nt, Ts or a record stride
 * >= 2^40: QDAS_EUNSUPPORTED.  Nt = 0 or V = 0: QDAS_OK, nothing is launched, the pointers may be NULL.
 * flags: QDAS_FDTD3_ZERO -- the entry clears the Nz x Nx x Ny x V elements of each state array (not the padding) on `queue` before the first step. */
#define QDAS_FDTD3_TZ 64
#define QDAS_FDTD3_TX 8
#define QDAS_FDTD3_TY 8
#define QDAS_FDTD3_ZERO 1
typedef struct qdas_fdtd3_desc {
    uint64_t Nz, Nx, Ny, V, Nt;        /* nodes with the PML, pulses, steps                                            */
    uint64_t ld, pstride, vstride;     /* state strides in elements: row (>= Nz), plane (>= Nx ld), pulse (>= Ny pstride) */
    uint64_t M, Ts, N;                 /* sources, rows of the source table, sensors                                   */
    uint64_t rec_st, rec_sn, rec_sv;   /* record strides in elements: step, sensor, pulse                              */
    double   dt_h, inv_h;              /* dt / h and 1 / h                                                             */
    int32_t  dtype, order;             /* QDAS_F32 | QDAS_F64; 2R: 2, 4 or 8                                           */
    int32_t  device, flags;            /* HIP ordinal, -1 = current; 0 | QDAS_FDTD3_ZERO                               */
    void    *queue;                    /* a hipStream_t                                                                */
} qdas_fdtd3_desc;
typedef struct qdas_fdtd3_args {
    void *p, *uz, *ux, *uy, *rz, *rx, *ry;             /* states, V x Ny x Nx x Nz (strided), updated in place */
    const void *c2, *rho, *dtrz, *dtrx, *dtry;         /* c^2, rho, dt / rho_sg of the three axes              */
    const void *az, *azs, *ax, *axs, *ay, *ays;        /* PML factors                                          */
    const void *s, *src_wz, *src_wx, *src_wy;          /* source table and per-source weights                  */
    const int32_t *src_node, *src_start, *src_list;
    const int32_t *sen_node, *sen_start, *sen_list;
    void *rec;
} qdas_fdtd3_args;
uint64_t qdas_fdtd3_bricks(uint64_t Nz, uint64_t Nx, uint64_t Ny);   /* ceil(Nz / TZ) ceil(Nx / TX) ceil(Ny / TY)                                       */
/* HOST helper: start[0 .. bricks] and list[0 .. n) from n HOST node indices; QDAS_EINVAL for a node outside the grid.  Brick (bz, bx, by) is
 * (by ceil(Nx / TX) + bx) ceil(Nz / TZ) + bz. */
int qdas_fdtd3_brick_lists(uint64_t Nz, uint64_t Nx, uint64_t Ny, uint64_t n, const int32_t *node, int32_t *start, int32_t *list);
int qdas_fdtd3(const qdas_fdtd3_desc *d, const qdas_fdtd3_args *a);

/* ---- Pair-wise windowed zero-normalized cross-correlation (pwznxcorr.hip): the base-MATLAB branch of the reference's kern/pwznxcorr.m (iflt = false:
 * convn(., w, 'same'), a zero pad at the end of the record, circshift) for every lag in ONE launch.  With h = floor(W / 2), P = max|lags| when `pad` (else 0),
 * Tp = T + P, both records extended by P zeros, K(a)[s] = sum_k w[k] a[s + h - k] for s in [0, Tp) and a = 0 outside [0, Tp) (MATLAB's 'same'):
 *   xlz = xl - K(xl) when `zero`, else xl;                xln = K(|xlz|^2)
 *   per lag l:  c[s] = conj(xr[(s + l) mod Tp]);          cz = c - K(c) when `zero`, else c
 *   y_l = K(xlz cz),  with `norm` divided by sqrt(xln) sqrt(K(|cz|^2)) (0 / 0 stays NaN);     the result is y_l[0 .. T-1].
 * `zero` subtracts the weighted window SUM as the reference does (weights ones(W) / W give the usual ZNCC); in the pad region xlz is -K(xl), not 0, and
 * for a positive lag the first l samples wrap into the pad region: both are reproduced.
 * xl, xr: DEVICE arrays of `dtype` (QDAS_F64 | QDAS_F32), real or interleaved complex, of N channel pairs x bsize[0] x bsize[1] records of T samples, the
 * samples of a record contiguous (stride 1); the other strides count elements (complex samples when cplx) and are given per operand -- xr may be xl
 * shifted by a channel stride (neighbouring channels) or broadcast one record with a stride of 0.  w: DEVICE array of W real `dtype` weights; with `norm`
 * they must not be negative (the reference's denominator turns complex; the caller checks).  lags: HOST table of nlags integers, in any order, duplicates
 * allowed, read during the call only.  y: DEVICE array of `dtype` (complex when cplx): y[t + n y_strideN + b0 y_bstride[0] + b1 y_bstride[1] + i y_strideL]
 * for lag i.  Every sum is a direct weighted sum over the window in the data's precision; no atomics: results are bit-reproducible.
 * A workgroup owns QDAS_PWZNXCORR_TIME_TILE output times of one record pair and keeps tile + 2 (W - 1) samples of the left and tile + 2 (W - 1) + (max lag -
 * min lag) samples of the right record in LDS (qdas_pwznxcorr_lds_bytes); beyond 64 KiB -- W = 256 with lags -256 .. 256 in complex double needs 53144
 * bytes and is inside --, more than QDAS_PWZNXCORR_MAX_LAGS lags, a lag beyond +-32767 or more than 2^31 - 1 workgroups: QDAS_EUNSUPPORTED, nothing is
 * launched.  The arguments are validated before any HIP call; T, N, a batch size or nlags = 0 is an empty result: nothing is launched, the data pointers may be NULL. */
#define QDAS_PWZNXCORR_TIME_TILE 256
#define QDAS_PWZNXCORR_MAX_LAGS  1024
typedef struct qdas_pwznxcorr_desc {
    int32_t  dtype;               /* QDAS_F64 | QDAS_F32                              */
    int32_t  cplx;                /* samples are interleaved complex                  */
    int32_t  device;              /* HIP device ordinal, -1 = current                 */
    int32_t  zero, norm, pad;     /* 0 | 1: the reference's options of the same names */
    uint64_t T;                   /* samples per record                               */
    uint64_t N;                   /* channel pairs                                    */
    uint64_t W;                   /* window length (>= 1)                             */
    uint64_t nlags;
    uint64_t bsize[2];            /* batch groups; unused: 1 (stride 0)               */
    int64_t  xl_strideN, xl_bstride[2];
    int64_t  xr_strideN, xr_bstride[2];
    int64_t  y_strideN, y_bstride[2], y_strideL;
} qdas_pwznxcorr_desc;
int qdas_pwznxcorr(const qdas_pwznxcorr_desc *desc, const void *xl, const void *xr, const void *w, const int64_t *lags, void *y, void *stream);
int qdas_pwznxcorr_time_tile(void);                                                   /* QDAS_PWZNXCORR_TIME_TILE of the library as built */
uint64_t qdas_pwznxcorr_lds_bytes(int dtype, int cplx, uint64_t W, uint64_t span);    /* LDS of one workgroup; span = max lag - min lag */

/* ---- Temporaries of the stream entries (qdas_shift_sum, qdas_das_lut, qdas_greens, qdas_convd's FFT path): taken from an arena the library keeps per (device,
 * stream).  One such call at a time runs per (device, stream) -- a second thread on the same stream waits --, and a call MAY BLOCK the host: when the stream's
 * previous call outgrew the arena (the next call waits for it, then regrows the arena to what that call needed, up to 512 MiB) or asks for a single temporary above
 * 64 MiB (freed, after a stream synchronisation, when the call returns).  Otherwise the calls only enqueue work.  qdas_device_trim releases idle arenas.
 * qdas_eikonal, qdas_adjoint and qdas_migration take their work space from the same arenas.  Two environment variables, both read per call:
 *   QDAS_SCRATCH_ARENA_MAX_MB=<n>   the 64 MiB above (0: every temporary is a block of its own, freed when its call returns);
 *   QDAS_SCRATCH_POISON=<0..255>    (tests; unset by default, then one getenv per temporary / plan allocation) every temporary is filled with this byte on
 *                                   the call's stream before the call uses it, and every device allocation a plan owns (misfit-tile list, partial images,
 *                                   fold buffers, staging) once, synchronously, when it is made: results must not depend on it. */

/* ---- Device staging for HOST callers of the device-pointer entries above (qdas_delays*, qdas_das_lut, qdas_wsinterpd, qdas_greens, qdas_convd,
 * qdas_pre_execute ...): the reference reaches those kernels with gpuArrays (kern/wsinterpd2.m:236, src/UltrasoundSystem.m:681-718, kern/convd.m:150-199),
 * a MEX gateway built WITHOUT the mxGPUArray API has host arrays only and must not need the HIP headers -- it allocates, copies and frees through
 * these three (mex/qdas_mex.c dev_in / dev_out).  device: HIP ordinal, -1 = current.  qdas_device_copy is synchronous; kind 0: host -> device,
 * 1: device -> host, 2: device -> device. */
int qdas_device_malloc(void **p, size_t bytes, int device);
int qdas_device_free(void *p, int device);      /* (buffers of qdas_device_malloc are kept for reuse, at most 4 GiB -- QDAS_STAGING_CACHE_MB --: a call-per-launch gateway does not map / unmap.
                                                 *  Like hipFree, qdas_device_free WAITS for the buffer's device -- every stream, blocking or not -- before the buffer can be handed
                                                 *  out again: work the caller launched on any stream may still be using it when it is freed.) */
int qdas_device_trim(void);                      /* ... and released here */
int qdas_device_copy(void *dst, const void *src, size_t bytes, int kind, int device);

/* ---- Layout conversion for row-major hosts (numpy / torch; no reference counterpart: MATLAB arrays are column-major already and
 * the ABI follows the reference's memory order, e.g. kern/das_spec.m:367-372 passes x(:,:,:,f) as it lies in memory).
 * out[c][b][a] = in[a][b][c] for a row-major A x B x C array of elem_bytes-sized elements (2 | 4 | 8 | 16): the column-major
 * image of T x N x M channel data or I1 x I2 x N delay tables.  Device pointers, in != out. */
int qdas_permute3(const void *in, void *out, uint64_t A, uint64_t B, uint64_t C, int elem_bytes, void *stream);

/* ---- Pre-processing in front of the DAS path: real RF traces -> analytic channel data, optionally downmixed.
 * Replaces ChannelData.hilbert (reference src/ChannelData.m:935-966: fft to N points along time, weights
 * [1; 2...; 1 + mod(N,2); 0...], ifft) and ChannelData.downmix (src/ChannelData.m:757-766: data .* exp(-2i*pi*fc*time))
 * applied after it -- one kernel, two real traces per complex transform, forward and inverse FFT stages LDS to LDS (pre.hip).
 * x: T x K real traces (K = N*M*F, device pointer) as fp32 or int16; y: Nfft x K complex64 (device).
 * Real input is half (fp32) / a quarter (int16) of the bytes of complex64 channel data on the PCIe link. */
#define QDAS_PRE_F32 0
#define QDAS_PRE_I16 1
typedef struct qdas_pre_desc {
    uint64_t T;        /* samples per input trace                                   */
    uint64_t K;        /* number of traces                                          */
    uint64_t Nfft;     /* transform length = output samples per trace (0 = T)       */
    int32_t  in_type;  /* QDAS_PRE_F32 | QDAS_PRE_I16                               */
    int32_t  device;   /* HIP device ordinal, -1 = current                          */
    double   fs, t0;   /* sampling frequency, time of sample 0 (downmix only)       */
    double   fdown;    /* downmix frequency [Hz]; 0 = no downmix                    */
} qdas_pre_desc;
typedef struct qdas_pre_plan qdas_pre_plan;
int  qdas_pre_plan_create(qdas_pre_plan **plan, const qdas_pre_desc *desc);
int  qdas_pre_execute(qdas_pre_plan *plan, const void *x, void *y, void *stream);
void qdas_pre_plan_destroy(qdas_pre_plan *plan);
/* 1: the plan runs the one-pass kernel (a trace pair resident in LDS: Nfft = 2^a 3^b 5^c 7^d 11^e 13^f <= 8192 whose stages fit 1024 threads; HBM sees the input once and
 * the output once); 0: hipFFT passes (any other length, or QDAS_PRE_HIPFFT=1 in the environment) */
int  qdas_pre_plan_one_pass(const qdas_pre_plan *plan);

/* ---- Variants of the fused kernel that are built on demand.  libqdas.so carries the instantiations the BASELINE configurations and frame streams
 * launch (csrc/das_tile_cfg.h TILE_PREBUILT); any other point of the template's matrix -- launch configuration `cfg` (das_tile_cfg.h) x interpolator
 * flag x remodulation x weight table -- is compiled by hiprtc when a plan first needs it (qdas_plan_create; ~2 s, then cached in memory and under
 * $QDAS_CACHE_DIR | ~/.cache/qdas), as the reference compiles its kernels per UltrasoundSystem (src/UltrasoundSystem.m:5527-5625).  This entry
 * builds one variant ahead of time (deployment, test sessions; `python -m qups_amd.warm` runs it over a list with one process per core).
 * Returns 0: built or already cached, 1: failed (qdas_last_error), 2: libqdas.so carries it, 3: no such variant.  Needs no device.
 * Without libhiprtc.so (or with QDAS_NO_LAZY=1) a plan that needs such a variant runs the generic kernel; qdas_last_error() after
 * qdas_plan_create says so, and a QDAS_KERNEL_TILED request fails with QDAS_EUNSUPPORTED. */
int  qdas_kernel_variant_build(int cfg, int interp, int fmod, int wtab);
/* 1: libqdas.so carries the variant, 0: it is built on demand, -1: no such variant */
int  qdas_kernel_variant_prebuilt(int cfg, int interp, int fmod, int wtab);

const char *qdas_last_error(void);
int  qdas_version(void);
/* device properties the host side reports next to measurements */
int  qdas_device_info(int device, char *name, size_t name_len, int *cu_count, int *clock_khz,
                      uint64_t *hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* QDAS_H */
