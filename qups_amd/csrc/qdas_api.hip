// qdas_api.hip -- the DAS plan of the C ABI of libqdas.so (see include/qdas.h for the contract and the reference call sites each
// entry replaces): validation, plan construction (device copies of geometry, folded apodization table, stride tables), kernel
// selection and launch, frame streaming, the one-shot qdas_DAS* / qdas_delays*.  Also the library's last-error string (api_util.h),
// version and device info.  Host-side only.  Every other one-shot entry sits below its kernels, in that kernel's file.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/qdas.h"
#include "api_util.h"
#include "qdas_kernels.h"
#include "jit.h"

using namespace qdas;

// ------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;

int qdas::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
const char *qdas::last_error() { return g_err.c_str(); }

extern "C" const char *qdas_last_error(void) { return g_err.c_str(); }
void qdas_internal_set_error(const char *msg) { g_err = msg ? msg : ""; }      // for the library's other translation units (api_util.h)
extern "C" int qdas_version(void) { return QDAS_VERSION; }

extern "C" int qdas_device_info(int device, char *name, size_t name_len, int *cu_count, int *clock_khz,
                                uint64_t *hbm_bytes) {
    if (device < 0) HIPCHK(hipGetDevice(&device));
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    if (name && name_len) { snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName); }
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    return QDAS_OK;
}

// ------------------------------------------------------------------------------------ plan
struct qdas_plan {
    qdas_desc d{};
    uint64_t I = 0, i_count = 0, y_ld = 0, oN = 1, oM = 1;
    double cinv0 = 0.0;                       // first entry of the sound-speed array (what `delays` uses, kern/das_spec.m:377)
    int device = 0;
    int kernel = QDAS_KERNEL_GENERIC;
    std::vector<void *> owned;                // device allocations made by the plan
    GenericParams gp{};
    TileParams tp{};
    TileConfig tc{};
    unsigned ntiles = 0, tile_cols = 0;
    bool no_fallback = false;                 // the probe found no tile whose delay spread exceeds the LDS window
    double misfit_frac = 0.0;                 // fraction of the chosen footprint's tiles that do not fit it
    bool wtab_real = false;                   // the folded weight table has no imaginary part
    // reciprocity fold (fold.hip; tile_params.h `fold`): the plan's folded copy of a frame (T x N x M complex64, upper triangle written per frame)
    // and the N x M weight table the fold pass applies (null: ones) -- the folded kernels themselves carry no table
    void *fold_buf = nullptr;
    const void *fold_wtab = nullptr;
    // tolerance mode (QDAS_PLAN_APPROX_SYMMETRY): bounds [samples] of the delay error the symmetry modes in use commit; 0 = exact symmetry, -1 = mode not in use
    double mirror_bound = -1.0, recip_bound = -1.0;
    bool prefolded = false;                   // QDAS_PLAN_PREFOLDED: execute is handed the folded frame (qdas_fold) -- no fold pass, no fold buffer
    // fp16 reciprocal data: the frame is folded into a complex64 copy (fold.hip, fp16 in) and beamformed by an fp32 PREFOLDED child plan into a complex64
    // image, which is rounded to the plan's complex32 output: the folded fp32 kernels serve fp16 data (C3 with fp16 data 23.7 -> 15 ms)
    qdas_plan *f16_child = nullptr;
    void *y32 = nullptr;
    bool fb2_ok = false;                      // frames of a sequence may share launches, 4 or 2 at a time (decided at plan creation)
    bool fb4_off = false;                     // ... but at most pairwise (QDAS_NO_FB4)
    bool fold2_ok = false;                    // folded data: two frames may share a launch
    void *fold_buf2 = nullptr;                // ... and the folded copy of the second one (made at the first stream of frames)
    // A lateral-mirror plan runs one frame per launch (its second window set is taken).  For a STREAM of frames four frames per launch share
    // more (index + weights of four traces instead of two): such plans keep a twin without the mirror mode, made at the first stream.
    qdas_plan *frames_twin = nullptr;
    bool twin_tried = false;
    uint32_t *fallback = nullptr;             // device: [0] = count, [1..ntiles]
    size_t jit_lds = 0;                       // dynamic LDS of the specialised kernel
    int jit_mb = 0, jit_w = 0;                // its transmits per stage, samples per window
    int hint_mb = 0, hint_w = 0;              // stage shape a plan-specialised build should take instead of the prebuilt configuration's (plan_stage_shape)
    hipFunction_t jit_fn = nullptr;           // plan-specialised kernel (QDAS_PLAN_JIT, jit.hip); null: prebuilt instantiation
    std::string jit_tag;                      // "jit <hash>" when the plan runs a hiprtc-specialised kernel (QDAS_PLAN_JIT)
    bool prep2 = false, prep4 = false;        // the two- / four-frame instantiations have been resolved (qdas_plan_execute_frames)
    bool timing = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float last_ms = 0.f;
    // host staging (mem == HOST)
    void *dx = nullptr, *dy = nullptr;
    size_t x_bytes = 0, y_bytes = 0;
    // second staging set + copy stream: frame f+1 is uploaded while frame f is beamformed (host-resident frame sequences)
    void *dx2 = nullptr, *dy2 = nullptr;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ex[2] = {nullptr, nullptr}, ek[2] = {nullptr, nullptr};

    ~qdas_plan() {
        if (frames_twin) qdas_plan_destroy(frames_twin);
        if (f16_child) qdas_plan_destroy(f16_child);
        for (void *p : owned) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        for (int k = 0; k < 2; ++k) { if (ex[k]) (void)hipEventDestroy(ex[k]); if (ek[k]) (void)hipEventDestroy(ek[k]); }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

// every device allocation of this file: hipMalloc, and -- QDAS_SCRATCH_POISON (csrc/scratch.hip scratch_poison: one getenv when unset) -- the block filled with
// that byte before anything else touches it, synchronously.  A buffer that is then wholly uploaded or cleared is unaffected; one that a kernel reads before the
// plan wrote it reads the poison instead of whatever hipMalloc handed back
static hipError_t plan_malloc(void **out, size_t bytes) {
    const hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) return e;
    const int poison = scratch_poison();
    if (poison < 0) return hipSuccess;
    const hipError_t m = hipMemset(*out, poison, bytes);
    if (m != hipSuccess) { (void)hipFree(*out); *out = nullptr; }
    return m;
}

static int dev_alloc(qdas_plan *pl, void **out, size_t bytes) {
    void *p = nullptr;
    hipError_t e = plan_malloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(QDAS_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    pl->owned.push_back(p);
    *out = p;
    return QDAS_OK;
}

// Product of the pixel-dependent apodization arrays of a plan, broadcast to one contiguous I1*I2*I3 x E array (E = N, M or 1) in the
// arrays' own element type: what the fused kernel indexes as [pixel + I * stage element].  (The reference multiplies the S arrays per
// pair in the data precision, src/bf.cu:118-120; here the pixel-dependent factors are multiplied once per plan, in fp32, rounded once.)
struct ApodFold {
    const void *base;
    uint64_t st[QDAS_MAX_APOD][5];      // per array: strides over I1, I2, I3, the element; offset (in elements of the array type)
    uint64_t I1, I2, I3, E;
    int ns;
};
template <class T, bool CPLX> __global__ void apod_fold_kernel(ApodFold f, T *out, uint64_t nel) {
    const uint64_t I = f.I1 * f.I2 * f.I3;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nel; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = q % I, e = q / I;
        const uint64_t i1 = i % f.I1, i2 = (i / f.I1) % f.I2, i3 = i / (f.I1 * f.I2);
        float wr = 1.f, wi = 0.f;
        for (int s = 0; s < f.ns; ++s) {
            const uint64_t k = f.st[s][4] + i1 * f.st[s][0] + i2 * f.st[s][1] + i3 * f.st[s][2] + e * f.st[s][3];
            if constexpr (CPLX) {
                const float ar = (float)((const T *)f.base)[2 * k], ai = (float)((const T *)f.base)[2 * k + 1];
                const float nr = wr * ar - wi * ai, ni = wr * ai + wi * ar;
                wr = nr; wi = ni;
            } else wr *= (float)((const T *)f.base)[k];
        }
        if constexpr (CPLX) { out[2 * q] = (T)wr; out[2 * q + 1] = (T)wi; }
        else out[q] = (T)wr;
    }
}

static inline hipError_t upload(void *dst, const void *src, size_t bytes) { return (hipError_t)qdas_internal_upload(dst, src, bytes); }

// device copy of a caller array (host -> new device buffer; device -> used in place, or -- QDAS_PLAN_COPY_INPUTS -- copied
// into a plan-owned buffer so that the plan outlives the caller's arrays)
static int import_array(qdas_plan *pl, const void *src, size_t bytes, int mem, const void **out) {
    const bool own = (pl->d.plan_flags & QDAS_PLAN_COPY_INPUTS) != 0;
    if ((mem == QDAS_MEM_DEVICE && !own) || bytes == 0 || !src) { *out = src; return QDAS_OK; }
    void *p;
    int rc = dev_alloc(pl, &p, bytes);
    if (rc) return rc;
    if (mem == QDAS_MEM_DEVICE) HIPCHK(hipMemcpy(p, src, bytes, hipMemcpyDeviceToDevice));
    else HIPCHK(upload(p, src, bytes));
    *out = p;
    return QDAS_OK;
}

// host copy of (part of) a caller array
static int fetch_host(const void *src, size_t bytes, int mem, void *dst) {
    if (mem == QDAS_MEM_DEVICE) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    else memcpy(dst, src, bytes);
    return QDAS_OK;
}

// Largest pixel pitch [m] along I1 (3 sampled columns) and across columns (3 sampled rows) of the scan: the inputs of the
// tiled kernel's shape model (choose_tile_shape below).
static int scan_pitch(const qdas_desc *desc, double *gz_out, double *gc_out) {
    const qdas_sizes &z = desc->sz;
    const uint64_t ncols = z.I2 * z.I3;
    const size_t rs = z.dtype == QDAS_F64 ? 8 : 4, ps = 3 * rs;          // bytes per coordinate / per pixel position (real(prec))
    const unsigned char *Pi = (const unsigned char *)desc->Pi;
    double gz = 0.0, gc = 0.0;
    std::vector<unsigned char> buf;
    auto dist = [&](uint64_t i, uint64_t j) {                             // distance between pixels i and j of buf
        double d[3];
        for (int k = 0; k < 3; ++k)
            d[k] = rs == 8 ? ((const double *)buf.data())[3 * i + k] - ((const double *)buf.data())[3 * j + k]
                           : (double)((const float *)buf.data())[3 * i + k] - (double)((const float *)buf.data())[3 * j + k];
        return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    };
    if (z.I1 > 1) {
        buf.resize(ps * z.I1);
        const uint64_t cs[3] = {0, ncols / 2, ncols - 1};
        for (int k = 0; k < 3; ++k) {
            int rc = fetch_host(Pi + ps * z.I1 * cs[k], ps * z.I1, desc->mem, buf.data());
            if (rc) return rc;
            for (uint64_t i = 0; i + 1 < z.I1; ++i) { const double d = dist(i, i + 1); if (d > gz) gz = d; }
        }
    }
    if (z.I2 > 1) {
        buf.resize(ps * ncols);
        const uint64_t rws[3] = {0, z.I1 / 2, z.I1 - 1};
        for (int k = 0; k < 3; ++k) {
            if (desc->mem == QDAS_MEM_DEVICE)
                HIPCHK(hipMemcpy2D(buf.data(), ps, Pi + ps * rws[k], ps * z.I1, ps, ncols, hipMemcpyDeviceToHost));
            else
                for (uint64_t c = 0; c < ncols; ++c) memcpy(&buf[ps * c], Pi + ps * (rws[k] + z.I1 * c), ps);
            for (uint64_t c = 0; c + 1 < ncols; ++c) {
                if ((c + 1) % z.I2 == 0) continue;         // slice boundary of a 3-D scan
                const double d = dist(c, c + 1);
                if (d > gc) gc = d;
            }
        }
    }
    *gz_out = (gz == gz) ? gz : 0.0;                     // NaN pixels: no information
    *gc_out = (gc == gc) ? gc : 0.0;
    return QDAS_OK;
}

static float half_to_float(uint16_t h) {
    const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m + 1024), (int)e - 25);
    return s ? -v : v;
}

static int validate(const qdas_desc *d) {
    const qdas_sizes &z = d->sz;
    if (z.dtype < QDAS_F64 || z.dtype > QDAS_F16) return fail(QDAS_EINVAL, "Unrecognized input precision %d", z.dtype);
    const int interp = z.flag & QDAS_FLAG_INTERP_MASK;
    if (interp > 5) return fail(QDAS_EINVAL, "QUPS:das_spec:UnrecognizedInput: Unrecognized interpolation flag %d: must be one of "
                                "{'nearest', 'linear', 'cubic', 'lanczos3'}.", interp);
    if (z.flag & ~63) return fail(QDAS_EINVAL, "Invalid beamformer flag 0x%x.", z.flag);
    if (z.S > QDAS_MAX_APOD) return fail(QDAS_EUNSUPPORTED, "at most %d apodization arrays are supported (got %llu)", QDAS_MAX_APOD,
                                         (unsigned long long)z.S);
    if (!(d->fs > 0.0) || !std::isfinite(d->fs)) return fail(QDAS_EINVAL, "Undefined sampling rate.");
    if (!std::isfinite(d->fmod)) return fail(QDAS_EINVAL, "modulation frequency must be finite");
    const uint64_t I = z.I1 * z.I2 * z.I3;
    if (d->i_begin > I || (d->i_count && d->i_begin + d->i_count > I))
        return fail(QDAS_EINVAL, "pixel shard [%llu, +%llu) exceeds the image (%llu pixels)", (unsigned long long)d->i_begin,
                    (unsigned long long)d->i_count, (unsigned long long)I);
    if (I && z.N && z.M) {
        if (!d->Pi || !d->Pr || !d->Pv || !d->Nv || !d->cinv || !d->acstride) return fail(QDAS_EINVAL, "null geometry / stride pointer");
        if (z.S && !d->apod) return fail(QDAS_EINVAL, "S > 0 but apod is null");
        if (d->rx_apod_kind < QDAS_RXAPOD_NONE || d->rx_apod_kind > QDAS_RXAPOD_FNUMBER_ORIENTED)
            return fail(QDAS_EINVAL, "Unrecognized generated receive apodization %d", d->rx_apod_kind);
        if ((d->rx_apod_kind == QDAS_RXAPOD_ACCEPTANCE || d->rx_apod_kind == QDAS_RXAPOD_COSINE || d->rx_apod_kind == QDAS_RXAPOD_FNUMBER_ORIENTED)
            && !d->rx_normals) return fail(QDAS_EINVAL, "generated receive apodization needs the element normals (rx_normals)");
        if (d->rx_apod_kind && !(d->rx_apod_p[0] == d->rx_apod_p[0])) return fail(QDAS_EINVAL, "generated receive apodization: NaN parameter");
    }
    if (d->mem != QDAS_MEM_HOST && d->mem != QDAS_MEM_DEVICE) return fail(QDAS_EINVAL, "bad mem kind %d", d->mem);
    if (z.T > 0x7fffffffull) return fail(QDAS_EUNSUPPORTED, "T must be < 2^31");
    return QDAS_OK;
}

// size (elements) of a broadcastable I1xI2xI3xNxM array from its stride row
static uint64_t bcast_numel(const uint64_t *st, const qdas_sizes &z) {
    const uint64_t dims[5] = {z.I1, z.I2, z.I3, z.N, z.M};
    uint64_t n = 1;
    for (int k = 0; k < 5; ++k) if (st[k]) n += (dims[k] - 1) * st[k];
    return n;
}

// Shape of the tiled kernel's tiles and waves (das_tile_impl.h).
//  * tile footprint (64x16, 32x32, 16x64 or 8x128 pixels of I1 x columns): every candidate is PROBED -- the kernel's own
//    prologue runs for all tiles and counts those whose delay spread does not fit the LDS window; only footprints with the
//    fewest misfits are considered (a misfit tile is redone by the generic kernel at >10x the cost).
//  * wave footprint inside the tile (2^w x 2^(6-w) pixels): an LDS access group is 32 lanes; it is conflict-free when the
//    lanes read <= 32 consecutive samples, i.e. (group depth) x (delay samples per pixel of depth) + (group columns) x
//    (lateral gradient) <= 32.  The shallowest-needed wave wins; ties go to the deeper wave (longer store runs).
// QDAS_TILE_Z / QDAS_WAVE_Z override the choice (profiling, tests).
template <typename F>
static int choose_tile_shape(qdas_plan *pl, const qdas_desc *desc, F &&set_grid) {
    TileParams &t = pl->tp;
    const qdas_sizes &z = desc->sz;
    auto lg = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
    int env_tz = 0, env_wz = 0;
    if (const char *e = getenv("QDAS_TILE_Z")) { const int v = atoi(e); if (v == 8 || v == 16 || v == 32 || v == 64) env_tz = v; }
    if (const char *e = getenv("QDAS_WAVE_Z")) { const int v = atoi(e); if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) env_wz = v; }
    double gz = 0.0, gc = 0.0;
    int rc = scan_pitch(desc, &gz, &gc);
    if (rc) return rc;
    const double per = 2.0 * std::fabs(t.cinv_fs);      // delay samples per metre of pixel pitch (both legs)
    const double spz = per * gz, spc = 0.35 * per * gc;  // per pixel of depth / per column (obliquity-weighted)
    // misfit count of each footprint
    double fbn[7] = {0, 0, 0, 0, 0, 0, 0}, best_fb = 2.0;   // misfit FRACTION of the footprint's tiles
    for (int l = 6; l >= 3; --l) {
        if (env_tz && (1 << l) != env_tz) continue;
        set_grid(l);
        TileParams p = t;
        p.probe = 1; p.wz_log2 = l; p.x = nullptr; p.y = nullptr; p.wtab = nullptr; p.apix = nullptr;
        HIPCHK(hipMemset(pl->fallback, 0, sizeof(uint32_t)));
        HIPCHK(launch_tile(p, z.dtype, pl->ntiles, nullptr));
        uint32_t cnt = 0;
        HIPCHK(hipMemcpy(&cnt, pl->fallback, sizeof(uint32_t), hipMemcpyDeviceToHost));
        fbn[l] = (double)cnt / (double)(pl->ntiles ? pl->ntiles : 1);
        if (fbn[l] < best_fb) best_fb = fbn[l];
    }
    int best_t = -1, best_w = -1;
    double best_c = 1e300;
    for (int l = 6; l >= 3; --l) {
        if (env_tz && (1 << l) != env_tz) continue;
        if (fbn[l] > best_fb + 1e-9) continue;
        for (int w = l; w >= 2 && w >= l - 4; --w) {
            if (env_wz && (1 << w) != env_wz && !(env_wz > (1 << l) && w == l)) continue;
            const int gd = w >= 5 ? 32 : (1 << w), gcn = 32 / gd;     // depth x columns of one 32-lane access group
            const double span = gd * spz + gcn * spc;
            const double c = span <= 32.0 ? 1.0 : span / 32.0;
            if (c < best_c - 1e-9) { best_c = c; best_t = l; best_w = w; }
        }
    }
    if (best_t < 0) { best_t = env_tz ? lg(env_tz) : 6; best_w = best_t; }
    // the window fit depends on the geometry only: a footprint without misfits never needs the per-frame fallback pass
    pl->no_fallback = fbn[best_t] == 0.0;
    pl->misfit_frac = fbn[best_t];
    HIPCHK(hipMemset(pl->fallback, 0, sizeof(uint32_t)));
    set_grid(best_t);
    t.wz_log2 = best_w;
    t.probe = 0;
    return QDAS_OK;
}

// Lateral-mirror symmetry (tile_params.h `mir`): is pixel column I2-1-c the mirror image (x -> -x) of column c, bit for bit?  `dev`: the largest
// distance |mirror(p') - p| over the pixels, as float bits (non-negative floats order like their bit patterns): what the tolerance mode bounds
__global__ void mirror_check_kernel(const float *Pi, uint64_t I1, uint64_t I2, uint32_t *bad, uint32_t *dev) {
    const uint64_t half = (I2 + 1) / 2, n = I1 * half;
    float worst = 0.f;
    bool exact = true;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i1 = q % I1, c = q / I1;
        const float *a = Pi + 3 * (i1 + I1 * c), *b = Pi + 3 * (i1 + I1 * (I2 - 1 - c));
        if (!(a[0] == -b[0] && a[1] == b[1] && a[2] == b[2])) {      // (NaN coordinates: not symmetric, in either mode)
            exact = false;
            const float dx = a[0] + b[0], dy = a[1] - b[1], dz = a[2] - b[2];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            worst = (d == d) ? fmaxf(worst, d) : INFINITY;
        }
    }
    if (!exact) { *bad = 1u; atomicMax(dev, __float_as_uint(worst)); }
}
// a per-pixel map (I1 x I2, contiguous): c[i1, I2-1-col] == c[i1, col] bit for bit?
__global__ void mirror_map_check_kernel(const uint32_t *c, uint64_t I1, uint64_t I2, uint32_t *bad) {
    const uint64_t n = I1 * (I2 / 2);
    bool same = true;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i1 = q % I1, col = q / I1;
        if (c[i1 + I1 * col] != c[i1 + I1 * (I2 - 1 - col)]) same = false;
    }
    if (!same) *bad = 1u;
}
static int mirror_symmetric_map(const float *dmap, uint64_t I1, uint64_t I2, bool *yes) {
    *yes = false;
    uint32_t *flag = nullptr, res = 1;
    HIPCHK(plan_malloc((void **)&flag, sizeof(uint32_t)));
    hipError_t e = hipMemset(flag, 0, sizeof(uint32_t));
    if (e == hipSuccess) {
        const uint64_t n = I1 * (I2 / 2);
        mirror_map_check_kernel<<<(unsigned)std::min<uint64_t>((n + 255) / 256 + 1, 4096), 256, 0, 0>>>((const uint32_t *)dmap, I1, I2, flag);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(&res, flag, sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    (void)hipFree(flag);
    HIPCHK(e);
    *yes = res == 0;
    return QDAS_OK;
}
// receivers, transmits (positions, normals, t0) and pixel columns mirror-symmetric about x = 0?  fp32 geometry.
// Exact mode (`tol` < 0): bit for bit.  Tolerance mode (QDAS_PLAN_APPROX_SYMMETRY, `tol` >= 0 in SAMPLES): positions may deviate -- distance is
// 1-Lipschitz in either end point, so |tau(p', N-1-n, M-1-m) - tau(p, n, m)| * fs <= cinv * fs * (2 max|M(p') - p| + max|M(r') - r| + max|M(v') - v|) =: bound,
// and the mode is taken when bound <= tol; normals and start times (which enter the plane-wave delay and the focused-wave sign) must still match exactly.
static int mirror_symmetric(const qdas_desc *desc, const float *dPi, bool *yes, double tol = -1.0, double cinv_fs = 0.0, double *bound = nullptr) {
    const qdas_sizes &z = desc->sz;
    *yes = false;
    if (bound) *bound = 0.0;
    std::vector<float> hr(3 * z.N), hv(4 * z.M), hn(3 * z.M);
    int rc;
    if ((rc = fetch_host(desc->Pr, hr.size() * 4, desc->mem, hr.data()))) return rc;
    if ((rc = fetch_host(desc->Pv, hv.size() * 4, desc->mem, hv.data()))) return rc;
    if ((rc = fetch_host(desc->Nv, hn.size() * 4, desc->mem, hn.data()))) return rc;
    double dr = 0.0, dv = 0.0;                          // largest deviation of a receiver / transmit position from its mirror partner's image
    auto dist3 = [](const float *a, const float *b) { const double dx = (double)a[0] + (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2]; return sqrt(dx * dx + dy * dy + dz * dz); };
    for (uint64_t n = 0; n < z.N; ++n) {
        const float *a = &hr[3 * n], *b = &hr[3 * (z.N - 1 - n)];
        if (!(a[0] == -b[0] && a[1] == b[1] && a[2] == b[2])) {
            if (tol < 0) return QDAS_OK;
            const double d = dist3(a, b);
            if (!(d == d)) return QDAS_OK;
            dr = std::max(dr, d);
        }
    }
    for (uint64_t m = 0; m < z.M; ++m) {
        const float *a = &hv[4 * m], *b = &hv[4 * (z.M - 1 - m)], *c = &hn[3 * m], *d = &hn[3 * (z.M - 1 - m)];
        if (!(a[3] == b[3] && c[0] == -d[0] && c[1] == d[1] && c[2] == d[2])) return QDAS_OK;       // start times and normals: exact in both modes
        if (!(a[0] == -b[0] && a[1] == b[1] && a[2] == b[2])) {
            if (tol < 0) return QDAS_OK;
            const double e = dist3(a, b);
            if (!(e == e)) return QDAS_OK;
            dv = std::max(dv, e);
        }
    }
    if (desc->rx_apod_kind && desc->rx_normals) {       // a generated receive apodization: the element normals as well
        std::vector<float> hx(3 * z.N);
        if ((rc = fetch_host(desc->rx_normals, hx.size() * 4, desc->mem, hx.data()))) return rc;
        for (uint64_t n = 0; n < z.N; ++n) {
            const float *a = &hx[3 * n], *b = &hx[3 * (z.N - 1 - n)];
            if (!(a[0] == -b[0] && a[1] == b[1] && a[2] == b[2])) return QDAS_OK;
        }
    }
    uint32_t *flag = nullptr;
    HIPCHK(plan_malloc((void **)&flag, 2 * sizeof(uint32_t)));
    hipError_t e = hipMemset(flag, 0, 2 * sizeof(uint32_t));
    uint32_t res[2] = {1u, 0x7f800000u};
    if (e == hipSuccess) {
        const uint64_t n = z.I1 * ((z.I2 + 1) / 2);
        mirror_check_kernel<<<(unsigned)std::min<uint64_t>((n + 255) / 256, 4096), 256, 0, 0>>>(dPi, z.I1, z.I2, flag, flag + 1);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(res, flag, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    (void)hipFree(flag);
    HIPCHK(e);
    float dpf;
    memcpy(&dpf, &res[1], 4);
    const double dp = res[0] ? (double)dpf : 0.0;
    if (tol < 0) { *yes = res[0] == 0; return QDAS_OK; }
    const double b = cinv_fs * (2.0 * dp + dr + dv);
    if (bound) *bound = b;
    *yes = b == b && b <= tol;
    return QDAS_OK;
}

// ------------------------------------------------------------------------------------ plan creation
// qdas_plan_create in steps.  WHAT a plan runs -- kernel, launch configuration, symmetry modes, and why not -- is decided by the pure functions of
// plan_modes.h (testable without a GPU: tests/modes/enumerate_modes.cpp); the steps below gather the facts those functions ask for (host comparisons of
// the geometry, the device's mirror check, allocations, window-fit probes) and carry out their decisions (uploads, tables, kernel builds).
static modes::Switches read_switches() {
    modes::Switches sw;
    auto on = [](const char *n) { return getenv(n) != nullptr; };
    sw.no_sym = on("QDAS_NO_SYM"); sw.no_fold = on("QDAS_NO_FOLD"); sw.no_jit = on("QDAS_NO_JIT"); sw.no_mirror = on("QDAS_NO_MIRROR"); sw.no_mirq = on("QDAS_NO_MIRQ");
    sw.no_narrow = on("QDAS_NO_NARROW"); sw.no_role_swap = on("QDAS_NO_ROLE_SWAP"); sw.no_bpix = on("QDAS_NO_BPIX"); sw.no_w64 = on("QDAS_NO_W64");
    sw.no_mirror_wpix = on("QDAS_NO_MIRROR_WPIX"); sw.no_mirror_wpix32 = on("QDAS_NO_MIRROR_WPIX32"); sw.no_side_split = on("QDAS_NO_SIDE_SPLIT"); sw.no_wide = on("QDAS_NO_WIDE");
    sw.no_fb2 = on("QDAS_NO_FB2"); sw.no_fb4 = on("QDAS_NO_FB4"); sw.no_fold16 = on("QDAS_NO_FOLD16");
    if (const char *e = getenv("QDAS_SYM_TOL")) { const double v = atof(e); if (v >= 0.0 && v <= 0.5) sw.sym_tol = v; }
    if (const char *e = getenv("QDAS_KSPLIT")) { const int v = atoi(e); if (v >= 1 && v <= 8) sw.ksplit = v; }
    if (const char *e = getenv("QDAS_KSPLIT_M")) { const int v = atoi(e); if (v >= 1 && v <= 8) sw.ksplit_m = v; }
    return sw;
}

// working state of one qdas_plan_create
struct PlanBuild {
    const qdas_desc *desc = nullptr;
    modes::Switches sw;
    modes::Request rq;
    modes::Symmetry sy;
    size_t ael = 0;                         // bytes per apodization entry
    int txkind = 0;                         // distance | signed distance | plane wave
    std::vector<float> host_tab;            // the folded N x M table as uploaded ([stage element + stages * block element])
    uint64_t kN_eff = 0;                    // stage elements after a side split
    modes::BuildOutcome outcome;            // what the build steps did (plan_modes.h derive_launch_shape: the model the finished plan is checked against)
};

// sizes, slab, output planes; QDAS_PLAN_MIRROR_SLAB validation
static int plan_init(qdas_plan *pl, const qdas_desc *desc) {
    pl->d = *desc;
    const qdas_sizes &z = pl->d.sz;
    pl->I = z.I1 * z.I2 * z.I3;
    pl->i_count = desc->i_count ? desc->i_count : pl->I - desc->i_begin;
    pl->y_ld = desc->y_ld ? desc->y_ld : pl->i_count;
    pl->oN = (z.flag & QDAS_FLAG_KEEP_RX) ? z.N : 1;
    pl->oM = (z.flag & QDAS_FLAG_KEEP_TX) ? z.M : 1;
    if (pl->y_ld < pl->i_count) return fail(QDAS_EINVAL, "y_ld smaller than the pixel count");
    if (desc->plan_flags & QDAS_PLAN_MIRROR_SLAB) {
        const bool ok = z.I3 == 1 && z.I2 % 2 == 0 && z.I1 && desc->i_begin % z.I1 == 0 && pl->i_count % z.I1 == 0 && pl->i_count
                        && desc->i_begin + pl->i_count <= pl->I / 2 && !(z.flag & (QDAS_FLAG_KEEP_RX | QDAS_FLAG_KEEP_TX)) && desc->kernel != QDAS_KERNEL_GENERIC;
        if (!ok) return fail(QDAS_EINVAL, "QDAS_PLAN_MIRROR_SLAB: the slab must be whole columns of the first half of an even number of columns (I3 == 1, 'DAS')");
        if (!desc->y_ld) pl->y_ld = 2 * pl->i_count;     // y holds slab A and its mirror image
        else if (desc->y_ld < 2 * pl->i_count) return fail(QDAS_EINVAL, "QDAS_PLAN_MIRROR_SLAB: y_ld smaller than 2 * i_count (y holds slab A and its mirror image)");
    }
    return QDAS_OK;
}

// stride tables (host pointer, reference kern/das_spec.m:257-260) + device copies of the constant inputs -> the generic kernel's parameter block
static int plan_import_inputs(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    const int dt = z.dtype;
    GenericParams &g = pl->gp;
    int rc;
    memcpy(g.cst, desc->acstride, sizeof g.cst);
    memset(g.ast, 0, sizeof g.ast);
    memcpy(g.ast, desc->acstride + 6, sizeof(uint64_t) * 6 * z.S);
    const size_t rs = real_size(dt);
    uint64_t apod_elems = 0;
    for (uint64_t s = 0; s < z.S; ++s) {
        const uint64_t end = g.ast[6 * s + 5] + bcast_numel(&g.ast[6 * s], z);
        if (end > apod_elems) apod_elems = end;
    }
    b.ael = desc->apod_real ? apod_real_size(dt) : data_size(dt);
    const uint64_t cinv_elems = bcast_numel(g.cst, z);
    if ((rc = import_array(pl, desc->Pi, 3 * pl->I * rs, desc->mem, &g.Pi))) return rc;
    if ((rc = import_array(pl, desc->Pr, 3 * z.N * rs, desc->mem, &g.Pr))) return rc;
    if ((rc = import_array(pl, desc->Pv, 4 * z.M * rs, desc->mem, &g.Pv))) return rc;
    if ((rc = import_array(pl, desc->Nv, 3 * z.M * rs, desc->mem, &g.Nv))) return rc;
    if ((rc = import_array(pl, desc->cinv, cinv_elems * rs, desc->mem, &g.cinv))) return rc;
    if ((rc = import_array(pl, desc->apod, apod_elems * b.ael, desc->mem, &g.apod))) return rc;
    g.T = z.T; g.N = z.N; g.M = z.M; g.I1 = z.I1; g.I2 = z.I2; g.I3 = z.I3;
    g.i_begin = desc->i_begin; g.i_count = pl->i_count; g.y_ld = pl->y_ld;
    // the reference passes [fs, fmod] in the kernel's real type (src/bf.cu:57-58)
    g.fs = dt == QDAS_F64 ? desc->fs : (double)(float)desc->fs;
    g.fmod = dt == QDAS_F64 ? desc->fmod : (double)(float)desc->fmod;
    g.S = (int32_t)z.S; g.flag = z.flag; g.VS = z.VS; g.DV = z.DV; g.apod_real = desc->apod_real;
    g.gen_kind = desc->rx_apod_kind; g.gen_p0 = desc->rx_apod_p[0]; g.gen_p1 = desc->rx_apod_p[1]; g.rxn = nullptr;
    if (g.gen_kind && desc->rx_normals && (rc = import_array(pl, desc->rx_normals, 3 * z.N * rs, desc->mem, &g.rxn))) return rc;
    g.tile_list = nullptr; g.blocks_per_tile = 0; g.tile_cols = 0; g.tiles_z = 0;
    if (dt == QDAS_F64) { if ((rc = fetch_host(desc->cinv, sizeof(double), desc->mem, &pl->cinv0))) return rc; }
    else { float c32; if ((rc = fetch_host(desc->cinv, sizeof(float), desc->mem, &c32))) return rc; pl->cinv0 = (double)c32; }
    return QDAS_OK;
}

// FACT (plan_modes.h Facts::recip_*): do the transmit elements equal the receive elements, with one start time?  Host comparison of the fp32 geometry.
static int gather_recip_facts(const qdas_desc *desc, modes::Facts *f) {
    const qdas_sizes &z = desc->sz;
    std::vector<float> hr(3 * z.N), hv(4 * z.M);
    int rc;
    if ((rc = fetch_host(desc->Pr, hr.size() * 4, desc->mem, hr.data()))) return rc;
    if ((rc = fetch_host(desc->Pv, hv.size() * 4, desc->mem, hv.data()))) return rc;
    f->recip_known = true; f->recip_one_t0 = true; f->recip_exact = true; f->recip_finite = true; f->recip_dev = 0.0;
    for (uint64_t m = 0; m < z.M; ++m) {
        if (memcmp(&hv[4 * m + 3], &hv[3], 4) != 0) { f->recip_one_t0 = false; break; }                 // one start time: exact in both modes
        if (memcmp(&hv[4 * m], &hr[3 * m], 12) != 0) {
            f->recip_exact = false;
            const double dx = (double)hv[4 * m] - hr[3 * m], dy = (double)hv[4 * m + 1] - hr[3 * m + 1], dz = (double)hv[4 * m + 2] - hr[3 * m + 2];
            const double dd = sqrt(dx * dx + dy * dy + dz * dz);      // tolerance mode: the largest distance between a transmit element and "its" receive element
            if (!(dd == dd)) f->recip_finite = false; else f->recip_dev = std::max(f->recip_dev, dd);
        }
    }
    return QDAS_OK;
}

// steps 1 + 2 of plan_modes.h: the request, then the symmetry modes -- gathering each fact the resolver asks for
static int plan_resolve_modes(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    b.rq = modes::analyze_request(*desc, b.sw);
    modes::Facts f;
    f.cinv0 = pl->cinv0;
    int rc;
    for (;;) {
        const int need = modes::resolve_symmetry(*desc, pl->i_count, b.rq, f, b.sw, &b.sy);
        if (need == modes::NEED_NOTHING) break;
        if (need == modes::NEED_RECIP) { if ((rc = gather_recip_facts(desc, &f))) return rc; }
        else if (need == modes::NEED_FOLD_BUF) {          // the plan's folded copy of a frame: without the memory for it, the plan simply does not fold
            void *fbuf = nullptr;
            f.fold_buf_known = true;
            if (plan_malloc(&fbuf, (size_t)z.T * z.N * z.M * 8) != hipSuccess) { (void)hipGetLastError(); f.fold_buf_ok = false; }
            else { pl->owned.push_back(fbuf); pl->fold_buf = fbuf; f.fold_buf_ok = true; }
        } else if (need == modes::NEED_MIRROR) {
            bool yes = false;
            double bound = 0.0;
            if ((rc = mirror_symmetric(desc, (const float *)pl->gp.Pi, &yes, b.sy.sym_tol, pl->cinv0 * desc->fs, &bound))) return rc;
            // (a sound-speed map: exact mode only -- plan_modes.h leaves sym_tol unset for maps --, and the map itself mirror-symmetric bit for bit)
            if (yes && b.rq.cmap && (rc = mirror_symmetric_map((const float *)pl->gp.cinv + pl->gp.cst[5], z.I1, z.I2, &yes))) return rc;
            f.mirror_known = true; f.mirror_yes = yes; f.mirror_bound = bound;
        }
    }
    if (b.sy.prefolded_refused)
        return fail(QDAS_EUNSUPPORTED, "QDAS_PLAN_PREFOLDED: a folded frame can only be beamformed by a reciprocal fp32 'DAS' plan without apodization arrays "
                                       "(transmit elements == receive elements bit for bit, one t0, N == M >= 2; weights belong to qdas_fold)");
    pl->prefolded = b.sy.prefolded;
    pl->tc = b.sy.tc();
    if (desc->kernel == QDAS_KERNEL_TILED && !b.sy.eligible) return fail(QDAS_EUNSUPPORTED, "%s", b.sy.why);
    pl->kernel = (b.sy.eligible && desc->kernel != QDAS_KERNEL_GENERIC) ? QDAS_KERNEL_TILED : QDAS_KERNEL_GENERIC;
    return QDAS_OK;
}

// roles swapped: stage elements = transmits (positions + {t0, normal} records), block elements = receivers (zero normals, zero start times)
static int upload_swapped_geometry(qdas_plan *pl, const qdas_desc *desc, uint64_t E, int shift) {      // E stage elements; element e reads transmit e >> shift
    const qdas_sizes &z = pl->d.sz;
    TileParams &t = pl->tp;
    std::vector<float> hr(3 * z.N), hv(4 * z.M), hn(3 * z.M);
    int rc;
    if ((rc = fetch_host(desc->Pr, hr.size() * 4, desc->mem, hr.data()))) return rc;
    if ((rc = fetch_host(desc->Pv, hv.size() * 4, desc->mem, hv.data()))) return rc;
    if ((rc = fetch_host(desc->Nv, hn.size() * 4, desc->mem, hn.data()))) return rc;
    std::vector<float> spos(3 * E), sst(4 * E), bpos(4 * z.N), bnrm(3 * z.N, 0.f);
    for (uint64_t e = 0; e < E; ++e) {
        const uint64_t m = e >> shift;
        for (int k = 0; k < 3; ++k) { spos[3 * e + k] = hv[4 * m + k]; sst[4 * e + 1 + k] = hn[3 * m + k]; }
        sst[4 * e] = hv[4 * m + 3];
    }
    for (uint64_t n = 0; n < z.N; ++n) { for (int k = 0; k < 3; ++k) bpos[4 * n + k] = hr[3 * n + k]; bpos[4 * n + 3] = 0.f; }
    const void *d0, *d1, *d2, *d3;
    if ((rc = import_array(pl, spos.data(), spos.size() * 4, QDAS_MEM_HOST, &d0))) return rc;
    if ((rc = import_array(pl, sst.data(), sst.size() * 4, QDAS_MEM_HOST, &d1))) return rc;
    if ((rc = import_array(pl, bpos.data(), bpos.size() * 4, QDAS_MEM_HOST, &d2))) return rc;
    if ((rc = import_array(pl, bnrm.data(), bnrm.size() * 4, QDAS_MEM_HOST, &d3))) return rc;
    t.Pr = (const float *)d0; t.St = (const float *)d1; t.Pv = (const float *)d2; t.Nv = (const float *)d3;
    return QDAS_OK;
}

// tile grid: (1 << tz_log2) pixels of I1 x tile_cols columns (columns = I2*I3 flattened)
static void plan_set_grid(qdas_plan *pl, int tzl) {
    TileParams &t = pl->tp;
    const qdas_sizes &z = pl->d.sz;
    t.tz_log2 = tzl;
    pl->tile_cols = ((unsigned)pl->tc.waves * 64u) >> tzl;
    const uint64_t col0 = pl->d.i_begin / z.I1, col1 = t.mir == 1 ? (z.I2 + 1) / 2 - 1 : (pl->d.i_begin + pl->i_count - 1) / z.I1;   // (mirror mode: the first half of the columns)
    t.tiles_z = (uint32_t)((z.I1 + (1u << tzl) - 1) >> tzl);
    t.tile_x0 = (uint32_t)(col0 / pl->tile_cols);
    t.tiles_x = (uint32_t)(col1 / pl->tile_cols) - t.tile_x0 + 1;
    pl->ntiles = t.tiles_z * t.tiles_x;
}

// the tiled kernel's parameter block from the resolved modes (everything except weights and the probed shape)
static int plan_setup_tile_params(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    const GenericParams &g = pl->gp;
    TileParams &t = pl->tp;
    int rc;
    t.Pi = (const float *)g.Pi; t.Pr = (const float *)g.Pr; t.Pv = (const float *)g.Pv; t.Nv = (const float *)g.Nv; t.St = nullptr;
    t.T = z.T; t.N = z.N; t.M = z.M; t.I1 = z.I1; t.I2 = z.I2; t.I3 = z.I3;
    t.i_begin = desc->i_begin; t.i_count = pl->i_count;
    const bool tp = z.flag & QDAS_FLAG_TPOSE;
    t.strN = tp ? z.T * z.M : z.T;                  // reference src/bf.cu:100
    t.strM = tp ? z.T : z.T * z.N;
    b.txkind = z.VS ? (z.DV ? 0 : 1) : 2;           // distance | signed distance | plane wave
    t.kindB = b.txkind; t.kindS = 0;
    if (b.sy.swap) {                                // roles swapped: stage elements = transmits, block elements = receivers
        if ((rc = upload_swapped_geometry(pl, desc, z.M, 0))) return rc;
        t.N = z.M; t.M = z.N;
        std::swap(t.strN, t.strM);
        t.kindB = 0; t.kindS = b.txkind;
    }
    t.fs = g.fs; t.fmod = g.fmod;
    t.cinv_fs = pl->cinv0 * g.fs;
    t.cinv_pix = b.rq.cmap ? (const float *)g.cinv + g.cst[5] : nullptr;
    t.flag = z.flag; t.VS = z.VS; t.DV = z.DV; t.sym = b.sy.sym; t.big = b.sy.big; t.fold = b.sy.rfold;
    t.mir = b.sy.mir ? (b.sy.mslab ? 2 : 1) : 0;
    unsigned max_tiles = 0;
    for (int l = 3; l <= 6; ++l) { plan_set_grid(pl, l); if (pl->ntiles > max_tiles) max_tiles = pl->ntiles; }
    void *fb;
    if ((rc = dev_alloc(pl, &fb, sizeof(uint32_t) * (max_tiles + 1)))) return rc;
    pl->fallback = (uint32_t *)fb;
    t.fallback_list = pl->fallback; t.fallback_cap = max_tiles;
    t.probe = 0; t.wz_log2 = 6; t.ksplit = 1; t.part = nullptr; t.nfr = 1; t.x_fstride = 0; t.y_fstride = 0;
    t.syn = b.rq.syn ? 1 : 0; t.y_ld = pl->y_ld;
    t.bf = b.rq.bfm ? 1 : 0;
    t.bf_pn = (z.flag & QDAS_FLAG_TPOSE) ? z.M : 1;      // plane nm = the data's aperture order (src/bf.cu:100,135)
    t.bf_pm = (z.flag & QDAS_FLAG_TPOSE) ? 1 : z.N;
    t.wtab = nullptr; t.apix = nullptr; t.apix_real = desc->apod_real;
    t.gen_kind = g.gen_kind; t.gen_p0 = g.gen_p0; t.gen_p1 = g.gen_p1; t.rxn = (const float *)g.rxn;
    t.bpix = nullptr;
    return QDAS_OK;
}

// product of the arrays `take` selects, broadcast to I x E entries (E = M: indexed by the transmit; N: by the receiver; 1: pixel-only)
template <class Take>
static int fold_pixel_arrays(qdas_plan *pl, const qdas_desc *desc, size_t ael, int side, Take take, void **out) {
    const qdas_sizes &z = pl->d.sz;
    const GenericParams &g = pl->gp;
    const int dt = z.dtype;
    ApodFold f;
    memset(&f, 0, sizeof f);
    f.base = g.apod; f.I1 = z.I1; f.I2 = z.I2; f.I3 = z.I3;
    f.E = side == 2 ? 1 : side == 1 ? z.M : z.N;
    for (uint64_t s = 0; s < z.S; ++s) {
        if (!take(s)) continue;
        const uint64_t *a = &g.ast[6 * s];
        uint64_t *q = f.st[f.ns++];
        q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; q[3] = side == 2 ? 0 : side == 1 ? (z.M > 1 ? a[4] : 0) : (z.N > 1 ? a[3] : 0); q[4] = a[5];
    }
    const uint64_t nel = z.I1 * z.I2 * z.I3 * f.E;
    void *fb;
    int frc = dev_alloc(pl, &fb, nel * ael);
    if (frc) return frc;
    const unsigned nb = (unsigned)std::min<uint64_t>((nel + 255) / 256, 1u << 20);
    if (desc->apod_real) {
        if (dt == QDAS_F32) apod_fold_kernel<float, false><<<nb, 256, 0, 0>>>(f, (float *)fb, nel);
        else apod_fold_kernel<_Float16, false><<<nb, 256, 0, 0>>>(f, (_Float16 *)fb, nel);
    } else {
        if (dt == QDAS_F32) apod_fold_kernel<float, true><<<nb, 256, 0, 0>>>(f, (float *)fb, nel);
        else apod_fold_kernel<_Float16, true><<<nb, 256, 0, 0>>>(f, (_Float16 *)fb, nel);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(0));
    *out = fb;
    return QDAS_OK;
}

// the pixel-dependent apodization of the plan: used in place, or multiplied into one plan-owned I x [N | M | 1] array (two with per-pair weights)
static int plan_pixel_weights(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    const GenericParams &g = pl->gp;
    TileParams &t = pl->tp;
    const modes::Request &rq = b.rq;
    int rc;
    if (rq.bpix_mode) {                                // transmit side (+ pixel-only arrays) -> stage weight; receive side -> per-pair weight (real fp32)
        void *fa_ = nullptr, *fb_ = nullptr;
        auto on_rx = [&](uint64_t s) { return g.ast[6 * s + 3] != 0 && z.N > 1; };
        if ((rc = fold_pixel_arrays(pl, desc, b.ael, 1, [&](uint64_t s) { return !on_rx(s); }, &fa_))) return rc;
        if ((rc = fold_pixel_arrays(pl, desc, b.ael, 0, on_rx, &fb_))) return rc;
        t.apix = (const unsigned char *)fa_; t.bpix = (const float *)fb_;
    } else if (rq.pix_fold) {
        void *fb = nullptr;
        if ((rc = fold_pixel_arrays(pl, desc, b.ael, rq.pix_only ? 2 : rq.pix_is_tx ? 1 : 0, [&](uint64_t s) { return rq.is_pix[s]; }, &fb))) return rc;
        t.apix = (const unsigned char *)fb;
    } else if (rq.pix_arr >= 0) {
        t.apix = (const unsigned char *)g.apod + g.ast[6 * rq.pix_arr + 5] * b.ael;
    }
    t.apix_pixel_only = rq.pix_only ? 1 : 0;
    t.act_bytes = ((t.apix || t.gen_kind) && z.dtype != QDAS_F64) ? (uint32_t)(8 * (t.N + 1)) : 0u;      // (fp64 data: the plain list of stages)
    return QDAS_OK;
}

// the pixel-independent apodization arrays folded into one N x M table (complex128 for fp64 data, else complex64; folded plans hand it to the fold pass)
static int plan_weight_table(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    const GenericParams &g = pl->gp;
    TileParams &t = pl->tp;
    const int dt = z.dtype;
    const size_t ael = b.ael;
    int rc;
    if (z.S > b.rq.npix && dt == QDAS_F64) {             // fp64 data: the table in double (complex128 entries)
        std::vector<double> tab(2 * z.N * z.M);
        for (size_t k = 0; k < z.N * z.M; ++k) { tab[2 * k] = 1.0; tab[2 * k + 1] = 0.0; }
        for (uint64_t s = 0; s < z.S; ++s) {
            if (b.rq.is_pix[s]) continue;                 // (the pixel x receiver array is applied per stage: das_tile_impl.h TileCfg::W64)
            const uint64_t *st = &g.ast[6 * s];
            const uint64_t nel = bcast_numel(st, z);
            std::vector<double> raw(nel * (desc->apod_real ? 1 : 2));
            if ((rc = fetch_host((const unsigned char *)desc->apod + st[5] * ael, nel * ael, desc->mem, raw.data()))) return rc;
            for (uint64_t m = 0; m < z.M; ++m)
                for (uint64_t n = 0; n < z.N; ++n) {
                    const uint64_t k = n * st[3] + m * st[4];
                    const double ar = desc->apod_real ? raw[k] : raw[2 * k], ai = desc->apod_real ? 0.0 : raw[2 * k + 1];
                    double &tr = tab[2 * (n + z.N * m)], &ti = tab[2 * (n + z.N * m) + 1];
                    const double nr = tr * ar - ti * ai, ni = tr * ai + ti * ar;
                    tr = nr; ti = ni;
                }
        }
        void *dtab;
        if ((rc = dev_alloc(pl, &dtab, tab.size() * sizeof(double)))) return rc;
        hipError_t e = upload(dtab, tab.data(), tab.size() * sizeof(double));
        if (e != hipSuccess) return fail(QDAS_EHIP, "hipMemcpy(wtab): %s", hipGetErrorString(e));
        t.wtab = dtab;
    } else if (z.S > b.rq.npix && dt != QDAS_F64) {
        std::vector<float> &tab = b.host_tab;
        tab.assign(2 * z.N * z.M, 0.f);
        for (size_t k = 0; k < z.N * z.M; ++k) { tab[2 * k] = 1.f; tab[2 * k + 1] = 0.f; }
        for (uint64_t s = 0; s < z.S; ++s) {
            if (b.rq.is_pix[s]) continue;
            const uint64_t *st = &g.ast[6 * s];
            const uint64_t nel = bcast_numel(st, z);
            std::vector<unsigned char> raw(nel * ael);
            if ((rc = fetch_host((const unsigned char *)desc->apod + st[5] * ael, nel * ael, desc->mem, raw.data()))) return rc;
            for (uint64_t m = 0; m < z.M; ++m)
                for (uint64_t n = 0; n < z.N; ++n) {
                    const uint64_t k = n * st[3] + m * st[4];
                    float ar, ai = 0.f;
                    if (desc->apod_real) ar = dt == QDAS_F32 ? ((const float *)raw.data())[k] : half_to_float(((const uint16_t *)raw.data())[k]);
                    else if (dt == QDAS_F32) { ar = ((const float *)raw.data())[2 * k]; ai = ((const float *)raw.data())[2 * k + 1]; }
                    else { ar = half_to_float(((const uint16_t *)raw.data())[2 * k]); ai = half_to_float(((const uint16_t *)raw.data())[2 * k + 1]); }
                    const size_t q = b.sy.swap ? (m + z.M * n) : (n + z.N * m);       // [stage element + stages * block element]
                    float &tr = tab[2 * q], &ti = tab[2 * q + 1];
                    const float nr = tr * ar - ti * ai, ni = tr * ai + ti * ar;
                    tr = nr; ti = ni;
                }
        }
        void *dtab;
        if ((rc = dev_alloc(pl, &dtab, tab.size() * sizeof(float)))) return rc;
        hipError_t e = upload(dtab, tab.data(), tab.size() * sizeof(float));
        if (e != hipSuccess) return fail(QDAS_EHIP, "hipMemcpy(wtab): %s", hipGetErrorString(e));
        t.wtab = dtab;
    }
    if (t.fold && t.wtab) { pl->fold_wtab = t.wtab; t.wtab = nullptr; }      // (folded data: the fold pass applies the table, trace by trace -- it need not be symmetric in any way)
    pl->wtab_real = !b.host_tab.empty();               // every entry of the table real?  (apodization windows usually are: hiprtc builds then accumulate with ONE packed FMA per sample)
    for (size_t k = 1; k < b.host_tab.size(); k += 2) if (b.host_tab[k] != 0.f) { pl->wtab_real = false; break; }
    return QDAS_OK;
}

// FACT: the folded table equals its own mirror image, w[n,m] == w[N-1-n,M-1-m] bit for bit (receive and transmit windows are)
static bool table_mirror_symmetric(const qdas_sizes &z, const std::vector<float> &tab, bool swap) {
    for (uint64_t m = 0; m < z.M; ++m)
        for (uint64_t n = 0; n < z.N; ++n) {
            const size_t q = swap ? (m + z.M * n) : (n + z.N * m), q2 = swap ? ((z.M - 1 - m) + z.M * (z.N - 1 - n)) : ((z.N - 1 - n) + z.N * (z.M - 1 - m));
            if (memcmp(&tab[2 * q], &tab[2 * q2], 8) != 0) return false;
        }
    return true;
}

// step 3 of plan_modes.h: the chain of window-fit probes; each step = one choose_tile_shape (four footprints on the device)
static int plan_probe_chain(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    TileParams &t = pl->tp;
    modes::ProbeState ps;
    ps.dtype = z.dtype; ps.sym = t.sym; ps.rfold = t.fold; ps.mir = t.mir; ps.narrow = 0; ps.bpix = b.rq.bpix_mode;
    ps.set_tc(b.sy.tc_sym, b.sy.tc_narrow, b.sy.tc_fb, b.sy.tc_mirq, b.sy.tc_fold);
    if (t.fold && pl->fold_buf) HIPCHK(hipMemset(pl->fold_buf, 0, (size_t)z.T * z.N * z.M * 8));      // (the lower triangle is never written: zeros, not garbage, where a border window reaches into it)
    const bool has_table = !b.host_tab.empty();
    const bool tsym = (t.mir && has_table && !t.fold) ? table_mirror_symmetric(z, b.host_tab, b.sy.swap) : true;
    auto set_grid = [&](int tzl) { plan_set_grid(pl, tzl); };
    auto probe = [&](const modes::ProbeState &s, bool *fit) -> int {
        t.mir = s.mir; t.narrow = s.narrow;
        pl->tc = s.tc();
        const int rc = choose_tile_shape(pl, desc, set_grid);
        *fit = pl->no_fallback;
        return rc;
    };
    int err = 0;
    (void)modes::run_probe_chain(ps, b.sw, has_table, tsym, probe, &err);
    if (err) return err;
    t.mir = ps.mir; t.narrow = ps.narrow;                // (the chain's last probe ran the final state: tc, grid and shape are the plan's)
    b.sy.mir = ps.mir != 0;
    b.outcome.mir = ps.mir; b.outcome.narrow = ps.narrow;
    return QDAS_OK;
}

// Focused transmits whose focal planes cut through the image: the delay flips sign there (src/bf.cu:106-108), so the tiles a plane
// crosses fit no window and would go to the generic kernel -- with a walking aperture that is half the image.  Second attempt:
// every transmit listed twice, once per side of its plane (tile_params.h kindS == 3); kept if fewer tiles misfit.
static int plan_side_split(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    TileParams &t = pl->tp;
    b.kN_eff = b.sy.kN;
    if (!modes::side_split_applicable(*desc, b.rq, b.sy, pl->no_fallback, b.txkind, b.sy.wtb != 0, b.sw)) return QDAS_OK;
    int rc;
    const TileParams keep = t;
    const double keep_frac = pl->misfit_frac;
    const unsigned keep_ntiles = pl->ntiles, keep_cols = pl->tile_cols;
    const bool tp = z.flag & QDAS_FLAG_TPOSE;
    const uint64_t E = 2 * z.M;                          // stage elements: (transmit, side)
    if ((rc = upload_swapped_geometry(pl, desc, E, 1))) return rc;
    t.N = E; t.M = z.N;
    t.strN = tp ? z.T : z.T * z.N;                       // stage element = transmit, block element = receiver
    t.strM = tp ? z.T * z.M : z.T;
    t.kindB = 0; t.kindS = 3; t.stage_shift = 1;
    t.gen_kind = t.apix ? 6 : 5; t.gen_p0 = t.gen_p1 = 0.0; t.rxn = nullptr;      // (6: the side rule times the plan's pixel x transmit / pixel-only array)
    t.act_bytes = (uint32_t)(8 * (E + 1));
    if (t.wtab) {                                        // the table in the new element order: [(2m + side) + 2M * n]
        std::vector<float> tab2(2 * E * z.N);
        for (uint64_t n = 0; n < z.N; ++n)
            for (uint64_t e = 0; e < E; ++e) {
                const uint64_t m = e >> 1, q = b.sy.swap ? (m + z.M * n) : (n + z.N * m);
                tab2[2 * (e + E * n)] = b.host_tab[2 * q]; tab2[2 * (e + E * n) + 1] = b.host_tab[2 * q + 1];
            }
        void *dtab2;
        if ((rc = dev_alloc(pl, &dtab2, tab2.size() * sizeof(float)))) return rc;
        hipError_t e2 = upload(dtab2, tab2.data(), tab2.size() * sizeof(float));
        if (e2 != hipSuccess) return fail(QDAS_EHIP, "hipMemcpy(wtab): %s", hipGetErrorString(e2));
        t.wtab = dtab2;
    }
    auto set_grid = [&](int tzl) { plan_set_grid(pl, tzl); };
    if ((rc = choose_tile_shape(pl, desc, set_grid))) return rc;
    if (pl->misfit_frac < keep_frac) { b.kN_eff = E; b.outcome.side_split = true; }
    else {                                               // no better: the plan as it was
        t = keep;
        pl->misfit_frac = keep_frac; pl->no_fallback = keep_frac == 0.0; pl->ntiles = keep_ntiles; pl->tile_cols = keep_cols;
        HIPCHK(hipMemset(pl->fallback, 0, sizeof(uint32_t)));
    }
    return QDAS_OK;
}

// Tiles that still do not fit (a pixel grid coarser than about lambda/2 -- volumes, previews --, steep delay gradients): fp32 plans
// try the 384-sample windows of launch configuration 14 (16 transmits per stage, same LDS image); kept if fewer tiles misfit.
// (a reciprocal plan gives up its mode for them: an image on the generic kernel costs ten times more than the shared index work saves)
static int plan_wide_windows(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    TileParams &t = pl->tp;
    if (!modes::wide_applicable(z.dtype, pl->no_fallback, b.rq.bfm, t.big, t.narrow, pl->prefolded, t.N, t.M, t.strN, t.strM, t.act_bytes != 0,
                                t.wtab || (t.fold && pl->fold_wtab), b.sw)) return QDAS_OK;      // (a folded plan's table comes back into the kernel there)
    int rc;
    const TileParams keep = t;
    const TileConfig keep_tc = pl->tc;
    const double keep_frac = pl->misfit_frac;
    const unsigned keep_ntiles = pl->ntiles, keep_cols = pl->tile_cols;
    t.narrow = 2; t.sym = 0;
    if (t.fold) { t.fold = 0; t.wtab = pl->fold_wtab; }      // (the wide-window configuration is a general-mode kernel on the frame as it is)
    pl->tc = tile_config(z.dtype, 0, 2);
    auto set_grid = [&](int tzl) { plan_set_grid(pl, tzl); };
    if ((rc = choose_tile_shape(pl, desc, set_grid))) return rc;
    b.outcome.wide = pl->misfit_frac < keep_frac;
    if (!b.outcome.wide) {
        t = keep; pl->tc = keep_tc;
        pl->misfit_frac = keep_frac; pl->no_fallback = keep_frac == 0.0; pl->ntiles = keep_ntiles; pl->tile_cols = keep_cols;
        HIPCHK(hipMemset(pl->fallback, 0, sizeof(uint32_t)));
    }
    return QDAS_OK;
}

// Stage shape of plan-specialised builds.  The prebuilt configurations stage 16 transmits x 2 window sets x 192 samples (general-mode lateral-mirror plans:
// BASELINE C2, plane-wave compounding) or 32 transmits x 192 samples (one window set: general mode, the reciprocity fold without the mirror mode); fp16 data: 384 samples.  A
// hiprtc build takes any shape: when every tile of some footprint fits ONE-KiB windows (128 samples of fp32, 256 of fp16 data), 32 x 2 resp. 64 x 1 of them -- the same 64 KiB
// per buffer (the one-set plans: 64 instead of 48), HALF the stages (barriers, receive-delay evaluations, weight loads, DMA issue) -- is the better shape (C2 1.70 -> 1.61 ms;
// C3 without any symmetry -6 %, the fold alone -3 %; round 6, fp16 data incl. plans with a pixel x receiver weight: BASELINE C5 1.73 -> 1.59 ms, same box).  Asked with the
// prebuilt probe kernels (tile_params.h probe_w); if the build fails later the plan runs the prebuilt kernel on the footprint chosen here (the narrower window fits the wider).
static int plan_stage_shape(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    TileParams &t = pl->tp;
    const bool jit_on = (desc->plan_flags & QDAS_PLAN_JIT) && !b.sw.no_jit;
    const bool f16 = z.dtype == QDAS_F16;
    // (fp32 frames with a pixel x receiver weight took this shape in round 6 as well: one accumulator per pixel -- TileCfg::ONEACC -- made room for the weighted totals, and a build
    //  that still needs scratch is rebuilt with the plain pair loop, jit.hip jit_kernel: C3 with a generated f/1.5 mask 13.3 -> see profiles/r06.
    //  fp16 data: the two-window-set plans only -- one set of 64 transmits measured SLOWER on BASELINE C5 without the mirror mode, 2.37 -> 2.80 ms: M = 96 is 1.5 such blocks)
    if (!(jit_on && (z.dtype == QDAS_F32 || f16) && !t.big && !t.bf && !t.syn && !t.bpix && t.narrow == 0 && !t.stage_shift && !t.cinv_pix
          && !(f16 && (t.sym || !t.mir)) && pl->no_fallback && !getenv("QDAS_NO_STAGE_SHAPE") && !getenv("QDAS_JIT_MB") && !getenv("QDAS_JIT_W"))) return QDAS_OK;
    int mb = 0, sets = 1;
    if (t.mir && !t.sym) { mb = 32; sets = 2; }                          // two window sets: a pixel and its mirror image
    else if (!t.mir && (!t.sym || t.fold)) { mb = 64; sets = 1; }        // one window set
    if (!mb || t.M < (uint64_t)mb) return QDAS_OK;
    const int w1k = f16 ? 256 : 128;                                     // samples of a one-KiB window
    // LDS image of the specialised build: the header of the prebuilt configuration (+ the stage weights of the longer stages) + 2 buffers x sets x mb windows x 1 KiB
    const int pixw = t.act_bytes ? 1 : 0;
    const size_t hdr = tile_lds_bytes(z.dtype, t.sym, t.N, t.M, 0, pixw, t.wtab ? 1 : 0, 0, t.fold) - tile_config(z.dtype, t.sym, 0, t.mir ? 2 : 1, 0, t.fold).lds_bytes;
    if (hdr + (t.wtab ? (size_t)2 * 2 * (size_t)mb * 8 : 0) + (size_t)2 * sets * mb * 1024 > (size_t)158 * 1024) return QDAS_OK;
    int rc;
    const TileParams keep = t;
    const double keep_frac = pl->misfit_frac;
    const unsigned keep_ntiles = pl->ntiles, keep_cols = pl->tile_cols;
    const bool keep_nf = pl->no_fallback;
    t.probe_w = w1k;
    auto set_grid = [&](int tzl) { plan_set_grid(pl, tzl); };
    if ((rc = choose_tile_shape(pl, desc, set_grid))) return rc;
    const bool fits = pl->no_fallback;
    t.probe_w = 0;
    if (fits) { pl->hint_mb = mb; pl->hint_w = w1k; }
    else {
        t = keep;
        pl->misfit_frac = keep_frac; pl->no_fallback = keep_nf; pl->ntiles = keep_ntiles; pl->tile_cols = keep_cols;
        HIPCHK(hipMemset(pl->fallback, 0, sizeof(uint32_t)));
    }
    return QDAS_OK;
}

// step 4 of plan_modes.h: workgroups per tile (+ the partial images of a split aperture)
static int plan_split_aperture(qdas_plan *pl, PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    TileParams &t = pl->tp;
    int ncu = 0, rc;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device));
    const unsigned cus = ncu > 0 ? (unsigned)ncu : 256u;
    int mb_eff = pl->hint_mb ? pl->hint_mb : pl->tc.mb;             // (transmits per stage of the kernel the plan means to run: plan_stage_shape)
    int mb_grp = pl->hint_mb ? pl->hint_mb : pl->tc.mb;             // (... and of the transmit-block groups of a two-dimensional split)
    if (const char *e = getenv("QDAS_JIT_MB")) { const int mb = atoi(e); if (mb >= 2 && mb % pl->tc.waves == 0 && (b.desc->plan_flags & QDAS_PLAN_JIT) && !b.sw.no_jit) { mb_eff = mb; mb_grp = mb; } }      // (tuning builds, plan_jit)
    t.ksplit = modes::choose_ksplit(pl->ntiles, cus, z.M, mb_eff, t.sym != 0, b.kN_eff, t.act_bytes != 0, t.syn != 0, b.sw);
    t.ksplit_m = modes::choose_ksplit_m(&t.ksplit, t.M, mb_grp, t.sym != 0, t.act_bytes != 0, t.syn != 0, z.dtype, b.sw);
    if (t.ksplit > 1 && !t.bf) {
        void *pb;
        if ((rc = dev_alloc(pl, &pb, sizeof(float) * 2 * (size_t)t.ksplit * 4 * pl->i_count * (t.mir == 2 ? 2 : 1)))) return rc;   // x4: up to four frames per launch (fp64 data: one complex128 frame -- fits as well)
        t.part = (float2 *)pb;
    }
    return QDAS_OK;
}

// QDAS_PLAN_JIT: the tiled kernel compiled for this plan's sizes (jit.hip).  A failure is not an error: the plan keeps its prebuilt kernel and
// qdas_last_error() says why -- unless the plan's mode exists as a hiprtc build only: *remake = the plan flag to add for a second attempt without it.
static int plan_jit(qdas_plan *pl, const qdas_desc *desc, int *remake) {
    const qdas_sizes &z = pl->d.sz;
    const int dt = z.dtype;
    *remake = 0;
    g_err.clear();
    if (!((desc->plan_flags & QDAS_PLAN_JIT) && pl->kernel == QDAS_KERNEL_TILED && !pl->tp.bf && !getenv("QDAS_NO_JIT"))) return QDAS_OK;
    const TileParams &t = pl->tp;
    JitSpec k{};
    k.interp = (z.flag & 7) == 4 ? 1 : (z.flag & 7); k.dtype = dt; k.fmod = t.fmod != 0.0; k.wtab = t.wtab != nullptr; k.sym = t.sym; k.big = t.big;
    const int narrow = (t.sym && dt == QDAS_F32 && t.narrow) ? 1 : (!t.sym && dt == QDAS_F32 && t.narrow == 2) ? 2 : 0;
    const int mirq = (t.sym && t.mir) ? 1 : 0;
    const Cfg &cg = CFGS[cfg_index(dt, t.sym, t.fold ? 1 : (t.mir ? 2 : 1), narrow, mirq, t.fold)];      // (fb = 2 selects the two-window-set configuration of a general-mode mirror plan; folded plans: one frame)
    k.mir = t.sym ? 0 : t.mir; k.mirq = mirq; k.mslab = t.mir == 2; k.fold = t.fold;
    k.waves = cg.waves; k.mb = cg.mb; k.w = cg.w; k.nbuf = cg.nbuf;
    k.N = t.N; k.M = t.M; k.T = t.T; k.I1 = t.I1; k.strN = t.strN; k.strM = t.strM;
    k.kindB = t.kindB; k.kindS = t.kindS; k.tzl = t.tz_log2; k.wzl = t.wz_log2; k.ksplit = t.ksplit;
    k.gen_kind = t.gen_kind; k.has_apix = t.apix != nullptr; k.apix_real = t.apix_real; k.syn = t.syn;
    k.has_st = t.St != nullptr; k.has_cinv_pix = t.cinv_pix != nullptr;
    k.wreal = (t.wtab && pl->wtab_real && !getenv("QDAS_NO_WREAL")) ? 1 : 0;
    // tuning: a specialised build may use another number of transmits per stage than the prebuilt configuration (its register
    // budget is smaller); the LDS image grows with it
    // reciprocal mode: the specialised kernel has the registers for 32-transmit stages (half the stages, barriers and per-stage
    // delay evaluations of the prebuilt 16-transmit configuration) whenever the 64 windows of a buffer stay within the 16-bit
    // immediate offsets of the LDS reads (C3: 30.9 -> 29.2 ms)
    if (t.sym && !mirq && !t.fold && z.M % 32 == 0 && 2 * 32 * k.w * (dt == QDAS_F16 ? 4 : 8) <= 65536 && !getenv("QDAS_JIT_NO_MB32")) k.mb = 32;
    if (pl->hint_mb && pl->hint_w) { k.mb = pl->hint_mb; k.w = pl->hint_w; }      // (plan_stage_shape: the tiles were probed for this window)
    if (const char *e = getenv("QDAS_JIT_MB")) {
        const int mb = atoi(e);
        if (mb >= 2 && mb % k.waves == 0 && (!t.sym || t.fold || z.M % (uint64_t)mb == 0) && (!mirq || t.fold)) k.mb = mb;
    }
    if (const char *e = getenv("QDAS_JIT_NBUF")) { const int nb = atoi(e); if (nb >= 2 && nb <= 4) k.nbuf = nb; }
    if (const char *e = getenv("QDAS_JIT_W")) { const int wv = atoi(e); if (wv >= 64 && wv <= 1024 && wv % 64 == 0) k.w = wv; }      // (experiments: tiles that do not fit go to the generic kernel)
    pl->jit_lds = dt == QDAS_F64 ? 0 : jit_tile_lds(k, t.N, t.M, t.act_bytes, t.wtab != nullptr);       // (fp64 data: the prebuilt configuration's own LDS image, das_tile.hip)
    const JitKernel jk = pl->jit_lds > (size_t)160 * 1024 ? JitKernel{nullptr, "", "LDS image too large for the requested configuration"} : jit_kernel(k, pl->device);
    pl->jit_fn = jk.fn;
    if (jk.fn) { pl->jit_tag = "jit " + jk.key; pl->jit_mb = k.mb; pl->jit_w = k.w; return QDAS_OK; }
    g_err = "QDAS_PLAN_JIT: " + jk.err + " -- using the prebuilt kernel";
    const bool unfolded = dt == QDAS_F32 && t.sym && !t.fold;                  // (likewise: the general kernels then)
    if ((dt == QDAS_F32 && t.mir && !t.sym && (t.apix || t.gen_kind)) || unfolded)      // exists only as a hiprtc build: the same plan without the mode
        *remake = unfolded ? QDAS_PLAN_NO_RECIPROCAL : QDAS_PLAN_NO_MIRROR;
    return QDAS_OK;
}

// fp16 reciprocal data on the folded fp32 kernels: an fp32 PREFOLDED child plan over the same geometry and slab; this plan folds each frame into a
// complex64 copy (its weight table applied on the way), the child beamforms it, the complex64 image is rounded to complex32.  If anything of that is
// not available (memory, a child that does not fit) the plan keeps its own fp16 reciprocal kernels.
static void plan_f16_child(qdas_plan *pl, const qdas_desc *desc) {
    const qdas_sizes &z = pl->d.sz;
    if (!(pl->kernel == QDAS_KERNEL_TILED && z.dtype == QDAS_F16 && pl->tp.sym && !pl->tp.syn && !pl->tp.bf && !(desc->plan_flags & QDAS_PLAN_NO_FOLD) && !getenv("QDAS_NO_FOLD")
          && !getenv("QDAS_NO_FOLD16") && z.N >= 2 && z.N <= 65535)) return;
    qdas_desc d = *desc;
    const GenericParams &gg = pl->gp;
    uint64_t acs[6] = {gg.cst[0], gg.cst[1], gg.cst[2], gg.cst[3], gg.cst[4], gg.cst[5]};
    d.sz.dtype = QDAS_F32; d.sz.S = 0;
    d.Pi = gg.Pi; d.Pr = gg.Pr; d.Pv = gg.Pv; d.Nv = gg.Nv; d.cinv = gg.cinv; d.apod = nullptr; d.rx_normals = nullptr; d.rx_apod_kind = 0; d.acstride = acs;
    d.mem = QDAS_MEM_DEVICE; d.device = pl->device; d.y_ld = 0;
    d.plan_flags = (d.plan_flags | QDAS_PLAN_PREFOLDED) & ~(QDAS_PLAN_COPY_INPUTS | QDAS_PLAN_NO_FOLD);
    const std::string keep = g_err;
    qdas_plan *child = nullptr;
    void *fb = nullptr, *yb = nullptr;
    if (qdas_plan_create(&child, &d) == QDAS_OK && child && child->kernel == QDAS_KERNEL_TILED && child->prefolded
        && plan_malloc(&fb, (size_t)z.T * z.N * z.M * 8) == hipSuccess && plan_malloc(&yb, (size_t)child->y_ld * 8 + 16) == hipSuccess
        && hipMemset(fb, 0, (size_t)z.T * z.N * z.M * 8) == hipSuccess) {
        pl->owned.push_back(fb); pl->owned.push_back(yb);
        pl->fold_buf = fb; pl->y32 = yb; pl->f16_child = child;
        pl->fold_wtab = pl->tp.wtab;               // (this plan's N x M table, float2: applied by the fold pass)
    } else {
        (void)hipGetLastError();
        if (fb) (void)hipFree(fb);
        if (yb) (void)hipFree(yb);
        if (child) qdas_plan_destroy(child);
    }
    g_err = keep;
}

// the instantiation this plan launches for one frame: libqdas.so carries it, or it is built now (das_tile_cfg.h tile_prebuilt, jit.hip lazy_tile_launch) --
// never inside an execute.  *no_compiler: the variant is missing and cannot be built (no libhiprtc.so, QDAS_NO_LAZY); g_err says which one it was.
static void plan_resolve_kernel(qdas_plan *pl, bool *no_compiler) {
    *no_compiler = false;
    if (!(pl->kernel == QDAS_KERNEL_TILED && !pl->jit_fn && !pl->f16_child)) return;      // (fp16 reciprocal data: the fp32 child plan resolved its own)
    std::string built;
    TileParams t1 = pl->tp;
    t1.nfr = 1;
    const hipError_t pe = prepare_tile(t1, pl->d.sz.dtype, pl->ntiles, &built);
    if (pe == hipErrorSharedObjectInitFailed) { *no_compiler = true; return; }
    if (pe != hipSuccess) (void)hipGetLastError();      // (anything else is the launch's to report)
    if (!built.empty()) pl->jit_tag = "built on demand " + built;
}

// step 5 of plan_modes.h (frames per launch of a stream), host staging, and what the plan must not keep
static int plan_finish(qdas_plan *pl, const qdas_desc *desc, const PlanBuild &b) {
    const qdas_sizes &z = pl->d.sz;
    const int dt = z.dtype;
    int rc;
    modes::PlanShape ps;
    ps.dtype = dt; ps.tiled = pl->kernel == QDAS_KERNEL_TILED; ps.sym = pl->tp.sym; ps.fold = pl->tp.fold; ps.mir = pl->tp.mir; ps.narrow = pl->tp.narrow; ps.big = pl->tp.big;
    ps.bf = pl->tp.bf; ps.syn = pl->tp.syn; ps.stage_shift = pl->tp.stage_shift; ps.has_apix = pl->tp.apix != nullptr; ps.has_wtab = pl->tp.wtab != nullptr;
    ps.has_bpix = pl->tp.bpix != nullptr; ps.gen_kind = pl->tp.gen_kind; ps.fmod = pl->tp.fmod; ps.N = pl->tp.N; ps.M = pl->tp.M; ps.mem_device = desc->mem == QDAS_MEM_DEVICE;
    const modes::StreamModes sm = modes::stream_modes(ps, z.N, z.M, b.sw);
    pl->fb2_ok = sm.fb2_ok; pl->fold2_ok = sm.fold2_ok; pl->fb4_off = sm.fb4_off;
    if (desc->mem == QDAS_MEM_HOST) {                   // staging buffers for x / y
        pl->x_bytes = (size_t)z.T * z.N * z.M * data_size(dt);
        pl->y_bytes = (size_t)pl->y_ld * pl->oN * pl->oM * data_size(dt);
        if ((rc = dev_alloc(pl, &pl->dx, pl->x_bytes))) return rc;
        if ((rc = dev_alloc(pl, &pl->dy, pl->y_bytes))) return rc;
    }
    // the plan keeps no pointer into caller memory it does not need: host arrays were copied; device arrays are used in place
    // (g.* / tp.*: they must stay valid for the life of the plan unless QDAS_PLAN_COPY_INPUTS made plan-owned copies)
    pl->mirror_bound = b.sy.mirror_bound; pl->recip_bound = b.sy.recip_bound;
    if (pl->fold_buf && !pl->f16_child && !(pl->kernel == QDAS_KERNEL_TILED && pl->tp.fold)) {      // (the plan left the fold after all: wide windows, strides, generic kernel)
        for (size_t k = 0; k < pl->owned.size(); ++k) if (pl->owned[k] == pl->fold_buf) { pl->owned.erase(pl->owned.begin() + (long)k); break; }
        (void)hipFree(pl->fold_buf);
        pl->fold_buf = nullptr;
    }
    pl->d.Pi = pl->d.Pr = pl->d.Pv = pl->d.Nv = pl->d.apod = pl->d.cinv = pl->d.rx_normals = nullptr;
    pl->d.acstride = nullptr;
    return QDAS_OK;
}

namespace qdas { modes::LaunchShape launch_shape(const TileParams &P, int dtype, bool jit); }      // das_tile.hip: the launcher's view of a parameter block

// The tile prologue's tables (window bases, extents, tile statistics: tile_params.h pro_tab) depend on the geometry only: computed ONCE per plan by the probe
// kernels -- the same prologue code, writing to a plan-owned buffer -- and loaded by every workgroup of every execute instead of being recomputed
// ((M + N) wave-wide reductions per wave and workgroup: 25 % of BASELINE C5's kernel time, ~10 % of C2's).  QDAS_NO_PRO_TAB=1: as before.
static int plan_cache_prologue(qdas_plan *pl) {
    TileParams &t = pl->tp;
    t.pro_tab = nullptr; t.pro_out = nullptr;
    if (getenv("QDAS_NO_PRO_TAB") || !pl->ntiles) return QDAS_OK;
    t.pro_mask = 0;
    const bool with_mask = t.act_bytes != 0 && !getenv("QDAS_NO_PRO_MASK");      // (a stage list: the tile's activity mask rides behind the statistics, plan_cache_activity)
    const size_t stride = 2 * ((size_t)t.M + t.N) + 8 + (with_mask ? (t.N + 31) / 32 : 0), bytes = (size_t)pl->ntiles * stride * sizeof(float);
    if (bytes > (1ull << 30)) return QDAS_OK;           // (thousands of elements x tens of thousands of tiles: not worth a GiB)
    void *buf = nullptr;
    if (plan_malloc(&buf, bytes) != hipSuccess) { (void)hipGetLastError(); return QDAS_OK; }      // (no memory for it: the kernels compute their tables themselves)
    pl->owned.push_back(buf);
    TileParams p = t;
    p.probe = 1; p.x = nullptr; p.y = nullptr; p.wtab = nullptr; p.apix = nullptr; p.pro_out = (float *)buf; p.pro_mask = with_mask ? 1 : 0;
    HIPCHK(hipMemsetAsync(buf, 0, bytes, 0));
    const hipError_t e = launch_tile(p, pl->d.sz.dtype, pl->ntiles, nullptr);
    if (e != hipSuccess) { (void)hipGetLastError(); return QDAS_OK; }      // (a configuration without a probe kernel: as before)
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemset(pl->fallback, 0, sizeof(uint32_t)));      // (the probe re-listed the misfit tiles: the frame kernels list them per launch)
    t.pro_tab = (const float *)buf;
    t.pro_mask = with_mask ? 3 : 0;                     // (3: room for the masks, not yet written -- plan_cache_activity, once the plan's kernel is resolved)
    return QDAS_OK;
}

// The tiles' activity masks (tile_params.h pro_mask): ONE launch of the plan's own kernel in mask mode -- every tile tests all its stage elements with exactly
// the rule the frames use (array / generated / side weights, the mirror image's share) and stores the mask; the frame kernels then load it instead of
// re-loading up to N weights per lane, workgroup and execute.  Any failure: the plan runs without the tables.
static void plan_cache_activity(qdas_plan *pl) {
    TileParams &t = pl->tp;
    if (pl->kernel != QDAS_KERNEL_TILED || t.pro_mask != 3) return;
    TileParams p = t;
    p.nfr = 1; p.x = nullptr; p.y = nullptr; p.ksplit = 1; p.ksplit_m = 1; p.part = nullptr; p.pro_mask = 2; p.pro_out = const_cast<float *>(t.pro_tab);
    const std::string keep = g_err;
    hipError_t e = launch_tile(p, pl->d.sz.dtype, pl->ntiles, nullptr, pl->jit_fn, pl->jit_lds);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess && !pl->no_fallback) e = hipMemset(pl->fallback, 0, sizeof(uint32_t));
    g_err = keep;
    if (e == hipSuccess) t.pro_mask = 1;
    else { (void)hipGetLastError(); t.pro_mask = 0; t.pro_tab = nullptr; }      // (the table's stride counted the masks: without them, no table)
}

// the tiled kernel's side of a plan: parameter block, weights, probed shape, split aperture -- then checked against the model of plan_modes.h
static int plan_build_tiled(qdas_plan *pl, const qdas_desc *desc, PlanBuild &b) {
    int rc;
    if ((rc = plan_setup_tile_params(pl, desc, b))) return rc;
    if ((rc = plan_pixel_weights(pl, desc, b))) return rc;
    if ((rc = plan_weight_table(pl, desc, b))) return rc;
    if ((rc = plan_probe_chain(pl, desc, b))) return rc;
    if ((rc = plan_side_split(pl, desc, b))) return rc;
    if ((rc = plan_wide_windows(pl, desc, b))) return rc;
    if ((rc = plan_stage_shape(pl, desc, b))) return rc;
    if ((rc = plan_split_aperture(pl, b))) return rc;
    if ((rc = plan_cache_prologue(pl))) return rc;
    b.outcome.ksplit = pl->tp.ksplit;
    const modes::LaunchShape model = modes::derive_launch_shape(*desc, b.rq, b.sy, b.outcome), built = launch_shape(pl->tp, pl->d.sz.dtype, false);
    if (const char *f = modes::shape_mismatch(model, built))
        return fail(QDAS_EINVAL, "internal: the built plan differs from the mode model of plan_modes.h in '%s' -- please report the descriptor", f);
    return QDAS_OK;
}

static int plan_create_impl(qdas_plan *pl, qdas_plan **out, const qdas_desc *desc, bool *replaced) {
    *replaced = false;
    int rc = plan_init(pl, desc);
    if (rc) return rc;
    const qdas_sizes &z = pl->d.sz;
    DeviceGuard guard(desc->device);
    if (guard.err != hipSuccess) return fail(QDAS_EHIP, "hipSetDevice(%d): %s", desc->device, hipGetErrorString(guard.err));
    { hipError_t e = hipGetDevice(&pl->device); if (e != hipSuccess) return fail(QDAS_EHIP, "hipGetDevice: %s", hipGetErrorString(e)); }
    if (pl->I == 0 || z.N == 0 || z.M == 0) return QDAS_OK;   // empty problem: execute() just zero-fills
    if ((desc->plan_flags & QDAS_PLAN_PREFOLDED) && z.S > 0)      // (a prefolded plan runs no fold pass: nothing would apply the table -- include/qdas.h QDAS_PLAN_PREFOLDED)
        return fail(QDAS_EUNSUPPORTED, "QDAS_PLAN_PREFOLDED: apodization arrays belong to the fold (qdas_fold_desc.wtab), not to the plan that is handed folded frames");
    PlanBuild b;
    b.desc = desc;
    b.sw = read_switches();
    if ((rc = plan_import_inputs(pl, desc, b))) return rc;
    if ((rc = plan_resolve_modes(pl, desc, b))) return rc;
    if (pl->kernel == QDAS_KERNEL_TILED && (rc = plan_build_tiled(pl, desc, b))) return rc;
    const bool mslab = (desc->plan_flags & QDAS_PLAN_MIRROR_SLAB) != 0;
    if (mslab && !(pl->kernel == QDAS_KERNEL_TILED && pl->tp.mir == 2))
        return fail(QDAS_EUNSUPPORTED, "QDAS_PLAN_MIRROR_SLAB: the lateral-mirror mode is not available for this problem (geometry not mirror-symmetric "
                                       "about x = 0, weights / modes it does not take, or tiles that do not fit the staging windows): use plain slabs");
    int remake = 0;
    if ((rc = plan_jit(pl, desc, &remake))) return rc;
    if (remake) {                                       // the plan's mode exists only as a hiprtc build, which failed: the same plan without the mode
        qdas_desc d2 = *desc;
        d2.plan_flags |= remake;
        const std::string keep = g_err;
        *replaced = true;
        const int rc2 = qdas_plan_create(out, &d2);
        if (rc2 == QDAS_OK) g_err = keep;
        return rc2;
    }
    if (pl->prefolded && pl->kernel == QDAS_KERNEL_TILED && !pl->no_fallback)
        return fail(QDAS_EUNSUPPORTED, "QDAS_PLAN_PREFOLDED: tiles of this image do not fit the staging windows (they would be redone from the unfolded frame)");
    plan_f16_child(pl, desc);
    bool no_compiler = false;
    plan_resolve_kernel(pl, &no_compiler);
    if (no_compiler) {                                  // re-made on the generic kernel (identical semantics, 5-12x slower), or an error when the caller insisted on the fused kernel
        const std::string why = g_err;
        if (desc->kernel == QDAS_KERNEL_TILED || mslab || pl->prefolded) return fail(QDAS_EUNSUPPORTED, "%s", why.c_str());
        qdas_desc d2 = *desc;
        d2.kernel = QDAS_KERNEL_GENERIC;
        *replaced = true;
        const int rc2 = qdas_plan_create(out, &d2);
        if (rc2 == QDAS_OK) g_err = why + " -- using the generic kernel";
        return rc2;
    }
    plan_cache_activity(pl);
    return plan_finish(pl, desc, b);
}

extern "C" int qdas_plan_create(qdas_plan **out, const qdas_desc *desc) {
    if (!out || !desc) return fail(QDAS_EINVAL, "null argument");
    *out = nullptr;
    int rc = validate(desc);
    if (rc) return rc;
    qdas_plan *pl = new qdas_plan();
    bool replaced = false;
    rc = plan_create_impl(pl, out, desc, &replaced);
    if (rc || replaced) { delete pl; return rc; }      // (replaced: *out holds the plan that was made in this one's stead)
    *out = pl;
    return QDAS_OK;
}

extern "C" void qdas_plan_destroy(qdas_plan *pl) {
    if (!pl) return;
    DeviceGuard guard(pl->device);
    delete pl;
}

extern "C" int qdas_plan_kernel(const qdas_plan *pl) { return pl ? pl->kernel : 0; }

extern "C" int qdas_plan_fallback_tiles(const qdas_plan *pl, uint64_t *n) {
    if (!pl || !n) return fail(QDAS_EINVAL, "null argument");
    if (pl->f16_child) return qdas_plan_fallback_tiles(pl->f16_child, n);
    *n = 0;
    if (pl->kernel != QDAS_KERNEL_TILED || !pl->fallback) return QDAS_OK;
    uint32_t c = 0;
    HIPCHK(hipMemcpy(&c, pl->fallback, sizeof c, hipMemcpyDeviceToHost));
    *n = c;
    return QDAS_OK;
}

extern "C" int qdas_plan_tile_shape(const qdas_plan *pl, int *tile_z, int *tile_cols, int *wave_z, int *ksplit) {
    if (!pl || !tile_z || !tile_cols) return fail(QDAS_EINVAL, "null argument");
    if (pl->f16_child) return qdas_plan_tile_shape(pl->f16_child, tile_z, tile_cols, wave_z, ksplit);
    const bool tiled = pl->kernel == QDAS_KERNEL_TILED;
    *tile_z = tiled ? (1 << pl->tp.tz_log2) : 0;
    *tile_cols = tiled ? (int)pl->tile_cols : 0;
    if (wave_z) *wave_z = tiled ? (1 << pl->tp.wz_log2) : 0;
    if (ksplit) *ksplit = tiled ? (int)pl->tp.ksplit : 0;
    return QDAS_OK;
}

extern "C" int qdas_plan_mirror(const qdas_plan *pl) { if (pl && pl->f16_child) return qdas_plan_mirror(pl->f16_child); return pl && pl->kernel == QDAS_KERNEL_TILED && pl->tp.mir ? 1 : 0; }

extern "C" int qdas_plan_reciprocal(const qdas_plan *pl) { return pl && pl->kernel == QDAS_KERNEL_TILED && pl->tp.sym ? 1 : 0; }

extern "C" int qdas_plan_symmetry_bound(const qdas_plan *pl, double *mirror_samples, double *reciprocal_samples) {
    if (!pl) return fail(QDAS_EINVAL, "null plan");
    if (pl->f16_child) return qdas_plan_symmetry_bound(pl->f16_child, mirror_samples, reciprocal_samples);
    const bool tiled = pl->kernel == QDAS_KERNEL_TILED;
    if (mirror_samples) *mirror_samples = (tiled && pl->tp.mir) ? pl->mirror_bound : -1.0;
    if (reciprocal_samples) *reciprocal_samples = (tiled && pl->tp.sym) ? pl->recip_bound : -1.0;
    return QDAS_OK;
}

extern "C" int qdas_plan_folded(const qdas_plan *pl) { if (pl && pl->f16_child) return 1; return pl && pl->kernel == QDAS_KERNEL_TILED && pl->tp.fold ? 1 : 0; }

// ---- the reciprocity fold as an entry of its own (qdas.h): for hosts that fold once and hand folded frames to QDAS_PLAN_PREFOLDED plans
extern "C" int qdas_fold(const qdas_fold_desc *d, const void *x, void *xs, void *stream) {
    if (!d || !x || !xs) return fail(QDAS_EINVAL, "null argument");
    if (d->dtype != QDAS_F32 && d->dtype != QDAS_F16) return fail(QDAS_EINVAL, "qdas_fold: complex64 or complex32 (fp16) frames");
    if (d->N > 65535) return fail(QDAS_EUNSUPPORTED, "qdas_fold: at most 65535 elements");
    DeviceGuard guard(d->device);
    HIPCHK(guard.err);
    HIPCHK(launch_fold(x, xs, d->wtab, d->T, d->N, d->strN ? d->strN : d->T, d->strM ? d->strM : d->T * d->N, (hipStream_t)stream, d->dtype == QDAS_F16));
    return QDAS_OK;
}

extern "C" int qdas_plan_kernel_name(const qdas_plan *pl, char *buf, size_t len) {
    if (!pl || !buf || !len) return fail(QDAS_EINVAL, "null argument");
    if (pl->f16_child) {                                // "das_tile_kernel<interp=3,f16>f32,sym,fold,...": fp16 data on the folded fp32 kernels
        char tmp[256];
        int rc = qdas_plan_kernel_name(pl->f16_child, tmp, sizeof tmp);
        if (rc) return rc;
        std::string nm(tmp);
        const size_t at = nm.find(",f32");
        if (at != std::string::npos) nm.replace(at, 4, ",f16>f32");
        if (pl->fold_wtab && nm.find(",wtab") == std::string::npos) { const size_t f = nm.find(",fold"); if (f != std::string::npos) nm.insert(f + 5, ",wtab"); }
        snprintf(buf, len, "%s", nm.c_str());
        return QDAS_OK;
    }
    const qdas_sizes &z = pl->d.sz;
    const char *dts = z.dtype == QDAS_F64 ? "f64" : (z.dtype == QDAS_F32 ? "f32" : "f16");
    if (pl->kernel == QDAS_KERNEL_TILED) {
        const TileParams &t = pl->tp;
        snprintf(buf, len, "das_tile_kernel<interp=%d,%s%s%s%s%s%s%s,mb=%d,W=%d> [%s]", z.flag & 7, dts, t.sym ? ",sym" : "", t.fold ? ",fold" : "", t.fmod != 0.0 ? ",fmod" : "",
                 (t.wtab || (t.fold && pl->fold_wtab)) ? ",wtab" : "", t.big ? ",big" : "", t.mir ? ",mirror" : ((t.St && !t.syn) ? ",roles swapped" : ""), pl->jit_fn ? pl->jit_mb : pl->tc.mb, (pl->jit_fn && pl->jit_w) ? pl->jit_w : pl->tc.window, pl->jit_tag.empty() ? "prebuilt" : pl->jit_tag.c_str());
    } else snprintf(buf, len, "das_generic_kernel<interp=%d,%s>", z.flag & 7, dts);
    return QDAS_OK;
}

extern "C" int qdas_plan_set_timing(qdas_plan *pl, int enable) {
    if (!pl) return fail(QDAS_EINVAL, "null plan");
    pl->timing = enable != 0;
    if (pl->timing && !pl->e0) { HIPCHK(hipEventCreate(&pl->e0)); HIPCHK(hipEventCreate(&pl->e1)); }
    return QDAS_OK;
}

extern "C" int qdas_plan_last_kernel_ms(const qdas_plan *pl, float *ms) {
    if (!pl || !ms) return fail(QDAS_EINVAL, "null argument");
    *ms = pl->last_ms;
    return QDAS_OK;
}

static int hip_rc(hipError_t e) { HIPCHK(e); return QDAS_OK; }

// One frame -- or, for the tiled kernel outside the reciprocal mode, TWO frames in one launch (nf == 2): frame 1 lives at
// x + x_fstride bytes / y + y_fstride elements and shares tap indices and weights with frame 0 (das_tile_impl.h "FB2").
static int run_frame(qdas_plan *pl, const void *x, void *y, hipStream_t s, int nf = 1, uint64_t x_fstride = 0, uint64_t y_fstride = 0) {
    const qdas_sizes &z = pl->d.sz;
    if (pl->f16_child && nf == 1) {                     // fp16 reciprocal data: fold into complex64, the folded fp32 kernels, round the image to complex32
        const TileParams &c = pl->f16_child->tp;
        HIPCHK(launch_fold(x, pl->fold_buf, pl->fold_wtab, z.T, z.N, c.strN, c.strM, s, 1));
        int rc = run_frame(pl->f16_child, pl->fold_buf, pl->y32, s);
        if (rc) return rc;
        HIPCHK(launch_y32_to_y16(pl->y32, y, pl->f16_child->y_ld, s));
        return QDAS_OK;
    }
    if (pl->kernel == QDAS_KERNEL_TILED) {
        TileParams t = pl->tp;
        t.x = x; t.y = y;
        t.nfr = nf; t.x_fstride = x_fstride; t.y_fstride = y_fstride;
        if (t.fold && pl->prefolded) {                  // (the caller folded the frames: qdas_fold)
            if (!pl->no_fallback) return fail(QDAS_EUNSUPPORTED, "QDAS_PLAN_PREFOLDED: tiles of this image do not fit the staging windows and would need the unfolded frame");
        } else if (t.fold) {                            // the reciprocity fold of this frame (fold.hip): one pass over HBM, then the fused kernel on the folded copy
            HIPCHK(launch_fold(x, pl->fold_buf, pl->fold_wtab, z.T, z.N, t.strN, t.strM, s));
            t.x = pl->fold_buf;
            if (nf == 2) {                              // (two frames per launch: the second frame's folded copy; the kernel reads it x_fstride BYTES after the first)
                if (!pl->fold_buf2) return fail(QDAS_EINVAL, "internal: no second fold buffer");
                HIPCHK(launch_fold((const char *)x + x_fstride, pl->fold_buf2, pl->fold_wtab, z.T, z.N, t.strN, t.strM, s));
                t.x_fstride = (uint64_t)((intptr_t)pl->fold_buf2 - (intptr_t)pl->fold_buf);      // (modulo 2^64: the kernel adds it to the base pointer)
            }
        }
        if (t.syn) {                                    // planes are accumulated with atomics: start from zero
            const size_t ds = data_size(z.dtype);        // (only this plan's pixels of every plane: y_ld may span a full-size buffer)
            for (int f = 0; f < nf; ++f)
                HIPCHK(hipMemset2DAsync((char *)y + (size_t)f * y_fstride * ds, (size_t)pl->y_ld * ds, 0, (size_t)pl->i_count * ds, pl->oN * pl->oM, s));
        }
        // (frames that share a launch run the prebuilt two- / four-frame kernels also in plans with a hiprtc build: shared tap indices and
        //  weights are worth more than the specialisation -- C2: 1.49 ms per frame in pairs, 1.64 ms one by one on the hiprtc build)
        const hipFunction_t jf = nf == 1 ? pl->jit_fn : nullptr;
        if (pl->no_fallback) return hip_rc(launch_tile(t, z.dtype, pl->ntiles, s, jf, pl->jit_lds));     // one launch per frame (+ the reduce of a split aperture)
        HIPCHK(hipMemsetAsync(pl->fallback, 0, sizeof(uint32_t), s));
        HIPCHK(launch_tile(t, z.dtype, pl->ntiles, s, jf, pl->jit_lds));
        // tiles whose delay window overflowed LDS are redone by the generic kernel; the launch is
        // sized for the worst case and exits immediately for ids >= the device-side count
        GenericParams g = pl->gp;
        g.x = x; g.y = y; g.y_ld = pl->y_ld;
        g.tile_list = pl->fallback;
        g.tile_cols = pl->tile_cols;
        g.tile_zl = (uint32_t)pl->tp.tz_log2;
        g.blocks_per_tile = (64 * pl->tc.waves + 255) / 256;
        g.tiles_z = pl->tp.tiles_z;
        HIPCHK(launch_generic(g, z.dtype, pl->ntiles * g.blocks_per_tile, s));
        for (int f = 1; f < nf; ++f) {                  // the same misfit tiles of the other frames of the launch
            g.x = (const char *)x + (size_t)f * x_fstride; g.y = (char *)y + (size_t)f * y_fstride * data_size(z.dtype);
            HIPCHK(launch_generic(g, z.dtype, pl->ntiles * g.blocks_per_tile, s));
        }
    } else {
        GenericParams g = pl->gp;
        g.x = x; g.y = y;
        HIPCHK(launch_generic(g, z.dtype, (unsigned)((pl->i_count + 255) / 256), s));
    }
    return QDAS_OK;
}

// One-time preparations of a STREAM of F frames (twin plan, second folded copy, frame-sharing instantiations, host staging): everything that allocates,
// compiles or synchronises.  qdas_plan_execute_frames runs it at the plan's first stream; qdas_plan_prepare_frames lets a caller run it ahead of time, so that
// the stream calls themselves only enqueue work (graph capture, latency-critical first frames).  Idempotent.
static int prepare_stream(qdas_plan *pl, uint64_t F, hipStream_t s) {
    const qdas_sizes &z = pl->d.sz;
    if (pl->I == 0 || z.N == 0 || z.M == 0 || pl->i_count == 0 || z.T == 0 || F < 2) return QDAS_OK;
    // a stream of >= 4 device-resident frames through a general-mode lateral-mirror plan: four frames per launch on the plan's twin
    if (F >= 4 && pl->kernel == QDAS_KERNEL_TILED && pl->tp.mir == 1 && !pl->tp.sym && !pl->tp.apix && !pl->tp.gen_kind && pl->d.mem == QDAS_MEM_DEVICE
        && !getenv("QDAS_NO_FB4") && !getenv("QDAS_NO_FB2") && !getenv("QDAS_NO_FRAMES_TWIN") && !pl->twin_tried) {
        pl->twin_tried = true;
        qdas_desc d = pl->d;                            // (the plan's own device copies / the caller's device arrays: both stay valid for the plan's life)
        const GenericParams &g = pl->gp;
        uint64_t acs[6 * (1 + QDAS_MAX_APOD)];
        memcpy(acs, g.cst, sizeof g.cst); memcpy(acs + 6, g.ast, sizeof(uint64_t) * 6 * z.S);
        d.Pi = g.Pi; d.Pr = g.Pr; d.Pv = g.Pv; d.Nv = g.Nv; d.cinv = g.cinv; d.apod = g.apod; d.rx_normals = g.rxn; d.acstride = acs;
        d.mem = QDAS_MEM_DEVICE; d.device = pl->device;
        d.plan_flags = (d.plan_flags | QDAS_PLAN_NO_MIRROR) & ~(QDAS_PLAN_COPY_INPUTS | QDAS_PLAN_JIT | QDAS_PLAN_MIRROR_SLAB);
        const std::string keep = g_err;
        if (qdas_plan_create(&pl->frames_twin, &d) != QDAS_OK) pl->frames_twin = nullptr;
        else if (!(pl->frames_twin->fb2_ok && !pl->frames_twin->fb4_off)) { qdas_plan_destroy(pl->frames_twin); pl->frames_twin = nullptr; }
        g_err = keep;
    }
    if (pl->frames_twin && F >= 4) return prepare_stream(pl->frames_twin, F, s);
    // folded data: frame pairs share a launch; the second folded copy is made now (once)
    if (pl->fold2_ok && !pl->prefolded && !pl->fold_buf2) {
        const size_t fb = (size_t)z.T * z.N * z.M * 8;
        void *p2 = nullptr;
        if (plan_malloc(&p2, fb) == hipSuccess) {
            pl->owned.push_back(p2);
            if (hipMemsetAsync(p2, 0, fb, s) == hipSuccess) pl->fold_buf2 = p2;
        } else (void)hipGetLastError();
        if (!pl->fold_buf2) pl->fold2_ok = false;       // (no memory for it: one frame per launch)
    }
    // the frame-sharing instantiations are resolved (built on demand when libqdas.so does not carry them) here, not inside the frame loop; without a
    // compiler the stream runs one frame per launch
    if ((pl->fb2_ok || pl->fold2_ok) && pl->kernel == QDAS_KERNEL_TILED) {
        const std::string keep = g_err;
        for (int nf = 2; nf <= 4; nf += 2) {
            bool &done = nf == 2 ? pl->prep2 : pl->prep4;
            if (done || (nf == 4 && (F < 4 || pl->fb4_off || pl->tp.fold))) continue;
            done = true;
            TileParams t = pl->tp;
            t.nfr = nf;
            if (prepare_tile(t, z.dtype, pl->ntiles, nullptr) == hipErrorSharedObjectInitFailed) {
                if (nf == 2) { pl->fb2_ok = false; pl->fold2_ok = false; } else pl->fb4_off = true;
            }
            (void)hipGetLastError();
        }
        g_err = keep;
    }
    if (pl->d.mem == QDAS_MEM_HOST && !pl->copy_stream) {      // host frames: a second staging set + copy stream (frame f+1 is uploaded while f is beamformed)
        int rc;
        if ((rc = dev_alloc(pl, &pl->dx2, pl->x_bytes)) || (rc = dev_alloc(pl, &pl->dy2, pl->y_bytes))) return rc;
        HIPCHK(hipStreamCreateWithFlags(&pl->copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIPCHK(hipEventCreateWithFlags(&pl->ex[k], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&pl->ek[k], hipEventDisableTiming));
        }
    }
    return QDAS_OK;
}

extern "C" int qdas_plan_prepare_frames(qdas_plan *pl, uint64_t F) {
    if (!pl) return fail(QDAS_EINVAL, "null plan");
    DeviceGuard guard(pl->device);
    HIPCHK(guard.err);
    int rc = prepare_stream(pl, F, nullptr);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    return QDAS_OK;
}

// host-resident frames: upload f+1 on the copy stream while f is beamformed
static int stream_host_frames(qdas_plan *pl, const void *x, void *y, uint64_t F, uint64_t x_stride, uint64_t y_stride, hipStream_t s) {
    const size_t ds = data_size(pl->d.sz.dtype);
    void *dxs[2] = {pl->dx, pl->dx2}, *dys[2] = {pl->dy, pl->dy2};
    hipStream_t sc = pl->copy_stream;
    HIPCHK(hipMemcpyAsync(dxs[0], x, pl->x_bytes, hipMemcpyHostToDevice, sc));
    HIPCHK(hipEventRecord(pl->ex[0], sc));
    for (uint64_t f = 0; f < F; ++f) {
        const int b = (int)(f & 1), nb = b ^ 1;
        HIPCHK(hipStreamWaitEvent(s, pl->ex[b], 0));
        int rc = run_frame(pl, dxs[b], dys[b], s);
        if (rc) return rc;
        HIPCHK(hipEventRecord(pl->ek[b], s));
        if (f + 1 < F) {                                // the other buffer's last reader was frame f-1
            if (f >= 1) HIPCHK(hipStreamWaitEvent(sc, pl->ek[nb], 0));
            HIPCHK(hipMemcpyAsync(dxs[nb], (const char *)x + (f + 1) * x_stride * ds, pl->x_bytes, hipMemcpyHostToDevice, sc));
            HIPCHK(hipEventRecord(pl->ex[nb], sc));
        }
        HIPCHK(hipMemcpyAsync((char *)y + f * y_stride * ds, dys[b], pl->y_bytes, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipStreamSynchronize(sc));
    return QDAS_OK;
}

static int stop_timer(qdas_plan *pl, hipStream_t s) {
    if (!pl->timing) return QDAS_OK;
    HIPCHK(hipEventRecord(pl->e1, s));
    HIPCHK(hipEventSynchronize(pl->e1));
    HIPCHK(hipEventElapsedTime(&pl->last_ms, pl->e0, pl->e1));
    return QDAS_OK;
}

extern "C" int qdas_plan_execute_frames(qdas_plan *pl, const void *x, void *y, uint64_t F, uint64_t x_stride,
                                        uint64_t y_stride, void *stream) {
    if (!pl) return fail(QDAS_EINVAL, "null plan");
    if (F == 0) return QDAS_OK;
    if (!y) return fail(QDAS_EINVAL, "null output");
    const qdas_sizes &z = pl->d.sz;
    const size_t ds = data_size(z.dtype);
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard guard(pl->device);
    HIPCHK(guard.err);
    const size_t ybytes = (size_t)pl->y_ld * pl->oN * pl->oM * ds;
    if (pl->I == 0 || z.N == 0 || z.M == 0 || pl->i_count == 0 || z.T == 0) {      // empty sum: zeros
        for (uint64_t f = 0; f < F && ybytes; ++f) {
            char *yf = (char *)y + f * y_stride * ds;
            if (pl->d.mem == QDAS_MEM_HOST) memset(yf, 0, ybytes);
            else HIPCHK(hipMemsetAsync(yf, 0, ybytes, s));
        }
        return QDAS_OK;
    }
    if (!x) return fail(QDAS_EINVAL, "null data");
    if (pl->timing) HIPCHK(hipEventRecord(pl->e0, s));
    int rc = prepare_stream(pl, F, s);                  // (a no-op after the plan's first stream, or after qdas_plan_prepare_frames)
    if (rc) return rc;
    if (F >= 4 && pl->frames_twin) {
        // the WHOLE stream goes through the twin (groups of four, then a pair, then a single frame on its own kernels): every frame of
        // one call is summed in the same order -- round 3 sent the tail through the mirror kernel.  The images equal
        // qdas_plan_execute's to fp32 re-association, not bit for bit (another kernel): include/qdas.h says so.
        pl->frames_twin->timing = false;
        rc = qdas_plan_execute_frames(pl->frames_twin, x, y, F, x_stride, y_stride, stream);
        return rc ? rc : stop_timer(pl, s);
    }
    // frame pairs share one launch (device-resident data, tiled kernel; QDAS_NO_FB2 disables); folded data: the caller's folded frames as they lie
    // (prefolded plans), or the plan's two folded copies
    bool pairs_ok = pl->fb2_ok && x_stride * ds < (1ull << 40);
    if (pl->fold2_ok && F >= 2) pairs_ok = pl->prefolded ? x_stride * ds < (1ull << 40) : pl->fold_buf2 != nullptr;
    if (pl->d.mem == QDAS_MEM_HOST && F >= 2) {
        rc = stream_host_frames(pl, x, y, F, x_stride, y_stride, s);
        return rc ? rc : stop_timer(pl, s);
    }
    for (uint64_t f = 0; f < F; ++f) {
        const char *xf = (const char *)x + f * x_stride * ds;
        char *yf = (char *)y + f * y_stride * ds;
        if (pairs_ok && f + 1 < F) {                    // four (else two) frames share a launch
            const int nf = (f + 3 < F && !pl->fb4_off && !pl->tp.fold) ? 4 : 2;
            rc = run_frame(pl, xf, yf, s, nf, x_stride * ds, y_stride);
            if (rc) return rc;
            f += nf - 1;
            continue;
        }
        if (pl->d.mem == QDAS_MEM_HOST) {
            HIPCHK(hipMemcpyAsync(pl->dx, xf, pl->x_bytes, hipMemcpyHostToDevice, s));
            rc = run_frame(pl, pl->dx, pl->dy, s);
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(yf, pl->dy, pl->y_bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        } else {
            rc = run_frame(pl, xf, yf, s);
            if (rc) return rc;
        }
    }
    return stop_timer(pl, s);
}

extern "C" int qdas_plan_execute(qdas_plan *pl, const void *x, void *y, void *stream) {
    return qdas_plan_execute_frames(pl, x, y, 1, 0, 0, stream);
}

extern "C" int qdas_plan_delays(qdas_plan *pl, void *tau, void *stream) {
    if (!pl || !tau) return fail(QDAS_EINVAL, "null argument");
    const qdas_sizes &z = pl->d.sz;
    if (pl->I == 0 || z.N == 0 || z.M == 0 || pl->i_count == 0) return QDAS_OK;
    DeviceGuard guard(pl->device);
    HIPCHK(guard.err);
    hipStream_t s = (hipStream_t)stream;
    const size_t rs = real_size(z.dtype);
    const double cinv = pl->cinv0;                     // (read at plan creation: the caller's arrays are not touched after it)
    GenericParams g = pl->gp;
    g.y_ld = pl->i_count;
    const size_t bytes = (size_t)pl->i_count * z.N * z.M * rs;
    if (pl->d.mem == QDAS_MEM_HOST) {
        void *dt;
        HIPCHK(plan_malloc(&dt, bytes));
        hipError_t e = launch_delays(g, z.dtype == QDAS_F64 ? 0 : 1, dt, cinv, s);
        if (e == hipSuccess) e = hipMemcpyAsync(tau, dt, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(dt);
        if (e != hipSuccess) return fail(QDAS_EHIP, "delays: %s", hipGetErrorString(e));
    } else {
        HIPCHK(launch_delays(g, z.dtype == QDAS_F64 ? 0 : 1, tau, cinv, s));
    }
    return QDAS_OK;
}

// ------------------------------------------------------------------------------------ one-shot entries
static int one_shot(const qdas_sizes *sz, int dtype, void *y, const void *Pi, const void *Pr, const void *Pv, const void *Nv,
                    const void *a, const void *cinv, const uint64_t *acs, const void *x, double fs, double fmod, void *stream) {
    if (!sz) return fail(QDAS_EINVAL, "null sizes");
    qdas_desc d{};
    d.sz = *sz;
    d.sz.dtype = dtype;
    d.fs = fs; d.fmod = fmod;
    d.Pi = Pi; d.Pr = Pr; d.Pv = Pv; d.Nv = Nv; d.apod = a; d.cinv = cinv; d.acstride = acs;
    d.mem = QDAS_MEM_DEVICE; d.device = -1; d.kernel = QDAS_KERNEL_AUTO;
    // qdas_plan_create reads the geometry, the weights and cinv on the NULL stream, which is not ordered with a non-blocking `stream`: whatever the caller queued
    // there to produce them has to be done first (the call waits for `stream` at its end anyway)
    if (stream) { hipError_t e = hipStreamSynchronize((hipStream_t)stream); if (e != hipSuccess) return fail(QDAS_EHIP, "sync: %s", hipGetErrorString(e)); }
    qdas_plan *pl = nullptr;
    int rc = qdas_plan_create(&pl, &d);
    if (rc) return rc;
    rc = qdas_plan_execute(pl, x, y, stream);
    if (!rc) { hipError_t e = hipStreamSynchronize((hipStream_t)stream); if (e != hipSuccess) rc = fail(QDAS_EHIP, "sync: %s", hipGetErrorString(e)); }
    qdas_plan_destroy(pl);
    return rc;
}

extern "C" int qdas_DAS(const qdas_sizes *sz, void *y, const double *Pi, const double *Pr, const double *Pv, const double *Nv,
                        const void *a, const double *cinv, const uint64_t *acs, const void *x, const double tv[2], void *stream) {
    if (!tv) return fail(QDAS_EINVAL, "null tvars");
    return one_shot(sz, QDAS_F64, y, Pi, Pr, Pv, Nv, a, cinv, acs, x, tv[0], tv[1], stream);
}
extern "C" int qdas_DASf(const qdas_sizes *sz, void *y, const float *Pi, const float *Pr, const float *Pv, const float *Nv,
                         const void *a, const float *cinv, const uint64_t *acs, const void *x, const float tv[2], void *stream) {
    if (!tv) return fail(QDAS_EINVAL, "null tvars");
    return one_shot(sz, QDAS_F32, y, Pi, Pr, Pv, Nv, a, cinv, acs, x, tv[0], tv[1], stream);
}
extern "C" int qdas_DASh(const qdas_sizes *sz, void *y, const float *Pi, const float *Pr, const float *Pv, const float *Nv,
                         const void *a, const float *cinv, const uint64_t *acs, const void *x, const float tv[2], void *stream) {
    if (!tv) return fail(QDAS_EINVAL, "null tvars");
    return one_shot(sz, QDAS_F16, y, Pi, Pr, Pv, Nv, a, cinv, acs, x, tv[0], tv[1], stream);
}

static int delays_one_shot(const qdas_sizes *sz, int dtype, void *tau, const void *Pi, const void *Pr, const void *Pv,
                           const void *Nv, double cinv, void *stream) {
    if (!sz || !tau) return fail(QDAS_EINVAL, "null argument");
    GenericParams g{};
    g.Pi = Pi; g.Pr = Pr; g.Pv = Pv; g.Nv = Nv;
    g.N = sz->N; g.M = sz->M; g.I1 = sz->I1; g.I2 = sz->I2; g.I3 = sz->I3;
    g.i_begin = 0; g.i_count = sz->I1 * sz->I2 * sz->I3; g.y_ld = g.i_count;
    g.VS = sz->VS; g.DV = sz->DV;
    if (g.i_count == 0 || g.N == 0 || g.M == 0) return QDAS_OK;
    if (!Pi || !Pr || !Pv || !Nv) return fail(QDAS_EINVAL, "null geometry pointer");
    HIPCHK(launch_delays(g, dtype, tau, cinv, (hipStream_t)stream));
    return QDAS_OK;
}
extern "C" int qdas_delays(const qdas_sizes *sz, double *tau, const double *Pi, const double *Pr, const double *Pv,
                           const double *Nv, double cinv, void *stream) {
    return delays_one_shot(sz, 0, tau, Pi, Pr, Pv, Nv, cinv, stream);
}
extern "C" int qdas_delaysf(const qdas_sizes *sz, float *tau, const float *Pi, const float *Pr, const float *Pv,
                            const float *Nv, float cinv, void *stream) {
    return delays_one_shot(sz, 1, tau, Pi, Pr, Pv, Nv, cinv, stream);
}
