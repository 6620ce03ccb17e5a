// staging.hip -- host -> device staging (host side and one copy kernel): the library's own synchronous upload (qdas_internal_upload, api_util.h) and the
// recycled device buffers of host callers of the device-pointer entries (qdas_device_malloc / free / trim / copy, include/qdas.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "api_util.h"
#include "qdas_kernels.h"

using namespace qdas;

// Host -> device, synchronous, for the library's own (mostly small) uploads: staged in pinned memory and written by a KERNEL -- whatever sits between a
// copy-engine (or CPU) write into freshly allocated memory and the kernel launched behind it (see csrc/scratch.hip for what was seen on this platform), a
// write issued by the shader engines goes through the same translation and caches as the reads that follow it.
__global__ void __launch_bounds__(256) upload_kernel(unsigned char *__restrict__ dst, const unsigned char *__restrict__ src, size_t bytes) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n16 = bytes / 16;
    if (((uintptr_t)dst & 15u) == 0) {
        if (i < n16) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
        if (i < bytes - 16 * n16) dst[16 * n16 + i] = src[16 * n16 + i];
    } else {
        for (size_t b = 16 * i; b < 16 * i + 16 && b < bytes; ++b) dst[b] = src[b];
    }
}
extern "C" int qdas_internal_upload(void *dst, const void *src, size_t bytes) {
    constexpr size_t CAP = 1u << 20;
    if (!bytes) return (int)hipSuccess;
    // (larger uploads go through the same pinned buffer, one MiB at a time -- ADVICE r5: they fell back to a plain hipMemcpy, the call the stale read of round 5
    //  involved; root cause unknown, tools/repro keeps reproducing it on fresh boxes -- so no upload of the library takes that path any more)
    static std::mutex mu;
    static void *pin = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!pin && hipHostMalloc(&pin, CAP, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { pin = nullptr; (void)hipGetLastError(); return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
    hipError_t e = hipSuccess;
    for (size_t at = 0; at < bytes && e == hipSuccess; at += CAP) {
        const size_t nb = bytes - at < CAP ? bytes - at : CAP;
        memcpy(pin, (const unsigned char *)src + at, nb);
        upload_kernel<<<(unsigned)((nb + 4095) / 4096), 256, 0, nullptr>>>((unsigned char *)dst + at, (const unsigned char *)pin, nb);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (the pinned buffer is rewritten by the next piece)
    }
    return (int)e;
}
static inline hipError_t upload(void *dst, const void *src, size_t bytes) { return (hipError_t)qdas_internal_upload(dst, src, bytes); }

// ---- device staging for host callers of the device-pointer entries (include/qdas.h; the MEX gateway's host-array path)
// Staging buffers are RECYCLED: a gateway call allocates its arguments and frees them again, and on this platform hipMalloc / hipFree around calls that
// use temporaries of the stream-ordered pool had the second call of a fresh process read stale memory (tools/repro/stale_pool.hip: 4 of 30 boxes; 0 of 30
// with the staged buffers kept; csrc/scratch.hip removes the pool side as well).  A buffer that stays mapped does not do that -- and hipMalloc / hipFree
// (synchronising, ~100 us each) leave the call path.  Freed buffers are kept per device and size class (256-byte steps below 1 MiB, 1 MiB steps above),
// at most 4 GiB in all (QDAS_STAGING_CACHE_MB; a gateway that stages a 1.5 GB record per call keeps that buffer too); qdas_device_trim releases them.
namespace {
struct StagingCache {
    std::mutex mu;
    struct Item { void *p; size_t bytes; int dev; };
    std::vector<Item> free_list;
    std::vector<Item> live;                               // (what qdas_device_malloc handed out: size class and device of a pointer)
    size_t cached = 0;
};
StagingCache &staging() { static StagingCache c; return c; }
size_t size_class(size_t bytes) { const size_t step = bytes < (1u << 20) ? 256 : (1u << 20); return (std::max<size_t>(bytes, 1) + step - 1) / step * step; }
}  // namespace

extern "C" int qdas_device_malloc(void **p, size_t bytes, int device) {
    if (!p) return fail(QDAS_EINVAL, "null argument");
    *p = nullptr;
    DeviceGuard guard(device);
    HIPCHK(guard.err);
    int dev = device;
    if (dev < 0) HIPCHK(hipGetDevice(&dev));
    const size_t cls = size_class(bytes);
    StagingCache &c = staging();
    {
        std::lock_guard<std::mutex> lk(c.mu);
        for (size_t k = c.free_list.size(); k-- > 0;)
            if (c.free_list[k].bytes == cls && c.free_list[k].dev == dev) {
                *p = c.free_list[k].p;
                c.cached -= cls;
                c.live.push_back(c.free_list[k]);
                c.free_list.erase(c.free_list.begin() + (long)k);
                return QDAS_OK;
            }
    }
    hipError_t e = hipMalloc(p, cls);
    if (e != hipSuccess) {                                // (out of memory: give the cache back and try once more)
        (void)hipGetLastError();
        qdas_device_trim();
        e = hipMalloc(p, cls);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return fail(QDAS_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
    std::lock_guard<std::mutex> lk(c.mu);
    c.live.push_back({*p, cls, dev});
    return QDAS_OK;
}
extern "C" int qdas_device_free(void *p, int device) {
    if (!p) return QDAS_OK;
    StagingCache &c = staging();
    {
        std::lock_guard<std::mutex> lk(c.mu);
        for (size_t k = 0; k < c.live.size(); ++k)
            if (c.live[k].p == p) {
                const StagingCache::Item it = c.live[k];
                c.live.erase(c.live.begin() + (long)k);
                static const size_t cap = [] { const char *e = getenv("QDAS_STAGING_CACHE_MB"); return (size_t)(e && atoll(e) >= 0 ? atoll(e) : 4096) << 20; }();
                if (c.cached + it.bytes <= cap) {
                    // hipFree waits for the device before it unmaps; a RECYCLED buffer must be as idle as a freed one: the next qdas_device_malloc of
                    // this size class hands it out at once, and a kernel the caller launched on a non-blocking stream may still be reading or writing it -- the
                    // next owner's upload (null stream: not ordered with hipStreamNonBlocking streams) would race with it.  One device-wide wait, outside the lock.
                    c.mu.unlock();
                    hipError_t se;
                    { DeviceGuard guard(it.dev); se = guard.err != hipSuccess ? guard.err : getenv("QDAS_DEVICE_FREE_NO_SYNC") ? hipSuccess : hipDeviceSynchronize(); }      // (the switch: tests show the hazard with it)
                    c.mu.lock();
                    if (se != hipSuccess) { (void)hipGetLastError(); c.live.push_back(it); return fail(QDAS_EHIP, "qdas_device_free: hipDeviceSynchronize: %s", hipGetErrorString(se)); }
                    c.free_list.push_back(it);
                    c.cached += it.bytes;
                    return QDAS_OK;
                }
                break;
            }
    }
    DeviceGuard guard(device);
    HIPCHK(guard.err);
    HIPCHK(hipFree(p));
    return QDAS_OK;
}
extern "C" int qdas_device_trim(void) {
    scratch_trim();                                       // (the one-shot entries' arenas of idle streams)
    StagingCache &c = staging();
    std::vector<StagingCache::Item> drop;
    {
        std::lock_guard<std::mutex> lk(c.mu);
        drop.swap(c.free_list);
        c.cached = 0;
    }
    int rc = QDAS_OK;
    for (const auto &it : drop) {
        DeviceGuard guard(it.dev);
        if (guard.err != hipSuccess || hipFree(it.p) != hipSuccess) { (void)hipGetLastError(); rc = QDAS_EHIP; }
    }
    return rc;
}
extern "C" int qdas_device_copy(void *dst, const void *src, size_t bytes, int kind, int device) {
    if (!bytes) return QDAS_OK;
    if (!dst || !src || kind < 0 || kind > 2) return fail(QDAS_EINVAL, "qdas_device_copy: null pointer or unknown kind");
    DeviceGuard guard(device);
    HIPCHK(guard.err);
    if (kind == 0) HIPCHK(upload(dst, src, bytes));
    else HIPCHK(hipMemcpy(dst, src, bytes, kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return QDAS_OK;
}
