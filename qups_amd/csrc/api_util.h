// api_util.h -- what the host side of every translation unit that holds an entry of the C ABI shares (internal): the thread's
// last-error string, the HIP error check, the device guard, the element sizes of the three precisions, the staged upload.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/qdas.h"

void qdas_internal_set_error(const char *msg);                                  // qdas_api.hip: the thread-local message behind qdas_last_error()
extern "C" int qdas_internal_upload(void *dst, const void *src, size_t bytes);  // staging.hip: host -> device through pinned staging, synchronous (a hipError_t)

namespace qdas {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));  // qdas_api.hip: sets the calling thread's message, returns `code`
const char *last_error();                                                        // ... and reads it (valid until the thread's next message)

#define HIPCHK(call)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return qdas::fail(QDAS_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// Every entry that works on a particular device switches to it for the duration of the call only: the calling thread's current
// device is restored on every return path (a MEX gateway or a plain C caller keeps issuing its own work where it was).
struct DeviceGuard {
    int prev = -1;
    bool restore = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); restore = err == hipSuccess; }
    }
    ~DeviceGuard() { if (restore) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

inline size_t real_size(int dtype) { return dtype == QDAS_F64 ? 8 : 4; }            // geometry / time type
inline size_t data_size(int dtype) { return dtype == QDAS_F64 ? 16 : (dtype == QDAS_F32 ? 8 : 4); }  // complex sample
inline size_t apod_real_size(int dtype) { return dtype == QDAS_F64 ? 8 : (dtype == QDAS_F32 ? 4 : 2); }

}  // namespace qdas
