// Host helpers of the files that call the HIP runtime (kcdc_internal.h stays free of it).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "kcdc_internal.h"

namespace kcdc {

// Records "what: <the runtime's text>" as the thread's error; returns KCDC_EIO (-5).
inline int hip_error(hipError_t e, const char* what) {
    return set_error(-5, std::string(what) + ": " + hipGetErrorString(e));
}

// Makes `dev` the calling thread's device for a scope.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;  // of hipSetDevice(dev), for callers that report it
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

}  // namespace kcdc
