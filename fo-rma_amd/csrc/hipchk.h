// hipchk.h — HIP error and device plumbing the entry points share (render.hip,
// selftest.hip, mctx.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"

#define HIPCHK(call)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fr::set_error(FR_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));       \
  } while (0)

namespace fr {

// Sets a call's device and restores the caller's current device when the call returns,
// so an entry point never leaves torch (or any other caller) on another device.
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = hipSetDevice(d);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

}  // namespace fr

#define SET_DEVICE(d)               \
  fr::DeviceGuard dev_guard_((d));  \
  HIPCHK(dev_guard_.err)
