// nmpc_host.hpp -- the host-side plumbing every C-ABI entry point of libnmpc_hip.so shares: the device guard, the error
// slots, the HIP-call check, the launch check and the entry guard.  An entry point reads, in this order:
//   1. the handle            if (!h) return ...;
//   2. the empty batch       if (B == 0) return NMPC_OK;      (its tensors have no storage: their pointers may be NULL)
//   3. the arguments         return fail(h, NMPC_E_ARG, ...)  all of it on the host, in front of anything that touches a device
//   4. the device            NMPC_ENTER(h, device);
//   5. the work              NMPC_TRY(h, hipMemcpyAsync(...)); hipLaunchKernelGGL(...);
//   6. the launches          return launched(h);
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/nmpc.h"

namespace nmpc {

// Every entry point runs on the device its handle (or its tensors) live on and leaves the caller's current device as
// it found it (torch keeps its own notion of the current device; an entry point that called hipSetDevice and returned
// would change it behind torch's back, and one that launched on the current device with a stream of another device
// would fail).  Opened through NMPC_ENTER, which reports a failed switch.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && dev >= 0 && dev != prev) {
            err = hipSetDevice(dev);
            switched = (err == hipSuccess);
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// device a pointer was allocated on, -1 if it is not a device pointer (handle-less entry points take their device
// from their first tensor)
inline int device_of(const void* p) {
    hipPointerAttribute_t attr;
    if (p && hipPointerGetAttributes(&attr, p) == hipSuccess) return attr.device;
    (void)hipGetLastError();
    return -1;
}

// The error slots.  H is a family's handle type (a struct with a std::string err).  It lives in the unnamed namespace of
// its family's translation unit, so every family has a thread-local string of its own for the calls that have no handle,
// and what one family reports never overwrites another's.
template <class H>
std::string& family_error() {
    thread_local std::string msg;
    return msg;
}

// record the message (in the handle, without one in its family's slot) and return the code
template <class H>
int fail(H* h, int code, const std::string& msg) {
    (h ? h->err : family_error<H>()) = msg;
    return code;
}

template <class H>
const char* last_error(const H* h) { return (h ? h->err : family_error<H>()).c_str(); }

// after the last launch of an entry point: launches report their errors through hipGetLastError alone
template <class H>
int launched(H* h) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NMPC_OK : fail(h, NMPC_E_HIP, std::string("hipGetLastError(): ") + hipGetErrorString(e));
}

}  // namespace nmpc

// a HIP call of an entry point (or of a helper that returns its code): NMPC_E_HIP and "<call>: <HIP's text>" if it fails
#define NMPC_TRY(h, expr)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return nmpc::fail(h, NMPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// the device of an entry point, for the rest of its scope; a switch that failed is the entry point's error
#define NMPC_ENTER(h, device)        \
    nmpc::DeviceGuard guard(device); \
    NMPC_TRY(h, guard.err)
