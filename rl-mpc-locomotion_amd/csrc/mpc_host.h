// mpc_host.h -- the host-side scaffolding every C ABI unit (mpc_*.hip) shares: the device guard, the error slot, the HIP error check and a
// byte rounding.  Host only, nothing in it reaches a kernel.  Not part of the C ABI.
//
// A unit keeps its own slot, and with it its own mpc_*_last_error, and names the slot's setter `fail`:
//   namespace {
//   thread_local mpchost::ErrorSlot g_err;
//   int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }
//   }
// (mpc_ppo_update.hip's `fail` forwards to mpc_ppo.hip's slot instead.)  HIP_TRY returns through that `fail`.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

namespace mpchost {

// Every entry point works on the device its handle was created on and leaves the caller's current device as it found it
// (a process may hold handles on several GPUs, and the caller -- torch -- has a current device of its own).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// the text behind a unit's mpc_*_last_error: one thread_local instance per unit
struct ErrorSlot : std::string {
  int fail(int code, const std::string &msg) { assign(msg); return code; }
};

inline size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

}  // namespace mpchost

// A failed HIP call returns MPC_E_HIP from the entry point, with the call as it is written in the source and HIP's text.  (One macro level on
// purpose: expr is stringified before any macro inside it expands.)
#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return fail(MPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
