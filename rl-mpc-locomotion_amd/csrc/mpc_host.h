// mpc_host.h -- the host-side scaffolding every C ABI unit (mpc_*.hip) shares.  Host only, nothing in it reaches a kernel.  Not part of the C ABI.
// What a unit gets from it:
//   DeviceGuard        works on the handle's device and restores the caller's
//   current_device     the device a `create` puts its handle on, or -1 for "no HIP device"
//   destroy_handle     the body of every mpc_*_destroy: guard, synchronise, delete
//   DeviceArray<T>     the owner of one hipMalloc'd array: a handle's `DeviceArray<T> d_x` is memory the handle owns and `delete` frees,
//                      a plain `T *d_x` is memory of somebody else's
//   sync_copy          a synchronous get / set of such an array: synchronise, copy, and after an upload synchronise again
//   ErrorSlot, HIP_TRY the text behind mpc_*_last_error and the check of a HIP call
//   round16            a byte rounding
//   aligned16, present16, Range, any_overlap   the pointer checks in front of 16-byte loads and of a call's output arrays
//   launch_over_ids    one launch over all robots, a host list of ids (uploaded and freed on the stream) or a device list
//   LdsLimit           a kernel's dynamic-LDS limit, grow-only per device
//
// A unit keeps its own slot, and with it its own mpc_*_last_error, and names the slot's setter `fail`:
//   namespace {
//   thread_local mpchost::ErrorSlot g_err;
//   int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }
//   }
// (Where several units share one mpc_*_last_error, one of them owns the slot and the others' `fail` forwards to it: mpc_ppo_update.hip's to
// mpc_ppo.hip's, mpc_ctrl.hip's and mpc_policy.hip's to mpc_batch.hip's.)  HIP_TRY returns through that `fail`.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>

namespace mpchost {

// Every entry point works on the device its handle was created on and leaves the caller's current device as it found it
// (a process may hold handles on several GPUs, and the caller -- torch -- has a current device of its own).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// The device a new handle lives on: the caller's current one.  -1 where there is no HIP device (the unit words its own MPC_E_NODEVICE message).
inline int current_device() {
  int ndev = 0, dev = -1;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || hipGetDevice(&dev) != hipSuccess) return -1;
  return dev;
}

// One hipMalloc'd array of T and its owner: freed by reset() and by the destructor, so a handle that holds its arrays as DeviceArray members
// has no free list to keep.  Converts to T * so that launches and the other units read it as the pointer it is.  One hipMalloc / hipFree per
// array, under the caller's device guard; an alloc* on an array that holds memory frees that first.
template <typename T>
class DeviceArray {
 public:
  DeviceArray() = default;
  DeviceArray(const DeviceArray &) = delete;
  DeviceArray &operator=(const DeviceArray &) = delete;
  DeviceArray(DeviceArray &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DeviceArray &operator=(DeviceArray &&o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  ~DeviceArray() { reset(); }

  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = hipMalloc(&p_, sizeof(T) * count);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  hipError_t alloc_zero(size_t count) {
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : hipMemset(p_, 0, sizeof(T) * count);
  }
  hipError_t alloc_copy(const T *host, size_t count) {
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : hipMemcpy(p_, host, sizeof(T) * count, hipMemcpyHostToDevice);
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
};

// What every mpc_*_destroy is: wait, on the handle's device, for the launches that may still read its arrays, then delete (the DeviceArray
// members free there, under the guard).  A handle that binds its device later and never did (device < 0) has nothing on any device.
template <typename Handle>
void destroy_handle(Handle *h) {
  if (!h) return;
  DeviceGuard guard_(h->device);
  if (h->device >= 0) (void)hipDeviceSynchronize();
  delete h;
}

// What a synchronous get / set of a handle's array is: wait for the launches that may still write or read it, copy `count` words, and after an
// upload wait again, so that whatever the caller launches next, on any stream, sees it.  Under the caller's device guard.
template <typename T>
hipError_t sync_copy(T *dst, const T *src, size_t count, hipMemcpyKind kind) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(dst, src, sizeof(T) * count, kind);
  return e != hipSuccess || kind != hipMemcpyHostToDevice ? e : hipDeviceSynchronize();
}

// the text behind a unit's mpc_*_last_error: one thread_local instance per unit
struct ErrorSlot : std::string {
  int fail(int code, const std::string &msg) { assign(msg); return code; }
};

inline size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// What a kernel's 16-byte loads ask of a pointer.  aligned16 lets null through: an optional array is checked like the others and a required one
// has its own null check, with its own message, in front.  present16 is for the entry points whose one message is "non-null and 16-byte aligned".
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool present16(const void *p) { return p && aligned16(p); }

// The byte ranges of the arrays a call writes: any_overlap is true where two of them share a byte.  A null range overlaps nothing.
struct Range { const void *p; size_t bytes; };
inline bool any_overlap(const Range *r, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(r[i].p), b = reinterpret_cast<uintptr_t>(r[j].p);
      if (a && b && a < b + r[j].bytes && b < a + r[i].bytes) return true;
    }
  return false;
}

// One launch over the robots a reset names: launch(d_ids, count) with (null, n) for all of them (ids null), with the k ids of a device list, or
// with the k ids of a host list, which are uploaded on the stream in front of the launch and freed on it behind.  Nothing to do for k <= 0.
enum class Ids { host, device };
template <typename Launch>
hipError_t launch_over_ids(const int *ids, int k, int n, Ids where, hipStream_t st, Launch launch) {
  if (ids && k <= 0) return hipSuccess;
  if (!ids || where == Ids::device) {
    launch(ids, ids ? k : n);
    return hipGetLastError();
  }
  int *d_ids = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_ids), sizeof(int) * k, st);
  if (e != hipSuccess) return e;
  if ((e = hipMemcpyAsync(d_ids, ids, sizeof(int) * k, hipMemcpyHostToDevice, st)) == hipSuccess) {
    launch(d_ids, k);
    e = hipGetLastError();
  }
  const hipError_t freed = hipFreeAsync(d_ids, st);
  return e != hipSuccess ? e : freed;
}

// The dynamic-LDS limit of one kernel (hipFuncAttributeMaxDynamicSharedMemorySize): one value per device and kernel, not one per handle, so it
// only ever grows -- a handle with a narrow net, made after one with a wide net, must not take the wide one's launches away (DESIGN.md section
// 8.4, "Two conventions of the C ABI units").  One instance per kernel, in the unit that launches it; raise() runs with the handle's device current.
class LdsLimit {
 public:
  template <typename... Args>
  explicit LdsLimit(void (*kernel)(Args...)) : kernel_(reinterpret_cast<const void *>(kernel)) {}
  hipError_t raise(int device, size_t bytes) {
    std::lock_guard<std::mutex> lock(mutex_);
    size_t &limit = limit_[device];
    if (bytes <= limit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel_, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) limit = bytes;
    return e;
  }

 private:
  const void *kernel_;
  std::mutex mutex_;
  std::map<int, size_t> limit_;
};

}  // namespace mpchost

// A failed HIP call returns MPC_E_HIP from the entry point, with the call as it is written in the source and HIP's text.  (One macro level on
// purpose: expr is stringified before any macro inside it expands.)
#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return fail(MPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
