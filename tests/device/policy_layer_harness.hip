// policy_layer_harness.hip -- policy::layer of csrc/policy_mlp.h behind a C entry, for tests/test_policy_layer_gpu.py: one workgroup of policy::kThreads per
// 16 rows copies its rows of `in` (the caller's words, the padding past K included) into LDS at the caller's stride, pre-fills the LDS output rows with the
// caller's words of `out` (a sentinel), calls policy::layer unchanged and copies all 16 x out_stride output words back, so the test sees every LDS word
// the layer wrote and every one it must not have.  The header is included as mpc_ppo.hip includes it.  Built by the test with
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -I csrc, as csrc/Makefile compiles the kernels.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {
#include "policy_mlp.h"
}

namespace {
constexpr size_t kMaxLds = 160 * 1024;       // what mpc_policy_create and mpc_ac_create allow

// in [groups * 16][in_stride], out [groups * 16][out_stride], moved as 32-bit words (a NaN's payload is kept)
__global__ __launch_bounds__(policy::kThreads) void layer_kernel(const uint32_t *__restrict__ in, int in_stride, uint32_t *__restrict__ out, int out_stride,
                                                                 const float *__restrict__ W, const float *__restrict__ b, int K, int NOUT, int elu) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *lin = lds, *lout = lds + policy::kRows * in_stride;
  const uint32_t *gin = in + (size_t)blockIdx.x * policy::kRows * in_stride;
  uint32_t *gout = out + (size_t)blockIdx.x * policy::kRows * out_stride;
  for (int e = threadIdx.x; e < policy::kRows * in_stride; e += policy::kThreads) reinterpret_cast<uint32_t *>(lin)[e] = gin[e];
  for (int e = threadIdx.x; e < policy::kRows * out_stride; e += policy::kThreads) reinterpret_cast<uint32_t *>(lout)[e] = gout[e];
  __syncthreads();
  policy::layer(lin, in_stride, lout, out_stride, W, b, K, NOUT, elu != 0);
  __syncthreads();
  for (int e = threadIdx.x; e < policy::kRows * out_stride; e += policy::kThreads) gout[e] = reinterpret_cast<const uint32_t *>(lout)[e];
}

bool aligned16(const void *p) { return p && (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace

extern "C" {

// out[0] = policy::kThreads, out[1] = policy::kWaves, out[2] = policy::kRows, out[3] = policy::kPad
void policy_layer_harness_constants(int *out) {
  out[0] = policy::kThreads; out[1] = policy::kWaves; out[2] = policy::kRows; out[3] = policy::kPad;
}

// The dynamic LDS of a launch: both row blocks.
long long policy_layer_harness_lds_bytes(int in_stride, int out_stride) {
  return (long long)sizeof(float) * policy::kRows * ((long long)in_stride + out_stride);
}

// Returns 0, -1 for a call outside what the C ABI guarantees policy::layer (K a positive multiple of 16, W 16-byte aligned, rows that hold their
// layer, the input rows 16-byte aligned in LDS) or outside the LDS of a CU, or the hipError_t of the set-up or the launch.
int policy_layer_harness_launch(const float *in, int in_stride, float *out, int out_stride, const float *W, const float *b, int K, int NOUT, int elu,
                                int groups, void *stream) {
  if (!in || !out || !b || !aligned16(W) || K <= 0 || K % 16 != 0 || NOUT <= 0 || groups <= 0) return -1;
  if (in_stride < K || in_stride % 4 != 0 || out_stride < NOUT) return -1;
  const long long bytes = policy_layer_harness_lds_bytes(in_stride, out_stride);
  if (bytes > (long long)kMaxLds) return -1;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(layer_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(layer_kernel, dim3((unsigned)groups), dim3(policy::kThreads), (size_t)bytes, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint32_t *>(in), in_stride, reinterpret_cast<uint32_t *>(out), out_stride, W, b, K, NOUT, elu);
  return (int)hipGetLastError();
}

}  // extern "C"
