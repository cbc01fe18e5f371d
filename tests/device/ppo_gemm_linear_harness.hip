// ppo_gemm_linear_harness.hip -- csrc/ppo_gemm.h's gemm_kernel<pgemm::kBackwardDataLinear, 2, TN> behind one C entry, for
// tests/test_recurrent_update_gpu.py, as tests/device/ppo_gemm_harness.hip does it for the other three kinds: the test fills a pgemm::Launch (a ctypes
// mirror of the struct) and names the tile itself, so the 128 x 128 tile runs at shapes far below those at which the plan picks it.
// Built by the test with hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off, as csrc/Makefile compiles the kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppo_gemm.h"

namespace {
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// what mpc_ppo_update_grads_sequence guarantees the kernel: 16-byte aligned operands, leading dimensions that are multiples of 4 floats and cover the width
bool admissible(const pgemm::Problem &p) {
  if (p.tiles_m == 0) return true;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.tiles_m < 0 || p.tiles_n <= 0 || p.chunks != 1) return false;
  if (!p.A || !p.B || !p.C || !aligned16(p.A) || !aligned16(p.B) || !aligned16(p.C)) return false;
  if (p.lda % 4 || p.ldb % 4 || p.ldc % 4 || p.ldc < p.N) return false;
  return p.lda >= p.K && p.ldb >= p.N;
}
}  // namespace

extern "C" {

int ppo_gemm_linear_harness_sizeof_launch() { return (int)sizeof(pgemm::Launch); }

// wide: 0 = gemm_kernel<3, 2, 1> (128 x 64), 1 = gemm_kernel<3, 2, 2> (128 x 128).  Returns 0, -1 for a launch the ABI would have refused, or the
// hipError_t of the launch.
int ppo_gemm_linear_harness_launch(const pgemm::Launch *launch, int wide, void *stream) {
  if (!launch) return -1;
  unsigned gx = 0;
  for (const pgemm::Problem &p : launch->p) {
    if (!admissible(p)) return -1;
    const int bn = wide ? 128 : 64;
    if (p.tiles_m && (p.tiles_m != (p.M + 127) / 128 || p.tiles_n != (p.N + bn - 1) / bn)) return -1;
    const unsigned g = (unsigned)(p.tiles_m * p.tiles_n);
    gx = g > gx ? g : gx;
  }
  if (gx == 0) return -1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (wide) hipLaunchKernelGGL((pgemm::gemm_kernel<pgemm::kBackwardDataLinear, 2, 2>), dim3(gx, 2), dim3(pgemm::kThreads), 0, s, *launch);
  else hipLaunchKernelGGL((pgemm::gemm_kernel<pgemm::kBackwardDataLinear, 2, 1>), dim3(gx, 2), dim3(pgemm::kThreads), 0, s, *launch);
  return (int)hipGetLastError();
}

}  // extern "C"
