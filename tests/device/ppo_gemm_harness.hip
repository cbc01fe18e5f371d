// ppo_gemm_harness.hip -- csrc/ppo_gemm.h's kernels behind a C entry each, for tests/test_ppo_gemm_gpu.py: the test fills a pgemm::Launch (a ctypes mirror
// of the struct, whose size is checked against ppo_gemm_harness_sizeof_launch) and names the instantiation itself; the launch plan of mpc_ppo_update.hip
// is not involved.  Built by the test with hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off, as csrc/Makefile compiles the kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppo_gemm.h"

namespace {
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// what the C ABI guarantees the kernel (mpc_ppo_update.hip): 16-byte aligned operands, leading dimensions that are multiples of 4 floats and cover the width
bool admissible(const pgemm::Problem &p, int kind) {
  if (p.tiles_m == 0) return true;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.tiles_m < 0 || p.tiles_n <= 0 || p.chunks <= 0) return false;
  if (!p.A || !p.B || !p.C || !aligned16(p.A) || !aligned16(p.B) || !aligned16(p.C)) return false;
  if (p.lda % 4 || p.ldb % 4 || p.ldc % 4 || p.ldc < p.N) return false;
  if (p.idx && p.idx_limit <= 0) return false;
  if (kind == pgemm::kForward) return p.aux && p.lda >= p.K && p.ldb >= p.K && p.chunks == 1;
  if (kind == pgemm::kBackwardData) return p.aux && p.ldaux >= p.N && p.lda >= p.K && p.ldb >= p.N && p.chunks == 1;
  return p.lda >= p.M && p.ldb >= p.N && p.chunk_rows > 0 && (long long)p.chunks * p.chunk_rows >= p.K && (long long)(p.chunks - 1) * p.chunk_rows < p.K;
}

template <int KIND>
void start(const pgemm::Launch &L, int wide, unsigned gx, hipStream_t s) {
  if (wide) hipLaunchKernelGGL((pgemm::gemm_kernel<KIND, 2, 2>), dim3(gx, 2), dim3(pgemm::kThreads), 0, s, L);
  else hipLaunchKernelGGL((pgemm::gemm_kernel<KIND, 2, 1>), dim3(gx, 2), dim3(pgemm::kThreads), 0, s, L);
}
}  // namespace

extern "C" {

int ppo_gemm_harness_sizeof_launch() { return (int)sizeof(pgemm::Launch); }

// kind: pgemm::Kind; wide: 0 = gemm_kernel<KIND, 2, 1> (128 x 64), 1 = gemm_kernel<KIND, 2, 2> (128 x 128).  Returns 0, -1 for a launch the ABI
// would have refused, or the hipError_t of the launch.
int ppo_gemm_harness_launch(const pgemm::Launch *launch, int kind, int wide, void *stream) {
  if (!launch || kind < pgemm::kForward || kind > pgemm::kBackwardWeight) return -1;
  unsigned gx = 0;
  for (const pgemm::Problem &p : launch->p) {
    if (!admissible(p, kind)) return -1;
    const int bn = wide ? 128 : 64;
    if (p.tiles_m && (p.tiles_m != (p.M + 127) / 128 || p.tiles_n != (p.N + bn - 1) / bn)) return -1;
    const unsigned g = (unsigned)(p.tiles_m * p.tiles_n * p.chunks);
    gx = g > gx ? g : gx;
  }
  if (gx == 0) return -1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (kind == pgemm::kForward) start<pgemm::kForward>(*launch, wide, gx, s);
  else if (kind == pgemm::kBackwardData) start<pgemm::kBackwardData>(*launch, wide, gx, s);
  else start<pgemm::kBackwardWeight>(*launch, wide, gx, s);
  return (int)hipGetLastError();
}

// pgemm::reduce_kernel over n entries: out[i][e] = the sum over chunks[i] partials of part[i][c][e], e < numel[i]
int ppo_gemm_harness_reduce(int n, const float *const *part, float *const *out, const int *numel, const int *chunks, void *stream) {
  if (n <= 0 || n > pgemm::kMaxReduce || !part || !out || !numel || !chunks) return -1;
  pgemm::ReduceTable t{};
  int maxn = 0;
  for (int i = 0; i < n; ++i) {
    if (!part[i] || !out[i] || numel[i] <= 0 || chunks[i] <= 0) return -1;
    t.e[i] = pgemm::ReduceEntry{part[i], out[i], numel[i], chunks[i]};
    maxn = numel[i] > maxn ? numel[i] : maxn;
  }
  hipLaunchKernelGGL(pgemm::reduce_kernel, dim3((unsigned)((maxn + pgemm::kThreads - 1) / pgemm::kThreads), (unsigned)n), dim3(pgemm::kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), t);
  return (int)hipGetLastError();
}

}  // extern "C"
