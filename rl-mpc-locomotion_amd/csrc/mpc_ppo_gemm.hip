// mpc_ppo_gemm.hip -- the one owner of ppo_gemm.h's kernels in the library: an internal unit with no C ABI.  mpc_ppo_update.hip and
// mpc_recurrent_bptt.hip fill ppo_gemm_plan.h's structs and call pgemm::launch (the plan's tile, chunking and grid filled into the launch, then
// gemm_kernel<KIND, 2, 2> or <KIND, 2, 1>; KIND one of ppo_gemm_plan.h's four) and pgemm::reduce (reduce_kernel).  Both only enqueue; the caller asks hipGetLastError in its own words.
#include <hip/hip_runtime.h>

#include "ppo_gemm.h"

namespace pgemm {

template <int KIND>
static void start(const Plan &plan, const Launch &L, hipStream_t s) {
  if (plan.wide) hipLaunchKernelGGL((gemm_kernel<KIND, 2, 2>), dim3(plan.grid_x, 2), dim3(kThreads), 0, s, L);
  else hipLaunchKernelGGL((gemm_kernel<KIND, 2, 1>), dim3(plan.grid_x, 2), dim3(kThreads), 0, s, L);
}

void launch(Kind kind, Launch &L, void *stream) {
  const Shape shape[2] = {{L.p[0].M, L.p[0].N, L.p[0].K}, {L.p[1].M, L.p[1].N, L.p[1].K}};
  const Plan plan = plan_gemm(kind, shape);
  for (int k = 0; k < 2; ++k) {
    Problem &p = L.p[k];
    p.tiles_m = plan.p[k].tiles_m;
    p.tiles_n = plan.p[k].tiles_n;
    p.chunks = plan.p[k].chunks;
    if (kind == kBackwardWeight) p.chunk_rows = plan.chunk_rows;
  }
  if (plan.grid_x == 0) return;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (kind == kForward) start<kForward>(plan, L, s);
  else if (kind == kBackwardData) start<kBackwardData>(plan, L, s);
  else if (kind == kBackwardDataLinear) start<kBackwardDataLinear>(plan, L, s);
  else start<kBackwardWeight>(plan, L, s);
}

void reduce(const ReduceTable &t, int entries, int max_numel, void *stream) {
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((max_numel + kThreads - 1) / kThreads), (unsigned)entries), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), t);
}

}  // namespace pgemm
