// mpc_domain_rand.hip -- the C ABI of mpc_domain_rand.h: the opt-in domain randomisation (domain_rand.h) on the device, in two kernels.
//   noise_kernel   a flat index over the column pairs of the matrix [n][W]: consecutive lanes sit on consecutive float2 of a row (every width
//                  is even), so a wave's load and its store each cover 512 consecutive bytes.  A grid-stride loop over at most 2048 workgroups
//                  (8 per CU).  A pair below `active` draws its two values (one Box-Muller pair, or two uniforms), recomputes the persistent
//                  correlated pair when the wave-uniform flag asks for it, and applies domain_rand.h's formula; a pad pair is copied.  The
//                  parameters travel by value as kernel arguments.  in may be out: a lane reads its own float2 before it writes it.
//   push_kernel    one lane per robot, the plant's grid: a robot that has not fallen gets a new world x, y velocity, as a double in the
//                  plant's structure-of-arrays state and as the float32 in the root-state tensor.
// No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "domain_rand.h"
#include "mpc_domain_rand.h"
#include "mpc_host.h"
#include "mpc_sim_internal.h"

using drand::Params;
using mpchost::DeviceGuard;

static_assert(MPC_DRAND_OBSERVATIONS == drand::kTargetObs && MPC_DRAND_ACTIONS == drand::kTargetAct, "mpc_domain_rand.h and domain_rand.h disagree");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 2048;  // 256 CUs x 8 workgroups; the loop strides over the rest

__global__ __launch_bounds__(kThreads) void noise_kernel(Params p, unsigned total, unsigned pairs_per_row, const float *__restrict__ col_scale,
                                                         const float *in, float *out, float *draws) {
  const unsigned stride = gridDim.x * kThreads;
  for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const unsigned r = i / pairs_per_row, pr = i - r * pairs_per_row;
    const float2 x = reinterpret_cast<const float2 *>(in)[i];
    float2 y;
    drand::noise_columns(p, r, pr, col_scale, x.x, x.y, y.x, y.y, draws ? draws + (size_t)r * (size_t)p.active * 2 : nullptr);
    reinterpret_cast<float2 *>(out)[i] = y;
  }
}

__global__ __launch_bounds__(simint::kSimThreads) void push_kernel(int n, unsigned long long seed, float v, unsigned push_index, double *f64,
                                                                   const int *__restrict__ i32, float *root) {
  const int r = (int)(blockIdx.x * simint::kSimThreads + threadIdx.x);
  if (r >= n) return;
  if (i32[8 * (size_t)n + r] != 0) return;                                 // fallen: stays frozen
#pragma unroll
  for (unsigned a = 0; a < 2; ++a) {
    const float pv = drand::push_value(seed, (uint32_t)r, push_index, a, v);
    f64[(size_t)(toysim::kOffV + a) * (size_t)n + r] = (double)pv;
    root[(size_t)r * 13 + 7 + a] = pv;
  }
}
}  // namespace

struct mpc_drand {
  int n = 0, device = 0;
  unsigned long long seed = 0;
  double *d_f64 = nullptr;             // the bound sim's state record (null until mpc_drand_bind)
  const int *d_i32 = nullptr;
};

extern "C" {

const char *mpc_drand_last_error(void) { return g_err.c_str(); }

void mpc_drand_destroy(mpc_drand *h) { delete h; }

int mpc_drand_create(mpc_drand **out, int n, unsigned long long seed) {
  if (!out) return fail(MPC_E_ARG, "mpc_drand_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_drand_create: n must be at least 1");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_drand_create: no HIP device");
  mpc_drand *h = new mpc_drand();
  h->n = n;
  h->seed = seed;
  h->device = device;
  *out = h;
  return MPC_OK;
}

int mpc_drand_bind(mpc_drand *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_drand_bind: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_drand_bind: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_drand_bind: the sim has " + std::to_string(s->n) + " robots, the randomisation " + std::to_string(h->n) + " environments");
  if (s->device != h->device) return fail(MPC_E_ARG, "mpc_drand_bind: the sim lives on another device");
  h->d_f64 = s->d_f64;
  h->d_i32 = s->d_i32;
  return MPC_OK;
}

int mpc_drand_noise(mpc_drand *h, int target, int distribution, int operation, double m, double s, double m_corr, double s_corr, double clip,
                    const float *d_col_scale, const float *d_in, float *d_out, int W, int active, long long tick, float *d_draws, void *stream) {
  if (!h || !d_in || !d_out) return fail(MPC_E_ARG, "mpc_drand_noise: null argument");
  if (target != MPC_DRAND_OBSERVATIONS && target != MPC_DRAND_ACTIONS) return fail(MPC_E_ARG, "mpc_drand_noise: target must be 0 (observations) or 1 (actions)");
  if (distribution != MPC_DRAND_GAUSSIAN && distribution != MPC_DRAND_UNIFORM)
    return fail(MPC_E_ARG, "mpc_drand_noise: distribution must be 0 (gaussian) or 1 (uniform)");
  if (operation != MPC_DRAND_ADDITIVE && operation != MPC_DRAND_SCALING) return fail(MPC_E_ARG, "mpc_drand_noise: operation must be 0 (additive) or 1 (scaling)");
  if (W < 2 || (W & 1)) return fail(MPC_E_ARG, "mpc_drand_noise: W must be even and at least 2");
  if ((long long)h->n * (W / 2) > 0x7FFFFFFFll) return fail(MPC_E_ARG, "mpc_drand_noise: n * W / 2 must stay below 2^31");
  if (active < 0 || active > W) return fail(MPC_E_ARG, "mpc_drand_noise: active must lie in [0, W]");
  if (tick < 0 || tick > 0xFFFFFFFFll) return fail(MPC_E_ARG, "mpc_drand_noise: tick must lie in [0, 2^32)");
  const float pf[4] = {(float)m, (float)s, (float)m_corr, (float)s_corr};
  const char *names[4] = {"m", "s", "m_corr", "s_corr"};
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(pf[i])) return fail(MPC_E_ARG, std::string("mpc_drand_noise: ") + names[i] + " must be finite as a float32");
  if (!(clip >= 0.0)) return fail(MPC_E_ARG, "mpc_drand_noise: clip must be >= 0");
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 7u) return fail(MPC_E_ARG, "mpc_drand_noise: d_in and d_out must be 8-byte aligned");
  const Params p = drand::make_params(target, h->seed, distribution, operation, pf[0], pf[1], pf[2], pf[3], (float)clip, active, (uint32_t)tick);
  const unsigned pairs = (unsigned)(W / 2), total = (unsigned)h->n * pairs;
  unsigned blocks = (total + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(noise_kernel, dim3(blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), p, total, pairs, d_col_scale, d_in, d_out,
                     d_draws);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_drand_push(mpc_drand *h, float *d_root, double max_vel, long long push_index, void *stream) {
  if (!h || !d_root) return fail(MPC_E_ARG, "mpc_drand_push: null argument");
  if (!std::isfinite((float)max_vel) || !(max_vel >= 0.0)) return fail(MPC_E_ARG, "mpc_drand_push: max_vel must be finite and >= 0");
  if (push_index < 0 || push_index > 0xFFFFFFFFll) return fail(MPC_E_ARG, "mpc_drand_push: push_index must lie in [0, 2^32)");
  if (!h->d_f64 || !h->d_i32) return fail(MPC_E_ARG, "mpc_drand_push: no sim bound (mpc_drand_bind)");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(push_kernel, simint::sim_grid(h->n), dim3(simint::kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), h->n, h->seed, (float)max_vel,
                     (unsigned)push_index, h->d_f64, h->d_i32, d_root);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
