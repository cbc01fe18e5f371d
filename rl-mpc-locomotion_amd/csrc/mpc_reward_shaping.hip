// mpc_reward_shaping.hip -- the C ABI of mpc_reward_shaping.h: the opt-in reward shaping terms, the reward they rewrite and their per-term episode
// sums (reward_shaping.h) on the device, in three kernels and three launches per tick.
//   shaping_close_kernel   one lane per environment, one wave per workgroup like terms_close_kernel.  A marked lane (id >= 0) puts its float32 sums
//                          and its closed flag into LDS and zeroes its sums and ticks; lanes 0 .. 8 then each add one word of the block's partial
//                          over the wave's 64 environments in environment order, in float64, and lanes 0 .. 15 write the row.
//   shaping_join_kernel    ONE workgroup of 256: the block partials are staged 256 rows at a time into LDS, lanes 0 .. 8 each add one word over
//                          the staged rows in block order and then add it to the window.
//   shaping_run_kernel     one workgroup of four waves per 16 environments (4096 environments are one workgroup on each of 256 CUs).  First the
//                          base-height means: each wave takes four of the block's environments at once, its 64 lanes on 64 consecutive heights of
//                          each row (coalesced, all loads in flight together), lane-strided partial sums, and the tree of reward_shaping.h as six
//                          lane exchanges; the means go to LDS.  Then 16 lanes of the first wave, one per environment: the task's six terms from
//                          what `finish` read, the eight terms, the reward, the history, sums += terms, ticks += 1.
// No atomics; the order of every sum is fixed, so a rerun from the same state is bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mpc_host.h"
#include "mpc_reward_shaping.h"
#include "mpc_sim_internal.h"
#include "mpc_task_config.h"
#include "reward_shaping.h"

using mpchost::DeviceArray;
using mpchost::DeviceGuard;
using rshape::kBlock;
using rshape::kDof;
using rshape::kLegs;
using rshape::kPartial;
using rshape::kTerms;
using rshape::kWords;

static_assert(MPC_SHAPING_TERMS == kTerms && MPC_SHAPING_SUMMARY == rshape::kSummaryLen && MPC_SHAPING_MAX_POINTS == rshape::kMaxPoints,
              "mpc_reward_shaping.h and reward_shaping.h disagree");
static_assert(toysim::kI32 >= kLegs, "the sim's int32 record starts with the four contact flags");
static_assert(rshape::kLanes == 64, "the base-height mean's lanes are one wave");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kEnvThreads = kBlock;    // one wave per workgroup of the close, and one workgroup per block of the reduction
constexpr int kJoinThreads = 256;      // block partials staged per pass of the join
constexpr int kRow = kTerms + 1;       // LDS row stride of the close kernel: 9 words, odd, so the 64 lanes' stores spread over the banks
constexpr int kRunThreads = 256;       // four waves per kRunEnvs environments
constexpr int kRunEnvs = 16;
constexpr int kRunWaves = kRunThreads / 64;
constexpr int kEnvsPerWave = kRunEnvs / kRunWaves;

__global__ __launch_bounds__(kEnvThreads) void shaping_close_kernel(int n, const int *__restrict__ ids, float *sums, int *ticks,
                                                                    double *__restrict__ partials) {
  __shared__ float rows[kEnvThreads * kRow];
  __shared__ int closed[kEnvThreads];
  const int lane = threadIdx.x;
  const int first = blockIdx.x * kEnvThreads;
  const int r = first + lane;
  int cl = 0;
  if (r < n && ids[r] >= 0) {
    float s[kTerms];
#pragma unroll
    for (int i = 0; i < kTerms; ++i) {
      s[i] = sums[(size_t)r * kTerms + i];
      rows[lane * kRow + i] = s[i];
      sums[(size_t)r * kTerms + i] = 0.0f;
    }
    cl = rshape::closes(ids[r], ticks[r], s) ? 1 : 0;
    ticks[r] = 0;
  }
  closed[lane] = cl;
  __syncthreads();
  if (lane < kPartial)
    partials[(size_t)blockIdx.x * kPartial + lane] = rshape::block_partial_word(min(kEnvThreads, n - first), closed, rows, kRow, lane);
}

__global__ __launch_bounds__(kJoinThreads) void shaping_join_kernel(int blocks, const double *__restrict__ partials, double *window) {
  __shared__ double stage[kJoinThreads * kPartial];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int base = 0; base < blocks; base += kJoinThreads) {
    const int here = min(kJoinThreads, blocks - base);
    for (int i = tid; i < here * kPartial; i += kJoinThreads) stage[i] = partials[(size_t)base * kPartial + i];
    __syncthreads();
    if (tid < kWords) acc = rshape::join_word(acc, here, stage, tid);
    __syncthreads();                   // the words are read before the next pass overwrites them
  }
  if (tid < kWords) window[tid] = window[tid] + acc;
}

__global__ __launch_bounds__(kRunThreads) void shaping_run_kernel(rltask::Config c, rshape::Spec k, int n, const float *__restrict__ root,
                                                                  const float *__restrict__ dof, const float *__restrict__ actions,
                                                                  const float *__restrict__ commands, const float *__restrict__ torques,
                                                                  const unsigned char *__restrict__ fell, const int *__restrict__ ids,
                                                                  const long long *__restrict__ reset, const long long *__restrict__ progress,
                                                                  const int *__restrict__ i32, const float *__restrict__ heights, int P,
                                                                  float *last_actions, float *last_dof_vel, float *air_time, int *last_contact,
                                                                  float *sums, int *ticks, float *rew, float *terms_out) {
  __shared__ float hbar[kRunEnvs];
  const int first = blockIdx.x * kRunEnvs;
  const bool with_height = k.scale[rshape::kBaseHeight] != 0.0f;
  if (with_height && P > 0) {                      // the same for every lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s[kEnvsPerWave], z[kEnvsPerWave];
#pragma unroll
    for (int j = 0; j < kEnvsPerWave; ++j) {       // (a slot past the last environment reads the last one's row again: its mean is never used)
      const int rc = min(first + wave * kEnvsPerWave + j, n - 1);
      z[j] = root[(size_t)rc * 13 + 2];
      s[j] = rshape::height_lane_partial(z[j], heights + (size_t)rc * P, P, lane);
    }
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) {
#pragma unroll
      for (int j = 0; j < kEnvsPerWave; ++j) s[j] = s[j] + __shfl_xor(s[j], stride, 64);       // lane 0 ends with height_join's s[0]
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kEnvsPerWave; ++j) hbar[wave * kEnvsPerWave + j] = rshape::height_mean_from_sum(s[j], z[j], P);
    }
  }
  __syncthreads();
  const int r = first + threadIdx.x;
  if (threadIdx.x >= kRunEnvs || r >= n) return;
  float rt[13], dq[2 * kDof], act[kDof], cmd[3], tq[kDof], t[rshape::kTaskTerms], e[kTerms];
  int contact[kLegs];
  rshape::Env env;
#pragma unroll
  for (int i = 0; i < 13; ++i) rt[i] = root[(size_t)r * 13 + i];
#pragma unroll
  for (int i = 0; i < 2 * kDof; ++i) dq[i] = dof[(size_t)r * 2 * kDof + i];
#pragma unroll
  for (int i = 0; i < kDof; ++i) {
    act[i] = actions[(size_t)r * kDof + i];
    tq[i] = torques[(size_t)r * kDof + i];
    env.last_actions[i] = last_actions[(size_t)r * kDof + i];
    env.last_dof_vel[i] = last_dof_vel[(size_t)r * kDof + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) cmd[i] = commands[(size_t)r * 3 + i];
#pragma unroll
  for (int l = 0; l < kLegs; ++l) {
    contact[l] = i32[(size_t)l * n + r];
    env.air_time[l] = air_time[(size_t)r * kLegs + l];
    env.last_contact[l] = last_contact[(size_t)r * kLegs + l];
  }
#pragma unroll
  for (int i = 0; i < kTerms; ++i) env.sums[i] = sums[(size_t)r * kTerms + i];
  env.ticks = ticks[r];
  rltask::reward_terms(c, rt, cmd, tq, rltask::contacts_from_fell(fell != nullptr && fell[r] != 0), t);
  rshape::tick_terms(c, k, rt, dq, act, cmd, ids[r], reset[r], progress[r], contact,
                     with_height ? (P > 0 ? hbar[threadIdx.x] : rshape::height_mean_from_sum(0.0f, rt[2], 0)) : 0.0f, env, e);
  rew[r] = rshape::reward_from(k, t, e);
  rshape::accumulate_env(e, env.sums, env.ticks);
#pragma unroll
  for (int i = 0; i < kDof; ++i) {
    last_actions[(size_t)r * kDof + i] = env.last_actions[i];
    last_dof_vel[(size_t)r * kDof + i] = env.last_dof_vel[i];
  }
#pragma unroll
  for (int l = 0; l < kLegs; ++l) {
    air_time[(size_t)r * kLegs + l] = env.air_time[l];
    last_contact[(size_t)r * kLegs + l] = env.last_contact[l];
  }
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sums[(size_t)r * kTerms + i] = env.sums[i];
  ticks[r] = env.ticks;
  if (terms_out) {
#pragma unroll
    for (int i = 0; i < kTerms; ++i) terms_out[(size_t)r * kTerms + i] = e[i];
  }
}

__global__ __launch_bounds__(64) void shaping_summary_kernel(const double *__restrict__ window, double episode_length_s, double *out) {
  const int j = threadIdx.x;
  if (j < kWords) out[rshape::kSumClosed + j] = window[j];
  if (j == 0) out[rshape::kSumEpisodeS] = episode_length_s;
}
}  // namespace

struct mpc_shaping {
  int n = 0, blocks = 0, device = 0;
  rltask::Config c{};
  rshape::Spec k{};
  double episode_length_s = 0.0;
  const int *d_i32 = nullptr;          // the bound sim's int32 state record (null until mpc_shaping_bind)
  DeviceArray<float> d_last_actions, d_last_dof_vel;   // [n][12] each
  DeviceArray<float> d_air_time;       // [n][4]
  DeviceArray<int> d_last_contact;     // [n][4]
  DeviceArray<float> d_sums;           // [n][8]
  DeviceArray<int> d_ticks;            // [n]
  DeviceArray<double> d_partials;      // [blocks][kPartial]
  DeviceArray<double> d_window;        // [kWords]
};

extern "C" {

const char *mpc_shaping_last_error(void) { return g_err.c_str(); }

void mpc_shaping_destroy(mpc_shaping *h) { mpchost::destroy_handle(h); }

int mpc_shaping_create(mpc_shaping **out, int n, const mpc_task_config *cfg, const double *scales, double base_height_target, double air_time_target,
                       double dt, double episode_length_s) {
  // everything is validated before the device is touched
  if (!out || !cfg || !scales) return fail(MPC_E_ARG, "mpc_shaping_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_shaping_create: n must be at least 1");
  const taskcfg::Fault bad = taskcfg::check(*cfg);
  if (bad == taskcfg::kNotFinite) return fail(MPC_E_ARG, "mpc_shaping_create: a scale or a command range is not finite");
  if (bad == taskcfg::kRangeOrder) return fail(MPC_E_ARG, "mpc_shaping_create: command range with min > max");
  if (bad == taskcfg::kEpisodeLength) return fail(MPC_E_ARG, "mpc_shaping_create: max_episode_length must be at least 1");
  if (!taskcfg::finite_all(cfg->default_dof_pos, 12)) return fail(MPC_E_ARG, "mpc_shaping_create: default_dof_pos is not finite");
  if (!taskcfg::finite_all(scales, kTerms)) return fail(MPC_E_ARG, "mpc_shaping_create: a shaping scale is not finite");
  if (!std::isfinite(base_height_target)) return fail(MPC_E_ARG, "mpc_shaping_create: base_height_target must be finite");
  if (!std::isfinite(air_time_target) || !(air_time_target >= 0.0)) return fail(MPC_E_ARG, "mpc_shaping_create: air_time_target must be finite and >= 0");
  if (!std::isfinite(dt) || !(dt > 0.0)) return fail(MPC_E_ARG, "mpc_shaping_create: dt must be finite and > 0");
  if (!std::isfinite(episode_length_s) || !(episode_length_s > 0.0))
    return fail(MPC_E_ARG, "mpc_shaping_create: episode_length_s must be finite and > 0");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_shaping_create: no HIP device");
  mpc_shaping *h = new mpc_shaping();
  h->n = n;
  h->blocks = (n + kBlock - 1) / kBlock;
  h->device = device;
  h->c = taskcfg::to_device_config(*cfg);
  for (int i = 0; i < kTerms; ++i) h->k.scale[i] = (float)scales[i];
  h->k.base_height_target = (float)base_height_target;
  h->k.air_time_target = (float)air_time_target;
  h->k.dt = (float)dt;
  h->episode_length_s = episode_length_s;
  hipError_t e;
  if ((e = h->d_last_actions.alloc_zero((size_t)n * kDof)) != hipSuccess || (e = h->d_last_dof_vel.alloc_zero((size_t)n * kDof)) != hipSuccess ||
      (e = h->d_air_time.alloc_zero((size_t)n * kLegs)) != hipSuccess || (e = h->d_last_contact.alloc_zero((size_t)n * kLegs)) != hipSuccess ||
      (e = h->d_sums.alloc_zero((size_t)n * kTerms)) != hipSuccess || (e = h->d_ticks.alloc_zero((size_t)n)) != hipSuccess ||
      (e = h->d_partials.alloc_zero((size_t)h->blocks * kPartial)) != hipSuccess || (e = h->d_window.alloc_zero(kWords)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess) {
    mpc_shaping_destroy(h);
    return fail(MPC_E_HIP, std::string("mpc_shaping_create: ") + hipGetErrorString(e));
  }
  *out = h;
  return MPC_OK;
}

int mpc_shaping_bind(mpc_shaping *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_shaping_bind: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_shaping_bind: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_shaping_bind: the sim has " + std::to_string(s->n) + " robots, the reward shaping " + std::to_string(h->n) + " environments");
  if (!s->d_i32) return fail(MPC_E_ARG, "mpc_shaping_bind: the sim has no state record");
  if (s->device != h->device) return fail(MPC_E_ARG, "mpc_shaping_bind: the sim lives on another device");
  h->d_i32 = s->d_i32;
  return MPC_OK;
}

int mpc_shaping_close(mpc_shaping *h, const int *d_reset_ids, void *stream) {
  if (!h || !d_reset_ids) return fail(MPC_E_ARG, "mpc_shaping_close: null argument");
  DeviceGuard guard_(h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(shaping_close_kernel, dim3((unsigned)h->blocks), dim3(kEnvThreads), 0, s, h->n, d_reset_ids, h->d_sums, h->d_ticks, h->d_partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(shaping_join_kernel, dim3(1), dim3(kJoinThreads), 0, s, h->blocks, (const double *)h->d_partials, h->d_window);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_shaping_run(mpc_shaping *h, const float *d_root, const float *d_dof, const float *d_actions, const float *d_commands, const float *d_torques,
                    const unsigned char *d_fell, const int *d_reset_ids, const long long *d_reset, const long long *d_progress, const float *d_heights,
                    int P, float *d_rew, float *d_terms, void *stream) {
  if (!h || !d_root || !d_dof || !d_actions || !d_commands || !d_torques || !d_reset_ids || !d_reset || !d_progress || !d_rew)
    return fail(MPC_E_ARG, "mpc_shaping_run: null argument");
  if (P < 0 || P > MPC_SHAPING_MAX_POINTS) return fail(MPC_E_ARG, "mpc_shaping_run: P must lie in [0, 208]");
  if ((P > 0) != (d_heights != nullptr)) return fail(MPC_E_ARG, "mpc_shaping_run: d_heights goes with P >= 1, NULL with P = 0");
  if (((uintptr_t)d_reset | (uintptr_t)d_progress) & 7u) return fail(MPC_E_ARG, "mpc_shaping_run: d_reset and d_progress must be 8-byte aligned");
  if (!h->d_i32) return fail(MPC_E_ARG, "mpc_shaping_run: no sim bound (mpc_shaping_bind)");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(shaping_run_kernel, dim3((unsigned)((h->n + kRunEnvs - 1) / kRunEnvs)), dim3(kRunThreads), 0, reinterpret_cast<hipStream_t>(stream), h->c, h->k, h->n, d_root,
                     d_dof, d_actions, d_commands, d_torques, d_fell, d_reset_ids, d_reset, d_progress, h->d_i32, d_heights, P, h->d_last_actions,
                     h->d_last_dof_vel, h->d_air_time, h->d_last_contact, h->d_sums, h->d_ticks, d_rew, d_terms);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_shaping_summary(mpc_shaping *h, double *d_out, void *stream) {
  if (!h || !d_out) return fail(MPC_E_ARG, "mpc_shaping_summary: null argument");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(shaping_summary_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (const double *)h->d_window, h->episode_length_s,
                     d_out);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_shaping_new_window(mpc_shaping *h, void *stream) {
  if (!h) return fail(MPC_E_ARG, "mpc_shaping_new_window: null handle");
  DeviceGuard guard_(h->device);
  HIP_TRY(hipMemsetAsync(h->d_window, 0, sizeof(double) * kWords, reinterpret_cast<hipStream_t>(stream)));
  return MPC_OK;
}

int mpc_shaping_arrays(mpc_shaping *h, float **d_last_actions, float **d_last_dof_vel, float **d_air_time, int **d_last_contact, float **d_sums,
                       int **d_ticks, double **d_window) {
  if (!h || !d_last_actions || !d_last_dof_vel || !d_air_time || !d_last_contact || !d_sums || !d_ticks || !d_window)
    return fail(MPC_E_ARG, "mpc_shaping_arrays: null argument");
  *d_last_actions = h->d_last_actions;
  *d_last_dof_vel = h->d_last_dof_vel;
  *d_air_time = h->d_air_time;
  *d_last_contact = h->d_last_contact;
  *d_sums = h->d_sums;
  *d_ticks = h->d_ticks;
  *d_window = h->d_window;
  return MPC_OK;
}

}  // extern "C"
