// mpc_episode_terms.hip -- the C ABI of mpc_episode_terms.h: the per-term episode reward sums and the command curriculum (episode_terms.h) on
// the device, in four kernels and at most four launches per tick.
//   terms_close_kernel       one lane per environment, one wave per workgroup like task_begin_kernel.  A marked lane (id >= 0) puts its float32
//                            sums and its closed flag into LDS, zeroes its sums and ticks and counts the resample; lanes 0 .. 6 then each add one
//                            word of the block's partial over the wave's 64 environments in environment order, in float64, and write it.
//   terms_join_kernel        ONE workgroup of 256: the block partials are staged 256 rows at a time into LDS (consecutive lanes on consecutive
//                            words), and lanes 0 .. 6 each add one word over the staged rows in block order; lane 0 then takes the decision, updates
//                            the x range, the widenings and the window accumulators.
//   terms_resample_kernel    one lane per environment: a marked lane draws its three commands from the ranges the join has just left.  Launched
//                            with a curriculum only.
//   terms_accumulate_kernel  one lane per environment: the six terms from what `finish` read, sums += terms, ticks += 1.
// No atomics; the order of every sum is fixed, so a rerun from the same state is bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "episode_terms.h"
#include "mpc_episode_terms.h"
#include "mpc_host.h"
#include "mpc_task_config.h"

using epterms::Curriculum;
using epterms::kBlock;
using epterms::kPartial;
using epterms::kTerms;
using mpchost::DeviceArray;
using mpchost::DeviceGuard;

static_assert(MPC_EPISODE_TERMS_SUMMARY == epterms::kSummaryLen && MPC_EPISODE_TERMS_STATE == epterms::kGlobLen && MPC_TASK_REW_TERMS == kTerms,
              "mpc_episode_terms.h and episode_terms.h disagree");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kEnvThreads = kBlock;    // one wave per workgroup, and one workgroup per block of the reduction
constexpr int kJoinThreads = 256;      // block partials staged per pass of the join
constexpr int kRow = kTerms + 1;       // LDS row stride of the close kernel: 7 words, odd, so the 64 lanes' stores spread over the banks

__global__ __launch_bounds__(kEnvThreads) void terms_close_kernel(int n, const int *__restrict__ ids, float *sums, int *ticks, int *counts,
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
    cl = epterms::closes(ids[r], ticks[r], s) ? 1 : 0;
    ticks[r] = 0;
    counts[r] = counts[r] + 1;
  }
  closed[lane] = cl;
  __syncthreads();
  if (lane < kPartial)
    partials[(size_t)blockIdx.x * kPartial + lane] = epterms::block_partial_word(min(kEnvThreads, n - first), closed, rows, kRow, lane);
}

__global__ __launch_bounds__(kJoinThreads) void terms_join_kernel(int blocks, const double *__restrict__ partials, Curriculum k, double *glob) {
  __shared__ double stage[kJoinThreads * kPartial];
  __shared__ double S[kPartial];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int base = 0; base < blocks; base += kJoinThreads) {
    const int here = min(kJoinThreads, blocks - base);
    for (int i = tid; i < here * kPartial; i += kJoinThreads) stage[i] = partials[(size_t)base * kPartial + i];
    __syncthreads();
    if (tid < kPartial) acc = epterms::join_word(acc, here, stage, tid);
    __syncthreads();                   // the words are read before the next pass overwrites them
  }
  if (tid < kPartial) S[tid] = acc;
  __syncthreads();
  if (tid == 0) epterms::join_tail(k, S, glob);
}

__global__ __launch_bounds__(kEnvThreads) void terms_resample_kernel(int n, unsigned long long seed, const int *__restrict__ ids,
                                                                     const int *__restrict__ counts, const double *__restrict__ glob,
                                                                     float *commands) {
  const int r = blockIdx.x * kEnvThreads + threadIdx.x;
  if (r >= n || ids[r] < 0) return;
  double ranges[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) ranges[i] = glob[epterms::kGlobRanges + i];
  float cmd[3];
  epterms::resample_env(seed, r, counts[r], ranges, cmd);
#pragma unroll
  for (int a = 0; a < 3; ++a) commands[(size_t)r * 3 + a] = cmd[a];
}

__global__ __launch_bounds__(kEnvThreads) void terms_accumulate_kernel(rltask::Config c, int n, const float *__restrict__ root,
                                                                       const float *__restrict__ commands, const float *__restrict__ torques,
                                                                       const unsigned char *__restrict__ fell, float *sums, int *ticks,
                                                                       float *terms_out) {
  const int r = blockIdx.x * kEnvThreads + threadIdx.x;
  if (r >= n) return;
  float rt[13], cmd[3], tq[12], terms[kTerms], s[kTerms];
#pragma unroll
  for (int i = 0; i < 13; ++i) rt[i] = root[(size_t)r * 13 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) cmd[i] = commands[(size_t)r * 3 + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) tq[i] = torques[(size_t)r * 12 + i];
  epterms::reward_terms(c, rt, cmd, tq, rltask::contacts_from_fell(fell != nullptr && fell[r] != 0), terms);
#pragma unroll
  for (int i = 0; i < kTerms; ++i) s[i] = sums[(size_t)r * kTerms + i];
  int t = ticks[r];
  epterms::accumulate_env(terms, s, t);
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sums[(size_t)r * kTerms + i] = s[i];
  ticks[r] = t;
  if (terms_out) {
#pragma unroll
    for (int i = 0; i < kTerms; ++i) terms_out[(size_t)r * kTerms + i] = terms[i];
  }
}

__global__ __launch_bounds__(64) void terms_summary_kernel(const double *__restrict__ glob, double episode_length_s, double *out) {
  const int j = threadIdx.x;
  if (j <= kTerms) out[epterms::kSumClosed + j] = glob[epterms::kGlobWindow + j];
  if (j == 0) {
    out[epterms::kSumLo] = glob[epterms::kGlobRanges + 0];
    out[epterms::kSumHi] = glob[epterms::kGlobRanges + 1];
    out[epterms::kSumWidenings] = glob[epterms::kGlobWidenings];
    out[epterms::kSumEpisodeS] = episode_length_s;
  }
}
}  // namespace

struct mpc_episode_terms {
  int n = 0, blocks = 0, device = 0;
  rltask::Config c{};
  bool curriculum = false;
  Curriculum k{};
  double episode_length_s = 0.0;
  DeviceArray<float> d_sums;           // [n][6]
  DeviceArray<int> d_ticks, d_counts;  // [n] each
  DeviceArray<double> d_partials;      // [blocks][kPartial]
  DeviceArray<double> d_glob;          // [kGlobLen]
};

static dim3 env_grid(const mpc_episode_terms *h) { return dim3((unsigned)h->blocks); }

extern "C" {

const char *mpc_episode_terms_last_error(void) { return g_err.c_str(); }

void mpc_episode_terms_destroy(mpc_episode_terms *h) { mpchost::destroy_handle(h); }

int mpc_episode_terms_create(mpc_episode_terms **out, int n, const mpc_task_config *cfg, double episode_length_s, int curriculum, double x_lo0,
                             double x_hi0, double step, double threshold, double max_curriculum, long long update_every) {
  // everything is validated before the device is touched
  if (!out || !cfg) return fail(MPC_E_ARG, "mpc_episode_terms_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_episode_terms_create: n must be at least 1");
  // (neither default_dof_pos nor clip_observations is checked: the terms read neither)
  const taskcfg::Fault bad = taskcfg::check(*cfg);
  if (bad == taskcfg::kNotFinite) return fail(MPC_E_ARG, "mpc_episode_terms_create: a scale or a command range is not finite");
  if (bad == taskcfg::kRangeOrder) return fail(MPC_E_ARG, "mpc_episode_terms_create: command range with min > max");
  if (bad == taskcfg::kEpisodeLength) return fail(MPC_E_ARG, "mpc_episode_terms_create: max_episode_length must be at least 1");
  if (!std::isfinite(episode_length_s) || !(episode_length_s > 0.0))
    return fail(MPC_E_ARG, "mpc_episode_terms_create: episode_length_s must be finite and > 0");
  if (curriculum) {
    if (!std::isfinite(x_lo0) || !std::isfinite(x_hi0) || !(x_lo0 <= 0.0 && 0.0 <= x_hi0))
      return fail(MPC_E_ARG, "mpc_episode_terms_create: the initial x range must satisfy lo <= 0 <= hi");
    if (!std::isfinite(max_curriculum) || !(max_curriculum >= std::fmax(std::fabs(x_lo0), std::fabs(x_hi0))))
      return fail(MPC_E_ARG, "mpc_episode_terms_create: max_curriculum must be finite and at least max(|lo|, |hi|) of the initial x range");
    if (!std::isfinite(step) || !(step > 0.0)) return fail(MPC_E_ARG, "mpc_episode_terms_create: step must be finite and > 0");
    if (!std::isfinite(threshold)) return fail(MPC_E_ARG, "mpc_episode_terms_create: threshold must be finite");
    if (update_every < 1) return fail(MPC_E_ARG, "mpc_episode_terms_create: update_every must be at least 1");
  }
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_episode_terms_create: no HIP device");
  mpc_episode_terms *h = new mpc_episode_terms();
  h->n = n;
  h->blocks = (n + kBlock - 1) / kBlock;
  h->device = device;
  h->c = taskcfg::to_device_config(*cfg);      // what the reward terms read
  h->curriculum = curriculum != 0;
  h->episode_length_s = episode_length_s;
  h->k = Curriculum{0, 0, h->curriculum ? update_every : 1, (double)cfg->max_episode_length, threshold, (double)h->c.rew[rltask::kRewLinVelXY], step,
                    max_curriculum};
  double glob[epterms::kGlobLen] = {};
  for (int a = 0; a < 3; ++a) { glob[2 * a] = cfg->command_range[a][0]; glob[2 * a + 1] = cfg->command_range[a][1]; }
  if (h->curriculum) { glob[0] = x_lo0; glob[1] = x_hi0; }
  hipError_t e;
  if ((e = h->d_sums.alloc_zero((size_t)n * kTerms)) != hipSuccess || (e = h->d_ticks.alloc_zero((size_t)n)) != hipSuccess ||
      (e = h->d_counts.alloc_zero((size_t)n)) != hipSuccess || (e = h->d_partials.alloc_zero((size_t)h->blocks * kPartial)) != hipSuccess ||
      (e = h->d_glob.alloc_copy(glob, epterms::kGlobLen)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
    mpc_episode_terms_destroy(h);
    return fail(MPC_E_HIP, std::string("mpc_episode_terms_create: ") + hipGetErrorString(e));
  }
  *out = h;
  return MPC_OK;
}

int mpc_episode_terms_close_and_resample(mpc_episode_terms *h, const int *d_reset_ids, float *d_commands, long long tick, int curriculum_enabled,
                                         void *stream) {
  if (!h || !d_reset_ids) return fail(MPC_E_ARG, "mpc_episode_terms_close_and_resample: null argument");
  if (h->curriculum && !d_commands) return fail(MPC_E_ARG, "mpc_episode_terms_close_and_resample: a command curriculum needs d_commands");
  if (tick < 0) return fail(MPC_E_ARG, "mpc_episode_terms_close_and_resample: tick must be >= 0");
  Curriculum k = h->k;
  k.enabled = h->curriculum && curriculum_enabled ? 1 : 0;
  k.tick = tick;
  DeviceGuard guard_(h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(terms_close_kernel, env_grid(h), dim3(kEnvThreads), 0, s, h->n, d_reset_ids, h->d_sums, h->d_ticks, h->d_counts, h->d_partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(terms_join_kernel, dim3(1), dim3(kJoinThreads), 0, s, h->blocks, (const double *)h->d_partials, k, h->d_glob);
  HIP_TRY(hipGetLastError());
  if (h->curriculum) {
    hipLaunchKernelGGL(terms_resample_kernel, env_grid(h), dim3(kEnvThreads), 0, s, h->n, h->c.seed, d_reset_ids, (const int *)h->d_counts,
                       (const double *)h->d_glob, d_commands);
    HIP_TRY(hipGetLastError());
  }
  return MPC_OK;
}

int mpc_episode_terms_accumulate(mpc_episode_terms *h, const float *d_root, const float *d_commands, const float *d_torques,
                                 const unsigned char *d_fell, float *d_terms, void *stream) {
  if (!h || !d_root || !d_commands || !d_torques) return fail(MPC_E_ARG, "mpc_episode_terms_accumulate: null argument");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(terms_accumulate_kernel, env_grid(h), dim3(kEnvThreads), 0, reinterpret_cast<hipStream_t>(stream), h->c, h->n, d_root, d_commands,
                     d_torques, d_fell, h->d_sums, h->d_ticks, d_terms);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_episode_terms_summary(mpc_episode_terms *h, double *d_out, void *stream) {
  if (!h || !d_out) return fail(MPC_E_ARG, "mpc_episode_terms_summary: null argument");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(terms_summary_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (const double *)h->d_glob, h->episode_length_s,
                     d_out);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_episode_terms_new_window(mpc_episode_terms *h, void *stream) {
  if (!h) return fail(MPC_E_ARG, "mpc_episode_terms_new_window: null handle");
  DeviceGuard guard_(h->device);
  HIP_TRY(hipMemsetAsync(h->d_glob + epterms::kGlobWindow, 0, sizeof(double) * (1 + kTerms), reinterpret_cast<hipStream_t>(stream)));
  return MPC_OK;
}

int mpc_episode_terms_arrays(mpc_episode_terms *h, float **d_sums, int **d_ticks, int **d_counts, double **d_state) {
  if (!h || !d_sums || !d_ticks || !d_counts || !d_state) return fail(MPC_E_ARG, "mpc_episode_terms_arrays: null argument");
  *d_sums = h->d_sums;
  *d_ticks = h->d_ticks;
  *d_counts = h->d_counts;
  *d_state = h->d_glob;
  return MPC_OK;
}

}  // extern "C"
