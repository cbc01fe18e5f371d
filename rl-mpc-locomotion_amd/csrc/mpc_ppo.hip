// mpc_ppo.hip -- the C ABI of include/mpc_ppo.h: the collection half of a PPO iteration (ppo_rollout.h) on the device.
//   ac_kernel          actor and critic in one launch: grid (ceil(n / 16), nets), blockIdx.y picks the net, so the critic's workgroups run beside the
//                      actor's instead of after them.  A workgroup carries 16 environments through its net's layers with policy::layer
//                      (policy_mlp.h, unchanged): the mean is the k-ordered MFMA chain of mpc_policy_step.  The actor's workgroups end in the sampling
//                      / log-prob epilogue (one lane per environment and action pair, then one lane per environment for the ordered sum), the
//                      critic's write the value (the second net's whole output row: mpc_ac_act_distill puts a teacher's actor there, whose row is
//                      its twelve-column mean).  The weights are read through the caller's pointers: nothing is copied at bind time or later.
//   rollout_add_kernel one lane per environment: bootstrapped reward and done flag into slot t.
//   returns_kernel     one lane per environment walks t = T-1 .. 0 over [T][N] storage (consecutive lanes on consecutive words).
//   normalise_kernel   ONE workgroup: lane i sums elements i, i + 1024, ... in float64, a fixed-order LDS tree joins the lanes; mean, then squared
//                      deviations, then the rewrite.  No atomics, so a rerun is bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mpc_ppo.h"
#include "mpc_ac_internal.h"
#include "mpc_host.h"
#include "policy_mlp.h"
#include "ppo_rollout.h"

using mpchost::DeviceGuard;
using mpchost::present16;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kLaneThreads = 64;       // the per-environment kernels: one wave per workgroup, 4096 environments are 64 waves
constexpr int kNormThreads = 1024;
constexpr int kActor = 0, kCritic = 1;

struct Nets {
  policy::Net net[2];                  // actor, critic
  const float *std;                    // [12]
};

struct ActOut {
  float *actions, *log_prob, *values, *mean, *sigma, *eps;
};

// grid (ceil(n / 16), nets); net = first_net + blockIdx.y.  sample: the actor's epilogue draws actions (mpc_ac_act); otherwise it writes the mean alone.
// The second net writes its whole output row to out.values [n][its outputs]: one column for a critic, twelve where mpc_ac_act_distill has put a
// teacher's actor there (out.log_prob is then null and not written).
// actor_obs [n][actor dims[0]] and critic_obs [n][critic dims[0]]: each net's workgroups stage their own rows at their own width (the same pointer
// twice where both nets read the same observations); the pointer of a net that the launch does not run is never read.
__global__ __launch_bounds__(policy::kThreads) void ac_kernel(Nets nets, int first_net, int sample, int n, const float *__restrict__ actor_obs,
                                                             const float *__restrict__ critic_obs, unsigned long long seed, unsigned int step, ActOut out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int which = first_net + (int)blockIdx.y;
  const policy::Net &net = nets.net[which];
  const float *__restrict__ obs = which == kCritic ? critic_obs : actor_obs;
  int wmax_even = 0, wmax_odd = 0;     // widest activation held by buffer 0 (layers 0, 2, ...) / buffer 1, as mpc_policy.hip's mlp_kernel lays them out
  for (int l = 0; l <= net.n_layers; ++l) {
    int &m = (l & 1) ? wmax_odd : wmax_even;
    m = net.dims[l] > m ? net.dims[l] : m;
  }
  float *buf[2] = {lds, lds + policy::kRows * (wmax_even + policy::kPad)};
  const int stride[2] = {wmax_even + policy::kPad, wmax_odd + policy::kPad};
  const int r0 = blockIdx.x * policy::kRows, d0 = net.dims[0];
  for (int e = threadIdx.x; e < policy::kRows * d0; e += policy::kThreads) {
    const int r = e / d0, k = e - r * d0;
    buf[0][r * stride[0] + k] = (r0 + r < n) ? obs[(size_t)(r0 + r) * d0 + k] : 0.f;
  }
  __syncthreads();
  const int L = net.n_layers;
  for (int l = 0; l < L; ++l) {
    policy::layer(buf[l & 1], stride[l & 1], buf[(l + 1) & 1], stride[(l + 1) & 1], net.w[l], net.b[l], net.dims[l], net.dims[l + 1], l + 1 < L);
    __syncthreads();
  }
  const float *res = buf[L & 1];
  const int rs = stride[L & 1];
  const int e = threadIdx.x;
  if (which == kCritic) {                // the second net's output row, as wide as it is: a critic's value, or (mpc_ac_act_distill) a teacher's mean
    const int w = net.dims[L], r = e / w, k = e - r * w;
    if (e < policy::kRows * w && r0 + r < n) out.values[(size_t)(r0 + r) * w + k] = res[r * rs + k];
    return;
  }
  // the actor's epilogue.  terms: the other activation buffer, free since the last barrier (it holds at least 16 x (16 + 4) words: the last
  // layer's input is a multiple of 16 wide)
  float *terms = buf[(L + 1) & 1];
  const int r = e / ppo::kPairs, p = e - r * ppo::kPairs;
  const bool live = e < policy::kRows * ppo::kPairs && r0 + r < n;
  if (live) {
    const size_t o = (size_t)(r0 + r) * ppo::kActions + 2 * p;
    const float m0 = res[r * rs + 2 * p], m1 = res[r * rs + 2 * p + 1];
    *reinterpret_cast<float2 *>(out.mean + o) = make_float2(m0, m1);
    if (sample) {
      const float s0 = nets.std[2 * p], s1 = nets.std[2 * p + 1];
      float z0, z1;
      ppo::normal_pair(seed, (uint32_t)(r0 + r), step, (uint32_t)p, z0, z1);
      const float a0 = ppo::action_of(m0, s0, z0), a1 = ppo::action_of(m1, s1, z1);
      terms[r * ppo::kActions + 2 * p] = ppo::log_prob_term(a0, m0, s0);
      terms[r * ppo::kActions + 2 * p + 1] = ppo::log_prob_term(a1, m1, s1);
      *reinterpret_cast<float2 *>(out.actions + o) = make_float2(a0, a1);
      *reinterpret_cast<float2 *>(out.sigma + o) = make_float2(s0, s1);
      if (out.eps) *reinterpret_cast<float2 *>(out.eps + o) = make_float2(z0, z1);
    }
  }
  if (!sample) return;
  __syncthreads();
  if (out.log_prob && e < policy::kRows && r0 + e < n) out.log_prob[r0 + e] = ppo::log_prob_sum(terms + e * ppo::kActions);
}

mpchost::LdsLimit g_ac_limit(ac_kernel);

__global__ __launch_bounds__(kLaneThreads) void rollout_add_kernel(int n, float gamma, const float *__restrict__ rew, const long long *__restrict__ reset,
                                                                   const long long *__restrict__ timeout, const float *__restrict__ values_t,
                                                                   float *__restrict__ rewards_t, float *__restrict__ dones_t) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  rewards_t[r] = ppo::bootstrap(rew[r], gamma, values_t[r], timeout[r] != 0 ? 1.0f : 0.0f);
  dones_t[r] = reset[r] != 0 ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(kLaneThreads) void returns_kernel(int n, int T, float gamma, float lam, const float *__restrict__ rewards,
                                                               const float *__restrict__ dones, const float *__restrict__ values,
                                                               const float *__restrict__ last_values, float *__restrict__ returns,
                                                               float *__restrict__ adv) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  ppo::gae_column(T, (size_t)n, rewards + r, dones + r, values + r, last_values[r], gamma, lam, returns + r, adv + r);
}

// sum over the workgroup of one float64 per lane, in a fixed order; every lane gets the result
__device__ __forceinline__ double block_sum(double v, double *tree) {
  __syncthreads();                     // (the previous use of the tree has been read)
  tree[threadIdx.x] = v;
  __syncthreads();
  for (int s = kNormThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) tree[threadIdx.x] += tree[threadIdx.x + s];
    __syncthreads();
  }
  return tree[0];
}

__global__ __launch_bounds__(kNormThreads) void normalise_kernel(size_t m, float *__restrict__ adv) {
  __shared__ double tree[kNormThreads];
  double s = 0.0;
#pragma unroll 8
  for (size_t i = threadIdx.x; i < m; i += kNormThreads) s += (double)adv[i];
  const double mean = block_sum(s, tree) / (double)m;
  double q = 0.0;
#pragma unroll 8
  for (size_t i = threadIdx.x; i < m; i += kNormThreads) {
    const double d = (double)adv[i] - mean;
    q += d * d;
  }
  const double std = sqrt(block_sum(q, tree) / (double)(m - 1));
#pragma unroll 8
  for (size_t i = threadIdx.x; i < m; i += kNormThreads) adv[i] = ppo::normalise_one(adv[i], mean, std);
}

bool unit_interval(double x) { return std::isfinite(x) && x >= 0.0 && x <= 1.0; }

// the limits of mpc_policy_create on one stack, with the width of its output fixed
const char *check_stack(int n_layers, const int *dims, int outputs) {
  if (n_layers <= 0 || n_layers > policy::kMaxLayers || !dims) return "1 .. 8 layers and their widths";
  for (int l = 0; l < n_layers; ++l)
    if (dims[l] <= 0 || dims[l] % 16 != 0) return "layer input widths must be positive multiples of 16";
  if (dims[n_layers] <= 0 || dims[n_layers] > 16) return "1 .. 16 outputs";
  if (dims[n_layers] != outputs) return outputs == 1 ? "the critic has one output" : "the actor has twelve outputs";
  return nullptr;
}
}  // namespace

struct mpc_ac {
  Nets nets{};
  size_t lds = 0;
  int device = -1;
  bool bound = false;
  bool asymmetric = false;             // made by mpc_ac_create_asymmetric: the critic reads rows of its own
};

// mpc_ac_internal.h: the handle as the update unit (mpc_ppo_update.hip) sees it
bool mpc_ac_get_view(const mpc_ac *ac, mpc_ac_view *out) {
  if (!ac || !out) return false;
  for (int k = 0; k < 2; ++k) {
    const policy::Net &net = ac->nets.net[k];
    out->n_layers[k] = net.n_layers;
    for (int l = 0; l <= net.n_layers; ++l) out->dims[k][l] = net.dims[l];
    for (int l = 0; l < net.n_layers; ++l) {
      out->w[k][l] = net.w[l];
      out->b[k][l] = net.b[l];
    }
  }
  out->std = ac->nets.std;
  out->device = ac->device;
  out->bound = ac->bound;
  out->asymmetric = ac->asymmetric;
  return true;
}

int mpc_ppo_set_error(int code, const char *message) { return fail(code, message); }

extern "C" {

const char *mpc_ppo_last_error(void) { return g_err.c_str(); }

void mpc_ac_destroy(mpc_ac *ac) { delete ac; }      // owns no device memory: the parameters are the caller's

// mpc_ac_create and mpc_ac_create_asymmetric: the same limits per stack, the LDS limit on the wider of the two
static int ac_create(const char *who, bool asymmetric, mpc_ac **out, int n_actor_layers, const int *actor_dims, int n_critic_layers, const int *critic_dims) {
  const std::string name(who);
  if (!out) return fail(MPC_E_ARG, name + ": bad argument");
  if (const char *why = check_stack(n_actor_layers, actor_dims, MPC_AC_ACTIONS)) return fail(MPC_E_ARG, name + ": actor: " + why);
  if (const char *why = check_stack(n_critic_layers, critic_dims, 1)) return fail(MPC_E_ARG, name + ": critic: " + why);
  if (!asymmetric && actor_dims[0] != critic_dims[0])
    return fail(MPC_E_ARG, name + ": actor and critic read the same observations (equal input widths)");
  mpc_ac *ac = new mpc_ac();
  ac->asymmetric = asymmetric;
  const int nl[2] = {n_actor_layers, n_critic_layers};
  const int *dims[2] = {actor_dims, critic_dims};
  for (int k = 0; k < 2; ++k) {
    ac->nets.net[k].n_layers = nl[k];
    for (int l = 0; l <= nl[k]; ++l) ac->nets.net[k].dims[l] = dims[k][l];
    const size_t b = policy::lds_bytes(ac->nets.net[k]);
    ac->lds = b > ac->lds ? b : ac->lds;
  }
  if (ac->lds > 160 * 1024) { delete ac; return fail(MPC_E_ARG, name + ": layers too wide for one CU's LDS"); }
  *out = ac;
  return MPC_OK;
}

int mpc_ac_create(mpc_ac **out, int n_actor_layers, const int *actor_dims, int n_critic_layers, const int *critic_dims) {
  return ac_create("mpc_ac_create", false, out, n_actor_layers, actor_dims, n_critic_layers, critic_dims);
}

int mpc_ac_create_asymmetric(mpc_ac **out, int n_actor_layers, const int *actor_dims, int n_critic_layers, const int *critic_dims) {
  return ac_create("mpc_ac_create_asymmetric", true, out, n_actor_layers, actor_dims, n_critic_layers, critic_dims);
}

int mpc_ac_bind(mpc_ac *ac, const float *const *d_actor_weights, const float *const *d_actor_biases, const float *const *d_critic_weights,
                const float *const *d_critic_biases, const float *d_std) {
  if (!ac || !d_actor_weights || !d_actor_biases || !d_critic_weights || !d_critic_biases) return fail(MPC_E_ARG, "mpc_ac_bind: bad argument");
  const float *const *w[2] = {d_actor_weights, d_critic_weights};
  const float *const *b[2] = {d_actor_biases, d_critic_biases};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < ac->nets.net[k].n_layers; ++l)
      if (!present16(w[k][l]) || !present16(b[k][l])) return fail(MPC_E_ARG, "mpc_ac_bind: every weight and bias pointer must be non-null and 16-byte aligned");
  if (!present16(d_std)) return fail(MPC_E_ARG, "mpc_ac_bind: d_std must be non-null and 16-byte aligned");
  const int dev = mpchost::current_device();
  if (dev < 0) return fail(MPC_E_NODEVICE, "mpc_ac_bind: no HIP device");
  if (g_ac_limit.raise(dev, ac->lds) != hipSuccess)
    return fail(MPC_E_HIP, "mpc_ac_bind: device set-up failed");
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < ac->nets.net[k].n_layers; ++l) {
      ac->nets.net[k].w[l] = w[k][l];
      ac->nets.net[k].b[l] = b[k][l];
    }
  ac->nets.std = d_std;
  ac->device = dev;
  ac->bound = true;
  return MPC_OK;
}

static int launch_nets(const Nets &pair, size_t lds, int device, int n, const float *d_obs, const float *d_critic_obs, int first_net, int nets, int sample,
                       unsigned long long seed, unsigned int step, const ActOut &o, void *stream) {
  DeviceGuard guard_(device);
  const dim3 grid((unsigned)((n + policy::kRows - 1) / policy::kRows), (unsigned)nets);
  hipLaunchKernelGGL(ac_kernel, grid, dim3(policy::kThreads), lds, reinterpret_cast<hipStream_t>(stream), pair, first_net, sample, n, d_obs, d_critic_obs,
                     seed, step, o);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

static int ac_launch(mpc_ac *ac, int n, const float *d_obs, const float *d_critic_obs, int first_net, int nets, int sample, unsigned long long seed,
                     unsigned int step, const ActOut &o, void *stream) {
  return launch_nets(ac->nets, ac->lds, ac->device, n, d_obs, d_critic_obs, first_net, nets, sample, seed, step, o, stream);
}

int mpc_ac_act(mpc_ac *ac, int n, const float *d_obs, unsigned long long seed, unsigned int step, float *d_actions, float *d_log_prob, float *d_values,
               float *d_mean, float *d_sigma, float *d_eps, void *stream) {
  if (!ac || n <= 0 || !d_obs || !d_actions || !d_log_prob || !d_values || !d_mean || !d_sigma) return fail(MPC_E_ARG, "mpc_ac_act: bad argument");
  // (rows of twelve floats are written as 8-byte pairs)
  if ((reinterpret_cast<uintptr_t>(d_actions) | reinterpret_cast<uintptr_t>(d_mean) | reinterpret_cast<uintptr_t>(d_sigma) | reinterpret_cast<uintptr_t>(d_eps)) & 7u)
    return fail(MPC_E_ARG, "mpc_ac_act: d_actions, d_mean, d_sigma and d_eps must be 8-byte aligned");
  if (ac->nets.net[kActor].dims[0] != ac->nets.net[kCritic].dims[0])
    return fail(MPC_E_ARG, "mpc_ac_act: the critic of this asymmetric handle reads rows of another width: use mpc_ac_act_asymmetric");
  if (!ac->bound) return fail(MPC_E_ARG, "mpc_ac_act: no parameters bound (mpc_ac_bind)");
  return ac_launch(ac, n, d_obs, d_obs, kActor, 2, 1, seed, step, ActOut{d_actions, d_log_prob, d_values, d_mean, d_sigma, d_eps}, stream);
}

int mpc_ac_act_asymmetric(mpc_ac *ac, int n, const float *d_obs, const float *d_critic_obs, unsigned long long seed, unsigned int step, float *d_actions,
                          float *d_log_prob, float *d_values, float *d_mean, float *d_sigma, float *d_eps, void *stream) {
  if (!ac || n <= 0 || !d_obs || !d_actions || !d_log_prob || !d_values || !d_mean || !d_sigma) return fail(MPC_E_ARG, "mpc_ac_act_asymmetric: bad argument");
  if (!d_critic_obs) return fail(MPC_E_ARG, "mpc_ac_act_asymmetric: d_critic_obs is null");
  if ((reinterpret_cast<uintptr_t>(d_actions) | reinterpret_cast<uintptr_t>(d_mean) | reinterpret_cast<uintptr_t>(d_sigma) | reinterpret_cast<uintptr_t>(d_eps)) & 7u)
    return fail(MPC_E_ARG, "mpc_ac_act_asymmetric: d_actions, d_mean, d_sigma and d_eps must be 8-byte aligned");
  if (!ac->bound) return fail(MPC_E_ARG, "mpc_ac_act_asymmetric: no parameters bound (mpc_ac_bind)");
  return ac_launch(ac, n, d_obs, d_critic_obs, kActor, 2, 1, seed, step, ActOut{d_actions, d_log_prob, d_values, d_mean, d_sigma, d_eps}, stream);
}

int mpc_ac_evaluate(mpc_ac *ac, int n, const float *d_obs, float *d_values, void *stream) {
  if (!ac || n <= 0 || !d_obs || !d_values) return fail(MPC_E_ARG, "mpc_ac_evaluate: bad argument");
  if (!ac->bound) return fail(MPC_E_ARG, "mpc_ac_evaluate: no parameters bound (mpc_ac_bind)");
  return ac_launch(ac, n, nullptr, d_obs, kCritic, 1, 0, 0, 0, ActOut{nullptr, nullptr, d_values, nullptr, nullptr, nullptr}, stream);
}

int mpc_ac_act_inference(mpc_ac *ac, int n, const float *d_obs, float *d_mean, void *stream) {
  if (!ac || n <= 0 || !d_obs || !d_mean || (reinterpret_cast<uintptr_t>(d_mean) & 7u)) return fail(MPC_E_ARG, "mpc_ac_act_inference: bad argument");
  if (!ac->bound) return fail(MPC_E_ARG, "mpc_ac_act_inference: no parameters bound (mpc_ac_bind)");
  return ac_launch(ac, n, d_obs, nullptr, kActor, 1, 0, 0, 0, ActOut{nullptr, nullptr, nullptr, d_mean, nullptr, nullptr}, stream);
}

// ac_kernel's two halves over two handles: the student's actor with the sampling epilogue, and the teacher's actor where a critic sits otherwise.
// The dynamic LDS is the larger of the two handles' own (ac_kernel's limit on this device holds both since their binds).
int mpc_ac_act_distill(mpc_ac *student, mpc_ac *teacher, int n, const float *d_obs, const float *d_teacher_obs, unsigned long long seed, unsigned int step,
                       float *d_actions, float *d_mean, float *d_sigma, float *d_teacher_actions, float *d_eps, void *stream) {
  if (!student || !teacher || n <= 0 || !d_obs || !d_actions || !d_mean || !d_sigma) return fail(MPC_E_ARG, "mpc_ac_act_distill: bad argument");
  if (!d_teacher_obs || !d_teacher_actions) return fail(MPC_E_ARG, "mpc_ac_act_distill: d_teacher_obs or d_teacher_actions is null");
  if ((reinterpret_cast<uintptr_t>(d_actions) | reinterpret_cast<uintptr_t>(d_mean) | reinterpret_cast<uintptr_t>(d_sigma) | reinterpret_cast<uintptr_t>(d_eps)) & 7u)
    return fail(MPC_E_ARG, "mpc_ac_act_distill: d_actions, d_mean, d_sigma and d_eps must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_teacher_actions) & 3u) return fail(MPC_E_ARG, "mpc_ac_act_distill: d_teacher_actions must be 4-byte aligned");
  if (!student->bound) return fail(MPC_E_ARG, "mpc_ac_act_distill: the student has no parameters bound (mpc_ac_bind)");
  if (!teacher->bound) return fail(MPC_E_ARG, "mpc_ac_act_distill: the teacher has no parameters bound (mpc_ac_bind)");
  if (student->device != teacher->device) return fail(MPC_E_ARG, "mpc_ac_act_distill: the student and the teacher are bound on different devices");
  Nets pair{};
  pair.net[0] = student->nets.net[kActor];
  pair.net[1] = teacher->nets.net[kActor];
  pair.std = student->nets.std;
  return launch_nets(pair, student->lds > teacher->lds ? student->lds : teacher->lds, student->device, n, d_obs, d_teacher_obs, 0, 2, 1, seed, step,
                     ActOut{d_actions, nullptr, d_teacher_actions, d_mean, d_sigma, d_eps}, stream);
}

int mpc_rollout_add(int n, double gamma, const float *d_rew, const long long *d_reset, const long long *d_timeout, const float *d_values_t,
                    float *d_rewards_t, float *d_dones_t, void *stream) {
  if (n <= 0 || !d_rew || !d_reset || !d_timeout || !d_values_t || !d_rewards_t || !d_dones_t) return fail(MPC_E_ARG, "mpc_rollout_add: bad argument");
  if (!unit_interval(gamma)) return fail(MPC_E_ARG, "mpc_rollout_add: gamma must lie in [0, 1]");
  hipLaunchKernelGGL(rollout_add_kernel, dim3((unsigned)((n + kLaneThreads - 1) / kLaneThreads)), dim3(kLaneThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     n, (float)gamma, d_rew, d_reset, d_timeout, d_values_t, d_rewards_t, d_dones_t);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_rollout_returns(int n, int T, double gamma, double lam, const float *d_rewards, const float *d_dones, const float *d_values,
                        const float *d_last_values, float *d_returns, float *d_advantages, void *stream) {
  if (n <= 0 || T <= 0 || !d_rewards || !d_dones || !d_values || !d_last_values || !d_returns || !d_advantages)
    return fail(MPC_E_ARG, "mpc_rollout_returns: bad argument");
  if (!unit_interval(gamma) || !unit_interval(lam)) return fail(MPC_E_ARG, "mpc_rollout_returns: gamma and lam must lie in [0, 1]");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(returns_kernel, dim3((unsigned)((n + kLaneThreads - 1) / kLaneThreads)), dim3(kLaneThreads), 0, s, n, T, (float)gamma, (float)lam,
                     d_rewards, d_dones, d_values, d_last_values, d_returns, d_advantages);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(normalise_kernel, dim3(1), dim3(kNormThreads), 0, s, (size_t)n * (size_t)T, d_advantages);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
