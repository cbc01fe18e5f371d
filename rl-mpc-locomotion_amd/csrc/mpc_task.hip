// mpc_task.hip -- the C ABI of include/mpc_task.h: the RL task's post-physics half (rl_task.h) on the device, in two kernels.
//   task_begin_kernel   one lane per environment: time-out flag, episode counter, reset ids, fresh commands.
//   task_finish_kernel  one lane per environment computes its 48 observations into LDS, reward and reset flag into registers; the wave then
//                       writes its 64 x 48 observation block with consecutive lanes on consecutive words (a lane writing its own row would put
//                       the lanes of a store 192 bytes apart).  One wave per workgroup, so the one barrier between the two halves is a wave's.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mpc_task.h"
#include "mpc_host.h"
#include "mpc_task_config.h"
#include "rl_task.h"

using namespace rltask;
using mpchost::DeviceGuard;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kTaskThreads = 64;     // one wave per workgroup: 4096 environments are 64 waves
constexpr int kRowPad = kObs + 1;    // LDS row stride: 49 words, so the 64 lanes writing entry j of their rows hit 64 different banks

struct ContactArgs {
  const float *forces;               // [n][bodies][3] or null
  const unsigned char *fell;         // [n] or null
  int bodies, base;
  int knee[kLegs], hip[kLegs];
};

__global__ __launch_bounds__(kTaskThreads) void task_begin_kernel(Config c, int n, long long *progress, long long *reset, long long *timeout,
                                                                  int *episode, int *ids, float *commands) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  long long p = progress[r], rs = reset[r], to;
  int ep = episode[r];
  float cmd[3];
  const int id = begin_env(c, r, p, rs, to, ep, cmd);
  timeout[r] = to;
  progress[r] = p;
  ids[r] = id;
  if (id >= 0) {
    reset[r] = rs;
    episode[r] = ep;
#pragma unroll
    for (int a = 0; a < 3; ++a) commands[(size_t)r * 3 + a] = cmd[a];
  }
}

__global__ __launch_bounds__(kTaskThreads) void task_finish_kernel(Config c, int n, const float *__restrict__ root, const float *__restrict__ dof,
                                                                   const float *__restrict__ commands, const float *__restrict__ actions,
                                                                   const float *__restrict__ torques, ContactArgs k,
                                                                   const long long *__restrict__ progress, float *__restrict__ obs,
                                                                   float *__restrict__ rew, long long *__restrict__ reset) {
  __shared__ float rows[kTaskThreads * kRowPad];
  const int lane = threadIdx.x;
  const int first = blockIdx.x * kTaskThreads;
  const int r = first + lane;
  if (r < n) {
    float rt[13], cmd[3], tq[12];
#pragma unroll
    for (int i = 0; i < 13; ++i) rt[i] = root[(size_t)r * 13 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) cmd[i] = commands[(size_t)r * 3 + i];
#pragma unroll
    for (int i = 0; i < 12; ++i) tq[i] = torques[(size_t)r * 12 + i];
    observe(c, rt, dof + (size_t)r * 24, cmd, actions + (size_t)r * 12, rows + lane * kRowPad);
    Contacts ct{false, false, 0};
    if (k.forces) ct = contacts_from_forces(k.forces + (size_t)r * 3 * k.bodies, k.base, k.knee, k.hip);
    if (k.fell) ct.base = ct.base || k.fell[r] != 0;
    bool rs;
    rew[r] = reward_reset(c, rt, cmd, tq, ct, progress[r], rs);
    reset[r] = rs ? 1 : 0;
  }
  __syncthreads();
  const int rows_here = min(kTaskThreads, n - first);
  float *out = obs + (size_t)first * kObs;
#pragma unroll 4
  for (int i = 0; i < kObs; ++i) {
    const int f = i * kTaskThreads + lane;       // word f of the block's rows_here x 48 output
    const int e = f / kObs;
    if (e < rows_here) out[f] = rows[e * kRowPad + (f - e * kObs)];
  }
}
}  // namespace

struct mpc_task {
  int n = 0, device = 0;
  Config c{};
  mpchost::DeviceArray<int> d_episode; // [n] how many times each environment has been reset: the generator's episode index
  mpc_task_buffer_set b{};
  bool bound = false;
};

static dim3 task_grid(int n) { return dim3((unsigned)((n + kTaskThreads - 1) / kTaskThreads)); }

extern "C" {

const char *mpc_task_last_error(void) { return g_err.c_str(); }

void mpc_task_destroy(mpc_task *t) { mpchost::destroy_handle(t); }

int mpc_task_create(mpc_task **out, int n, const mpc_task_config *cfg) {
  if (!out || n <= 0 || !cfg) return fail(MPC_E_ARG, "mpc_task_create: bad argument");
  const taskcfg::Fault bad = taskcfg::check(*cfg);
  if (bad == taskcfg::kNotFinite || !taskcfg::finite_all(cfg->default_dof_pos, 12))
    return fail(MPC_E_ARG, "mpc_task_create: a scale, a command range or a default joint angle is not finite");
  if (bad == taskcfg::kRangeOrder) return fail(MPC_E_ARG, "mpc_task_create: command range with min > max");
  if (!(cfg->clip_observations > 0.0)) return fail(MPC_E_ARG, "mpc_task_create: clip_observations must be positive");
  if (bad == taskcfg::kEpisodeLength) return fail(MPC_E_ARG, "mpc_task_create: max_episode_length must be at least 1");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_task_create: no HIP device");
  mpc_task *t = new mpc_task();
  t->n = n;
  t->device = device;
  t->c = taskcfg::to_device_config(*cfg);
  hipError_t e;
  if ((e = t->d_episode.alloc_zero((size_t)n)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
    mpc_task_destroy(t);
    return fail(MPC_E_HIP, std::string("mpc_task_create: ") + hipGetErrorString(e));
  }
  *out = t;
  return MPC_OK;
}

int mpc_task_buffers(mpc_task *t, const mpc_task_buffer_set *b) {
  if (!t || !b || !b->d_progress || !b->d_reset || !b->d_timeout || !b->d_reset_ids || !b->d_commands || !b->d_obs || !b->d_rew)
    return fail(MPC_E_ARG, "mpc_task_buffers: bad argument (all seven buffers are required)");
  t->b = *b;
  t->bound = true;
  return MPC_OK;
}

int mpc_task_begin(mpc_task *t, void *stream) {
  if (!t) return fail(MPC_E_ARG, "mpc_task_begin: bad argument");
  if (!t->bound) return fail(MPC_E_ARG, "mpc_task_begin: no buffers bound (mpc_task_buffers)");
  DeviceGuard guard_(t->device);
  hipLaunchKernelGGL(task_begin_kernel, task_grid(t->n), dim3(kTaskThreads), 0, reinterpret_cast<hipStream_t>(stream), t->c, t->n, t->b.d_progress,
                     t->b.d_reset, t->b.d_timeout, t->d_episode, t->b.d_reset_ids, t->b.d_commands);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_task_finish(mpc_task *t, const float *d_root, const float *d_dof, const float *d_actions, const float *d_torques,
                    const float *d_contact_forces, int bodies, int base_index, const int *knee_indices, const int *hip_indices,
                    const unsigned char *d_fell, void *stream) {
  if (!t || !d_root || !d_dof || !d_actions || !d_torques) return fail(MPC_E_ARG, "mpc_task_finish: bad argument");
  if (!t->bound) return fail(MPC_E_ARG, "mpc_task_finish: no buffers bound (mpc_task_buffers)");
  ContactArgs k{};
  k.forces = d_contact_forces;
  k.fell = d_fell;
  if (d_contact_forces) {
    if (bodies <= 0 || !knee_indices || !hip_indices || base_index < 0 || base_index >= bodies)
      return fail(MPC_E_ARG, "mpc_task_finish: contact forces need bodies > 0, a base index below it and the knee and hip indices");
    k.bodies = bodies;
    k.base = base_index;
    for (int l = 0; l < kLegs; ++l) {
      if (knee_indices[l] < 0 || knee_indices[l] >= bodies || hip_indices[l] < 0 || hip_indices[l] >= bodies)
        return fail(MPC_E_ARG, "mpc_task_finish: knee or hip index outside [0, bodies)");
      k.knee[l] = knee_indices[l];
      k.hip[l] = hip_indices[l];
    }
  }
  DeviceGuard guard_(t->device);
  hipLaunchKernelGGL(task_finish_kernel, task_grid(t->n), dim3(kTaskThreads), 0, reinterpret_cast<hipStream_t>(stream), t->c, t->n, d_root, d_dof,
                     (const float *)t->b.d_commands, d_actions, d_torques, k, (const long long *)t->b.d_progress, t->b.d_obs, t->b.d_rew, t->b.d_reset);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
