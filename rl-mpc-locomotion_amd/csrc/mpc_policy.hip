// mpc_policy.hip -- the weight policy of include/mpc_batch.h (RL_Environment/WeightPolicy.py): mpc_policy_*, its observation rows and the packing
// of the controller's command rows (mpc_pack_commands*).  The layers are policy_mlp.h's.  Errors land in mpc_batch.hip's slot (mpc_last_error).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpc_batch.h"
#include "mpc_batch_internal.h"
#include "policy_mlp.h"

using mpchost::DeviceArray;

struct mpc_policy {
  int device = 0;
  policy::Net net{};
  DeviceArray<float> d_params; // all weights and biases, one allocation
  size_t lds = 0;
};

namespace {

int fail(int code, const std::string &msg) { return batchint::set_error(code, msg); }      // (mpc_batch.hip's slot: one mpc_last_error for the three units)

// obs [n, dims[0]] -> actions [n, dims[L]] (may be null) and weights [n, dims[L]] = clamp(a, -1, 1) * scale + shift
__global__ __launch_bounds__(policy::kThreads) void mlp_kernel(policy::Net net, int n, const float *__restrict__ obs, float *__restrict__ actions,
                                                              float *__restrict__ weights) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int wmax_even = 0, wmax_odd = 0;   // widest activation held by buffer 0 (layers 0, 2, ...) / buffer 1
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
  for (int l = 0; l < net.n_layers; ++l) {
    policy::layer(buf[l & 1], stride[l & 1], buf[(l + 1) & 1], stride[(l + 1) & 1], net.w[l], net.b[l], net.dims[l], net.dims[l + 1], l + 1 < net.n_layers);
    __syncthreads();
  }
  const int L = net.n_layers, dl = net.dims[L];
  const float *res = buf[L & 1];
  for (int e = threadIdx.x; e < policy::kRows * dl; e += policy::kThreads) {
    const int r = e / dl, k = e - r * dl;
    if (r0 + r >= n) continue;
    const float a = res[r * stride[L & 1] + k];
    if (actions) actions[(size_t)(r0 + r) * dl + k] = a;
    const float c = fminf(fmaxf(a, -1.f), 1.f);          // torch.clamp(current_action, -1, 1); _rescale_actions(-1, 1, .) is the identity
    weights[(size_t)(r0 + r) * dl + k] = c * net.scale[k] + net.shift[k];
  }
}
mpchost::LdsLimit g_mlp_limit(mlp_kernel);

// WeightPolicy.compute_observations (:120-139): [vBody * lin, omegaBody * ang, -ground_normal_yaw, commands * (lin, lin, ang),
// dof_pos * dps, dof_vel * dvs, previous actions]  (48 floats).  est = [vBody3, omegaBody3, rpy3, R9] as written by the
// estimator kernel; dof = [12][2] (pos, vel); scales = {lin, ang, dof_pos, dof_vel}.
// normal: ground_normal_yaw of robot r at normal[r * normal_stride + 0 .. 2] (3: a packed [n, 3] array; sizeof(CtrlState) / 4: the controller's own state records)
__global__ void observations_kernel(int n, const float *__restrict__ dof, const float *__restrict__ est, const float *__restrict__ normal, int normal_stride,
                                    const float *__restrict__ cmd3, const float *__restrict__ prev, float lin, float ang, float dps, float dvs,
                                    float *__restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 48) return;
  const int r = i / 48, k = i - 48 * r;
  float v;
  if (k < 3) v = est[18 * r + k] * lin;
  else if (k < 6) v = est[18 * r + k] * ang;
  else if (k < 9) v = -normal[(size_t)normal_stride * r + k - 6];
  else if (k < 12) v = cmd3[3 * r + k - 9] * (k < 11 ? lin : ang);
  else if (k < 24) v = dof[24 * r + 2 * (k - 12)] * dps;
  else if (k < 36) v = dof[24 * r + 2 * (k - 24) + 1] * dvs;
  else v = prev[12 * r + k - 36];
  obs[i] = v;
}

// commands of controller.run: np.concatenate((commands[idx], actions_rescale[idx], [0.0])) (RL_Environment/tasks/aliengo.py:251)
__global__ void pack_commands_kernel(int n, const float *__restrict__ cmd3, const float *__restrict__ w12, float *__restrict__ cmd16) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 16) return;
  const int r = i / 16, k = i - 16 * r;
  cmd16[i] = k < 3 ? cmd3[3 * r + k] : k < 15 ? w12[12 * r + k - 3] : 0.f;
}

// ... with the rescale of VecTask.pre_physics_step in front of it: actions_rescale = torch.mul(actions, MPC_param_scale).add(MPC_param_const)
// (RL_Environment/tasks/aliengo.py:237-245) -- a float32 product, then a float32 sum, like torch's two kernels (no fused multiply-add)
struct Rescale { float scale[12], shift[12]; };
__global__ void pack_commands_scaled_kernel(int n, const float *__restrict__ cmd3, const float *__restrict__ act12, Rescale rs, float *__restrict__ cmd16) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 16) return;
  const int r = i / 16, k = i - 16 * r;
  float v = 0.f;
  if (k < 3) v = cmd3[3 * r + k];
  else if (k < 15) v = __fadd_rn(__fmul_rn(act12[12 * r + k - 3], rs.scale[k - 3]), rs.shift[k - 3]);
  cmd16[i] = v;
}
}  // namespace

hipError_t batchint::launch_observations(int n, const float *d_dof, const float *d_est, const float *d_normal, int normal_stride, const float *d_cmd3,
                                         const float *d_prev_actions, const float *scales4, float *d_obs, hipStream_t stream) {
  hipLaunchKernelGGL(observations_kernel, dim3((n * 48 + 255) / 256), dim3(256), 0, stream, n, d_dof, d_est, d_normal, normal_stride, d_cmd3, d_prev_actions, scales4[0],
                     scales4[1], scales4[2], scales4[3], d_obs);
  return hipGetLastError();
}

extern "C" {

void mpc_policy_destroy(mpc_policy *p) { mpchost::destroy_handle(p); }

int mpc_policy_create(mpc_policy **out, int n_layers, const int *dims, const float *const *weights, const float *const *biases,
                      const float *act_scale, const float *act_const) {
  if (!out || n_layers <= 0 || n_layers > policy::kMaxLayers || !dims || !weights || !biases || !act_scale || !act_const)
    return fail(MPC_E_ARG, "mpc_policy_create: bad argument");
  size_t total = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (dims[l] <= 0 || dims[l + 1] <= 0 || dims[l] % 16 != 0 || !weights[l] || !biases[l])
      return fail(MPC_E_ARG, "mpc_policy_create: layer input widths must be positive multiples of 16");
    total += (size_t)dims[l] * dims[l + 1] + (((size_t)dims[l + 1] + 7) / 8) * 8;   // keeps every array 32-byte aligned
  }
  if (dims[n_layers] > 16) return fail(MPC_E_ARG, "mpc_policy_create: at most 16 outputs");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_policy_create: no HIP device");
  mpc_policy *p = new mpc_policy();
  p->device = device;
  p->net.n_layers = n_layers;
  for (int l = 0; l <= n_layers; ++l) p->net.dims[l] = dims[l];
  std::vector<float> host(total, 0.f);
  if (p->d_params.alloc(total) != hipSuccess) { delete p; return fail(MPC_E_HIP, "mpc_policy_create: hipMalloc"); }
  size_t off = 0;
  for (int l = 0; l < n_layers; ++l) {
    const size_t nw = (size_t)dims[l] * dims[l + 1], nb = (((size_t)dims[l + 1] + 7) / 8) * 8;
    std::memcpy(host.data() + off, weights[l], sizeof(float) * nw);
    p->net.w[l] = p->d_params + off; off += nw;
    std::memcpy(host.data() + off, biases[l], sizeof(float) * dims[l + 1]);
    p->net.b[l] = p->d_params + off; off += nb;
  }
  for (int k = 0; k < dims[n_layers]; ++k) { p->net.scale[k] = act_scale[k]; p->net.shift[k] = act_const[k]; }
  p->lds = policy::lds_bytes(p->net);
  if (p->lds > 160 * 1024) { mpc_policy_destroy(p); return fail(MPC_E_ARG, "mpc_policy_create: layers too wide for one CU's LDS"); }
  if (hipMemcpy(p->d_params, host.data(), sizeof(float) * total, hipMemcpyHostToDevice) != hipSuccess ||
      g_mlp_limit.raise(device, p->lds) != hipSuccess) {
    mpc_policy_destroy(p);
    return fail(MPC_E_HIP, "mpc_policy_create: device set-up failed");
  }
  *out = p;
  return MPC_OK;
}

int mpc_policy_step(mpc_policy *p, int n, const float *d_obs, float *d_actions, float *d_weights, void *stream) {
  if (!p || n <= 0 || !d_obs || !d_weights) return fail(MPC_E_ARG, "mpc_policy_step: bad argument");
  const int blocks = (n + policy::kRows - 1) / policy::kRows;
  hipLaunchKernelGGL(mlp_kernel, dim3(blocks), dim3(policy::kThreads), p->lds, (hipStream_t)stream, p->net, n, d_obs, d_actions, d_weights);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_policy_observations(int n, const float *d_dof, const float *d_est, const float *d_normal, const float *d_cmd3,
                            const float *d_prev_actions, const float *scales4, float *d_obs, void *stream) {
  if (n <= 0 || !d_dof || !d_est || !d_normal || !d_cmd3 || !d_prev_actions || !scales4 || !d_obs)
    return fail(MPC_E_ARG, "mpc_policy_observations: bad argument");
  HIP_TRY(batchint::launch_observations(n, d_dof, d_est, d_normal, 3, d_cmd3, d_prev_actions, scales4, d_obs, (hipStream_t)stream));
  return MPC_OK;
}

int mpc_pack_commands_scaled(int n, const float *d_cmd3, const float *d_actions12, const float *scale12, const float *const12, float *d_cmd16, void *stream) {
  if (n <= 0 || !d_cmd3 || !d_actions12 || !scale12 || !const12 || !d_cmd16) return fail(MPC_E_ARG, "mpc_pack_commands_scaled: bad argument");
  Rescale rs;
  for (int k = 0; k < 12; ++k) { rs.scale[k] = scale12[k]; rs.shift[k] = const12[k]; }
  hipLaunchKernelGGL(pack_commands_scaled_kernel, dim3((n * 16 + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_cmd3, d_actions12, rs, d_cmd16);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_pack_commands(int n, const float *d_cmd3, const float *d_weights12, float *d_cmd16, void *stream) {
  if (n <= 0 || !d_cmd3 || !d_weights12 || !d_cmd16) return fail(MPC_E_ARG, "mpc_pack_commands: bad argument");
  hipLaunchKernelGGL(pack_commands_kernel, dim3((n * 16 + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_cmd3, d_weights12, d_cmd16);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
