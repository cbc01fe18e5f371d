// mpc_recurrent_policy.hip -- the C ABI of mpc_recurrent_policy.h: a deployed recurrent weight policy's tick on the device.
//   step_kernel        grid ceil(n / 16), policy::kThreads threads.  A workgroup stages the x and h rows of 16 robots in LDS (the reset applied to h
//                      there), runs the actor's LSTM cell on the fp32 MFMA pipe and finishes it in registers, leaves h' in LDS for the actor's
//                      layers (policy::layer, as mlp_kernel runs them) and writes the raw actions and the MPC weights (recurrent_policy.h).
//                      The parameters are the handle's own device copy.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mpc_host.h"
#include "mpc_recurrent_policy.h"
#include "recurrent_host.h"
#include "recurrent_policy.h"

using mpchost::aligned16;
using mpchost::DeviceArray;
using mpchost::DeviceGuard;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

size_t padded8(size_t count) { return (count + 7) / 8 * 8; }      // keeps every array of the one allocation 32-byte aligned

mpchost::LdsLimit g_step_limit(recurrent_policy::step_kernel);
}  // namespace

struct mpc_recurrent_policy {
  int device = -1;
  recurrent_policy::Launch launch{};
  DeviceArray<float> d_params;         // the memory's four arrays, then every layer's weight and bias: one allocation
  size_t lds = 0;
};

extern "C" {

const char *mpc_recurrent_policy_last_error(void) { return g_err.c_str(); }

void mpc_recurrent_policy_destroy(mpc_recurrent_policy *p) { mpchost::destroy_handle(p); }

int mpc_recurrent_policy_create(mpc_recurrent_policy **out, int I, int H, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int n_layers,
                                const int *dims, const float *const *weights, const float *const *biases, const float *act_scale, const float *act_const) {
  const std::string who = "mpc_recurrent_policy_create: ";
  if (!out || !w_ih || !w_hh || !b_ih || !b_hh || !dims || !weights || !biases || !act_scale || !act_const) return fail(MPC_E_ARG, who + "null argument");
  const std::string why = recurrent::size_refusal(I, H);
  if (!why.empty()) return fail(MPC_E_ARG, who + why);
  if (n_layers < 1 || n_layers > policy::kMaxLayers)
    return fail(MPC_E_ARG, who + std::to_string(n_layers) + " layers: 1 .. " + std::to_string(policy::kMaxLayers) + " are built");
  if (dims[0] != H) return fail(MPC_E_ARG, who + "the actor's first layer reads dims[0] = " + std::to_string(dims[0]) + " inputs, the memory gives " + std::to_string(H));
  if (dims[n_layers] < 1 || dims[n_layers] > 16) return fail(MPC_E_ARG, who + std::to_string(dims[n_layers]) + " outputs: 1 .. 16 are built");
  for (int l = 1; l < n_layers; ++l)
    if (dims[l] <= 0 || dims[l] % 16 != 0)
      return fail(MPC_E_ARG, who + "the hidden width dims[" + std::to_string(l) + "] = " + std::to_string(dims[l]) + " is not a positive multiple of 16");
  for (int l = 0; l < n_layers; ++l)
    if (!weights[l] || !biases[l]) return fail(MPC_E_ARG, who + "layer " + std::to_string(l) + ": null weight or bias");
  policy::Net net{};
  net.n_layers = n_layers;
  for (int l = 0; l <= n_layers; ++l) net.dims[l] = dims[l];
  const size_t lds = recurrent_policy::lds_bytes(I, H, net);
  if (lds > (size_t)MPC_RECURRENT_POLICY_MAX_LDS)
    return fail(MPC_E_ARG, who + "16 rows of x, h and the actor's widest layers need " + std::to_string(lds) + " bytes of LDS, more than one CU's 160 KB");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, who + "no HIP device");

  // the one allocation: [w_ih | w_hh | b_ih | b_hh | W_0 | b_0 | ...], every count a multiple of 8 floats
  const size_t G = 4 * (size_t)H;
  size_t total = G * I + G * H + 2 * G;
  for (int l = 0; l < n_layers; ++l) total += (size_t)dims[l] * dims[l + 1] + padded8((size_t)dims[l + 1]);
  std::vector<float> host(total, 0.f);
  mpc_recurrent_policy *p = new mpc_recurrent_policy();
  p->device = device;
  p->lds = lds;
  if (p->d_params.alloc(total) != hipSuccess) { delete p; return fail(MPC_E_HIP, who + "hipMalloc"); }
  size_t off = 0;
  const auto put = [&](const float *src, size_t count, size_t room) {
    std::memcpy(host.data() + off, src, sizeof(float) * count);
    const float *at = p->d_params + off;
    off += room;
    return at;
  };
  recurrent::Cell &cell = p->launch.cell;
  cell.I = I;
  cell.H = H;
  cell.w_ih = put(w_ih, G * I, G * I);
  cell.w_hh = put(w_hh, G * H, G * H);
  cell.b_ih = put(b_ih, G, G);
  cell.b_hh = put(b_hh, G, G);
  for (int l = 0; l < n_layers; ++l) {
    const size_t nw = (size_t)dims[l] * dims[l + 1];
    net.w[l] = put(weights[l], nw, nw);
    net.b[l] = put(biases[l], (size_t)dims[l + 1], padded8((size_t)dims[l + 1]));
  }
  for (int k = 0; k < dims[n_layers]; ++k) { net.scale[k] = act_scale[k]; net.shift[k] = act_const[k]; }
  p->launch.net = net;
  if (hipMemcpy(p->d_params, host.data(), sizeof(float) * total, hipMemcpyHostToDevice) != hipSuccess ||
      g_step_limit.raise(device, p->lds) != hipSuccess) {
    mpc_recurrent_policy_destroy(p);
    return fail(MPC_E_HIP, who + "device set-up failed");
  }
  *out = p;
  return MPC_OK;
}

int mpc_recurrent_policy_step(mpc_recurrent_policy *p, int n, const float *d_obs, float *d_h, float *d_c, const long long *d_reset, float *d_actions, float *d_weights,
                              void *stream) {
  const std::string who = "mpc_recurrent_policy_step: ";
  if (!d_obs || !d_h || !d_c || !d_weights) return fail(MPC_E_ARG, who + "d_obs, d_h, d_c or d_weights is null");
  if (n < 1) return fail(MPC_E_ARG, who + "n must be at least 1");
  if (!aligned16(d_obs) || !aligned16(d_h) || !aligned16(d_c) || !aligned16(d_actions) || !aligned16(d_weights))
    return fail(MPC_E_ARG, who + "every float pointer must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_reset) & 7u) return fail(MPC_E_ARG, who + "d_reset must be 8-byte aligned");
  if (d_h == d_c) return fail(MPC_E_ARG, who + "d_h and d_c must not be the same array");
  if (!p) return fail(MPC_E_ARG, who + "null handle");
  DeviceGuard guard_(p->device);
  const dim3 grid((unsigned)((n + recurrent_policy::kRows - 1) / recurrent_policy::kRows));
  hipLaunchKernelGGL(recurrent_policy::step_kernel, grid, dim3(recurrent_policy::kThreads), p->lds, reinterpret_cast<hipStream_t>(stream), p->launch, n, d_obs, d_h,
                     d_c, d_reset, d_actions, d_weights);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
