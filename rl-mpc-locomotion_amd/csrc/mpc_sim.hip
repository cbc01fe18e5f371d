// mpc_sim.hip -- the C ABI of include/mpc_sim.h: the batched toy plant (toy_sim.h) on the device, one lane per robot.
// The state is structure-of-arrays in HBM (entry j of robot r at [j * n + r]: the lanes of a wave load and store consecutive words); a tick
// loads a robot's 49 doubles and 9 ints into registers, runs toy_step and writes the state back and the float32 observation out.  That shell is
// sim_step.h's, shared with the other units' step kernels; the kernels here are its plane ground and nominal plant.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mpc_sim.h"
#include "mpc_host.h"
#include "mpc_sim_internal.h"
#include "toy_sim.h"

using namespace simstep;               // (and with it toysim)
using mpchost::DeviceGuard;
using simint::kSimThreads;
using simint::plane_source;
using simint::sim_grid;
using simint::step_args;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

// (re)initialise robots ids[0 .. k) (all n when ids is null)
__global__ __launch_bounds__(kSimThreads) void sim_init_kernel(Args a, PlaneSource g, const double *yaw0, const int *ids, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) init_robot(a, i, ids, g, yaw0);
}

__global__ __launch_bounds__(kSimThreads) void sim_step_kernel(Args a, PlaneSource g, const float *__restrict__ tau, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) step_robot(a, r, g, Nominal{}, tau, dof, root);
}

__global__ __launch_bounds__(kSimThreads) void sim_observe_kernel(Args a, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  State s;
  unpack(s, a.f64 + r, a.i32 + r, a.n);
  write_obs(s, r, dof, root);
}

__global__ __launch_bounds__(kSimThreads) void sim_flags_kernel(int n, const int *i32, unsigned char *contact, unsigned char *fell) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (contact) {
#pragma unroll
    for (int l = 0; l < 4; ++l) contact[(size_t)r * 4 + l] = i32[(size_t)l * n + r] != 0;
  }
  if (fell) fell[r] = i32[(size_t)8 * n + r] != 0;
}
}  // namespace

// (struct mpc_sim and the builders of the launch arguments: mpc_sim_internal.h)

extern "C" {

const char *mpc_sim_last_error(void) { return g_err.c_str(); }

void mpc_sim_destroy(mpc_sim *s) { mpchost::destroy_handle(s); }

int mpc_sim_create(mpc_sim **out, int n, const int *robot_type, int n_types, const double *table, const double *slope, const double *yaw0, double dt) {
  if (!out || n <= 0 || !robot_type || n_types <= 0 || !table || !(dt > 0.0)) return fail(MPC_E_ARG, "mpc_sim_create: bad argument");
  for (int r = 0; r < n; ++r)
    if (robot_type[r] < 0 || robot_type[r] >= n_types) return fail(MPC_E_ARG, "mpc_sim_create: robot_type out of range");
  std::vector<Params> params(n_types);
  for (int t = 0; t < n_types; ++t) {
    const double *row = table + (size_t)kRobotCols * t;
    if (!(row[kColMass] > 0.0) || !(row[kColInertia] > 0.0) || !(row[kColInertia + 1] > 0.0) || !(row[kColInertia + 2] > 0.0))
      return fail(MPC_E_ARG, "mpc_sim_create: robot table row with a non-positive mass or inertia");
    params_from_row(params[t], row);
  }
  std::vector<double> sl(2 * (size_t)n, 0.0), yaw(n, 0.0);
  if (slope) for (size_t i = 0; i < sl.size(); ++i) sl[i] = slope[i];
  if (yaw0) for (int r = 0; r < n; ++r) yaw[r] = yaw0[r];
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_sim_create: no HIP device");
  mpc_sim *s = new mpc_sim();
  s->n = n;
  s->device = device;
  s->dt = dt;
  hipError_t e;
  if ((e = s->d_f64.alloc(kF64 * (size_t)n)) != hipSuccess || (e = s->d_i32.alloc(kI32 * (size_t)n)) != hipSuccess ||
      (e = s->d_type.alloc_copy(robot_type, (size_t)n)) != hipSuccess || (e = s->d_slope.alloc_copy(sl.data(), sl.size())) != hipSuccess ||
      (e = s->d_yaw.alloc_copy(yaw.data(), (size_t)n)) != hipSuccess || (e = s->d_params.alloc_copy(params.data(), (size_t)n_types)) != hipSuccess) {
    mpc_sim_destroy(s);
    return fail(MPC_E_HIP, std::string("mpc_sim_create: ") + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(sim_init_kernel, sim_grid(n), dim3(kSimThreads), 0, nullptr, step_args(s), plane_source(s), (const double *)s->d_yaw, (const int *)nullptr, n);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
    mpc_sim_destroy(s);
    return fail(MPC_E_HIP, std::string("mpc_sim_create: ") + hipGetErrorString(e));
  }
  *out = s;
  return MPC_OK;
}

int mpc_sim_size(mpc_sim *s) { return s ? s->n : 0; }

int mpc_sim_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, void *stream) {
  if (!s || !d_tau) return fail(MPC_E_ARG, "mpc_sim_step: bad argument");
  DeviceGuard guard_(s->device);
  if (s->friction) {                   // a friction record is attached (mpc_friction_attach): the Coulomb instantiation of its ground
    HIP_TRY(simint::friction_launch_step(s, d_tau, d_dof, d_root, reinterpret_cast<hipStream_t>(stream)));
    return MPC_OK;
  }
  if (s->d_plant) {                    // a plant record is attached (mpc_plant_rand_attach): the parametrised instantiation of its ground
    HIP_TRY(simint::plant_launch_step(s, d_tau, d_dof, d_root, reinterpret_cast<hipStream_t>(stream)));
    return MPC_OK;
  }
  if (s->d_heights) {                  // a terrain is attached (mpc_terrain_attach): the height-field instantiation
    HIP_TRY(simint::terrain_launch_step(s, d_tau, d_dof, d_root, reinterpret_cast<hipStream_t>(stream)));
    return MPC_OK;
  }
  hipLaunchKernelGGL(sim_step_kernel, sim_grid(s->n), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), step_args(s), plane_source(s), d_tau, d_dof, d_root);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_sim_observe(mpc_sim *s, float *d_dof, float *d_root, void *stream) {
  if (!s || (!d_dof && !d_root)) return fail(MPC_E_ARG, "mpc_sim_observe: bad argument");
  DeviceGuard guard_(s->device);
  hipLaunchKernelGGL(sim_observe_kernel, sim_grid(s->n), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), step_args(s), d_dof, d_root);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_sim_reset_device(mpc_sim *s, const int *d_ids, int k, void *stream) {
  if (!s || !d_ids || k < 0) return fail(MPC_E_ARG, "mpc_sim_reset_device: bad argument");
  if (k == 0) return MPC_OK;
  DeviceGuard guard_(s->device);
  if (s->d_heights) {
    HIP_TRY(simint::terrain_launch_init(s, d_ids, k, reinterpret_cast<hipStream_t>(stream)));
    return MPC_OK;
  }
  hipLaunchKernelGGL(sim_init_kernel, sim_grid(k), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), step_args(s), plane_source(s), (const double *)s->d_yaw, d_ids, k);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_sim_get_state(mpc_sim *s, double *h_f64, int *h_i32) {
  if (!s || !h_f64 || !h_i32) return fail(MPC_E_ARG, "mpc_sim_get_state: bad argument");
  DeviceGuard guard_(s->device);
  const size_t n = (size_t)s->n;
  std::vector<double> f(kF64 * n);
  std::vector<int> k(kI32 * n);
  HIP_TRY(mpchost::sync_copy(f.data(), s->d_f64.get(), f.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(k.data(), s->d_i32, sizeof(int) * k.size(), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < n; ++r) {
    for (int j = 0; j < kF64; ++j) h_f64[r * kF64 + j] = f[j * n + r];
    for (int j = 0; j < kI32; ++j) h_i32[r * kI32 + j] = k[j * n + r];
  }
  return MPC_OK;
}

int mpc_sim_set_state(mpc_sim *s, const double *h_f64, const int *h_i32) {
  if (!s || !h_f64 || !h_i32) return fail(MPC_E_ARG, "mpc_sim_set_state: bad argument");
  DeviceGuard guard_(s->device);
  const size_t n = (size_t)s->n;
  std::vector<double> f(kF64 * n);
  std::vector<int> k(kI32 * n);
  for (size_t r = 0; r < n; ++r) {
    for (int j = 0; j < kF64; ++j) f[j * n + r] = h_f64[r * kF64 + j];
    for (int j = 0; j < kI32; ++j) k[j * n + r] = h_i32[r * kI32 + j];
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(s->d_f64, f.data(), sizeof(double) * f.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->d_i32, k.data(), sizeof(int) * k.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return MPC_OK;
}

int mpc_sim_flags(mpc_sim *s, unsigned char *d_contact, unsigned char *d_fell, void *stream) {
  if (!s || (!d_contact && !d_fell)) return fail(MPC_E_ARG, "mpc_sim_flags: bad argument");
  DeviceGuard guard_(s->device);
  hipLaunchKernelGGL(sim_flags_kernel, sim_grid(s->n), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), s->n, s->d_i32, d_contact, d_fell);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
