// mpc_plant_rand.hip -- the C ABI of mpc_plant_rand.h: the opt-in per-robot plant randomisation (plant_rand.h) on the device, and the step
// kernels of a sim that carries a plant record.
//   plant_draw_kernel          one lane per slot of the id array, the plant's grid: a listed environment reads its draw counter, draws its
//                              record (plant_rand.h), writes the three doubles into the structure-of-arrays record and the counter back.
//   plant_step_plane_kernel    mpc_sim.hip's sim_step_kernel and mpc_terrain.hip's terrain_step_kernel with toy_step_plant in place of toy_step
//   plant_step_field_kernel    (sim_step.h's shell with its PlantRecord model): each lane loads its three doubles (one word per lane per entry,
//                              consecutive lanes on consecutive words) and steps with mass + payload, its twelve widened torques times strength,
//                              and its own gravity.
// No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "mpc_host.h"
#include "mpc_plant_rand.h"
#include "mpc_sim_internal.h"
#include "plant_rand.h"
#include "toy_sim.h"

using namespace simstep;               // (and with it toysim)
using mpchost::DeviceGuard;
using simint::kSimThreads;
using simint::sim_grid;

static_assert(MPC_PLANT_AXES == kPlant && MPC_PLANT_PAYLOAD == kPlantPayload && MPC_PLANT_STRENGTH == kPlantStrength && MPC_PLANT_GRAVITY == kPlantGravZ,
              "mpc_plant_rand.h and toy_sim.h disagree");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

__global__ __launch_bounds__(kSimThreads) void plant_draw_kernel(int n, int k, const int *__restrict__ ids, plantrand::Ranges rg, unsigned long long seed,
                                                                 unsigned *counter, double *plant) {
  const int i = (int)(blockIdx.x * kSimThreads + threadIdx.x);
  if (i >= k) return;
  const int r = ids ? ids[i] : i;
  if (r < 0 || r >= n) return;
  const unsigned e = counter[r];
  double rec[kPlant];
  plantrand::draw_record(seed, (uint32_t)r, e, rg, rec);
#pragma unroll
  for (int j = 0; j < kPlant; ++j) plant[(size_t)j * (size_t)n + r] = rec[j];
  counter[r] = e + 1u;
}

__global__ __launch_bounds__(kSimThreads) void plant_step_plane_kernel(Args a, PlantRecord m, PlaneSource g, const float *__restrict__ tau, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) step_robot(a, r, g, m, tau, dof, root);
}

__global__ __launch_bounds__(kSimThreads) void plant_step_field_kernel(Args a, PlantRecord m, FieldSource f, const float *__restrict__ tau, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) step_robot(a, r, f, m, tau, dof, root);
}
}  // namespace

namespace simint {

hipError_t plant_launch_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, hipStream_t stream) {
  const PlantRecord m{s->d_plant};
  if (s->d_heights) hipLaunchKernelGGL(plant_step_field_kernel, sim_grid(s->n), dim3(kSimThreads), 0, stream, step_args(s), m, field_source(s), d_tau, d_dof, d_root);
  else hipLaunchKernelGGL(plant_step_plane_kernel, sim_grid(s->n), dim3(kSimThreads), 0, stream, step_args(s), m, plane_source(s), d_tau, d_dof, d_root);
  return hipGetLastError();
}

}  // namespace simint

struct mpc_plant_rand {
  int n = 0, device = 0;
  unsigned long long seed = 0;
  double *d_plant = nullptr;                   // the attached sim's record (the sim owns it; null until mpc_plant_rand_attach)
  mpchost::DeviceArray<unsigned> d_counter;    // [n] draws made so far
};

extern "C" {

const char *mpc_plant_rand_last_error(void) { return g_err.c_str(); }

void mpc_plant_rand_destroy(mpc_plant_rand *h) { mpchost::destroy_handle(h); }

int mpc_plant_rand_create(mpc_plant_rand **out, int n, unsigned long long seed) {
  if (!out) return fail(MPC_E_ARG, "mpc_plant_rand_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_plant_rand_create: n must be at least 1");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_plant_rand_create: no HIP device");
  mpc_plant_rand *h = new mpc_plant_rand();
  h->n = n;
  h->seed = seed;
  h->device = device;
  *out = h;
  return MPC_OK;
}

int mpc_plant_rand_attach(mpc_plant_rand *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_plant_rand_attach: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_plant_rand_attach: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_plant_rand_attach: the sim has " + std::to_string(s->n) + " robots, the randomisation " + std::to_string(h->n) + " environments");
  if (s->device != h->device) return fail(MPC_E_ARG, "mpc_plant_rand_attach: the sim lives on another device");
  if (h->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_attach: the randomisation is attached to a sim already");
  if (s->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_attach: the sim has a plant record already");
  const size_t n = (size_t)h->n;
  std::vector<double> rec(kPlant * n);
  for (int j = 0; j < kPlant; ++j)
    for (size_t r = 0; r < n; ++r) rec[j * n + r] = plantrand::neutral(j);
  DeviceGuard guard_(h->device);
  // both arrays are built first: a failed attach leaves the sim without a record (the temporaries free what they hold)
  mpchost::DeviceArray<double> d_rec;
  mpchost::DeviceArray<unsigned> d_cnt;
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess || (e = d_rec.alloc_copy(rec.data(), rec.size())) != hipSuccess || (e = d_cnt.alloc_zero(n)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess)
    return fail(MPC_E_HIP, std::string("mpc_plant_rand_attach: ") + hipGetErrorString(e));
  s->d_plant = std::move(d_rec);
  h->d_counter = std::move(d_cnt);
  h->d_plant = s->d_plant;
  return MPC_OK;
}

int mpc_plant_rand_draw(mpc_plant_rand *h, const int *d_ids, int k, const int *present, const double *ranges, void *stream) {
  // the ranges first: they can be refused without a handle
  if (!present || !ranges) return fail(MPC_E_ARG, "mpc_plant_rand_draw: null argument");
  if (k < 0) return fail(MPC_E_ARG, "mpc_plant_rand_draw: negative id count");
  static const char *const names[kPlant] = {"payload", "strength", "gravity"};
  plantrand::Ranges rg{};
  for (int a = 0; a < kPlant; ++a) {
    rg.present[a] = present[a] != 0;
    if (!rg.present[a]) continue;
    rg.lo[a] = (float)ranges[2 * a];
    rg.hi[a] = (float)ranges[2 * a + 1];
    if (!std::isfinite(rg.lo[a]) || !std::isfinite(rg.hi[a])) return fail(MPC_E_ARG, std::string("mpc_plant_rand_draw: ") + names[a] + " range must be finite as float32");
    if (rg.lo[a] > rg.hi[a]) return fail(MPC_E_ARG, std::string("mpc_plant_rand_draw: ") + names[a] + " range with lo > hi");
  }
  if (rg.present[kPlantStrength] && rg.lo[kPlantStrength] < 0.0f) return fail(MPC_E_ARG, "mpc_plant_rand_draw: strength lo must be >= 0");
  if (!h) return fail(MPC_E_ARG, "mpc_plant_rand_draw: null handle");
  if (!d_ids && k != h->n) return fail(MPC_E_ARG, "mpc_plant_rand_draw: without ids k must be n (all environments)");
  if (!h->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_draw: no sim attached (mpc_plant_rand_attach)");
  if (k == 0) return MPC_OK;
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(plant_draw_kernel, sim_grid(k), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), h->n, k, d_ids, rg, h->seed,
                     (unsigned *)h->d_counter, h->d_plant);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_plant_rand_get_params(mpc_plant_rand *h, double *h_params) {
  if (!h || !h_params) return fail(MPC_E_ARG, "mpc_plant_rand_get_params: null argument");
  if (!h->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_get_params: no sim attached (mpc_plant_rand_attach)");
  DeviceGuard guard_(h->device);
  const size_t n = (size_t)h->n;
  std::vector<double> rec(kPlant * n);
  HIP_TRY(mpchost::sync_copy(rec.data(), h->d_plant, rec.size(), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < n; ++r)
    for (int j = 0; j < kPlant; ++j) h_params[r * kPlant + j] = rec[j * n + r];
  return MPC_OK;
}

int mpc_plant_rand_set_params(mpc_plant_rand *h, const double *h_params, const double *h_mass) {
  if (!h || !h_params) return fail(MPC_E_ARG, "mpc_plant_rand_set_params: null argument");
  const size_t n = (size_t)h->n;
  for (size_t r = 0; r < n; ++r) {
    const double *p = h_params + r * kPlant;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
      return fail(MPC_E_ARG, "mpc_plant_rand_set_params: the record of robot " + std::to_string(r) + " is not finite");
    if (p[kPlantStrength] < 0.0) return fail(MPC_E_ARG, "mpc_plant_rand_set_params: the strength of robot " + std::to_string(r) + " is negative");
    if (h_mass && !(h_mass[r] + p[kPlantPayload] > 0.0))
      return fail(MPC_E_ARG, "mpc_plant_rand_set_params: the payload of robot " + std::to_string(r) + " leaves no positive mass");
  }
  if (!h->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_set_params: no sim attached (mpc_plant_rand_attach)");
  DeviceGuard guard_(h->device);
  std::vector<double> rec(kPlant * n);
  for (size_t r = 0; r < n; ++r)
    for (int j = 0; j < kPlant; ++j) rec[j * n + r] = h_params[r * kPlant + j];
  HIP_TRY(mpchost::sync_copy(h->d_plant, rec.data(), rec.size(), hipMemcpyHostToDevice));
  return MPC_OK;
}

int mpc_plant_rand_get_counters(mpc_plant_rand *h, unsigned int *h_counters) {
  if (!h || !h_counters) return fail(MPC_E_ARG, "mpc_plant_rand_get_counters: null argument");
  if (!h->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_get_counters: no sim attached (mpc_plant_rand_attach)");
  DeviceGuard guard_(h->device);
  HIP_TRY(mpchost::sync_copy(h_counters, h->d_counter.get(), (size_t)h->n, hipMemcpyDeviceToHost));
  return MPC_OK;
}

int mpc_plant_rand_set_counters(mpc_plant_rand *h, const unsigned int *h_counters) {
  if (!h || !h_counters) return fail(MPC_E_ARG, "mpc_plant_rand_set_counters: null argument");
  if (!h->d_plant) return fail(MPC_E_ARG, "mpc_plant_rand_set_counters: no sim attached (mpc_plant_rand_attach)");
  DeviceGuard guard_(h->device);
  HIP_TRY(mpchost::sync_copy(h->d_counter.get(), h_counters, (size_t)h->n, hipMemcpyHostToDevice));
  return MPC_OK;
}

}  // extern "C"
