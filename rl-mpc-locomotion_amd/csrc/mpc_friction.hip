// mpc_friction.hip -- the C ABI of mpc_friction.h: the opt-in Coulomb friction of the toy plant on the device.
//   friction_draw_kernel        one lane per slot of the id array, the plant's grid: a listed environment has its force and slip rows zeroed
//                               and, where the draw resamples, reads its draw counter, draws its coefficient (friction.h) and writes both back.
//   friction_step_plane_kernel  mpc_plant_rand.hip's step kernels with toy_step_friction in place of toy_step_plant (sim_step.h's shell with its
//   friction_step_field_kernel  CoulombModel): each lane loads its coefficient and, where the sim has a plant record, its three doubles (the
//                               neutral constants where not: a branch that is uniform over the launch), steps, and writes its twelve force
//                               and four slip floats (zeros for a fallen robot).
// No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "friction.h"
#include "mpc_friction.h"
#include "mpc_host.h"
#include "mpc_sim_internal.h"
#include "toy_sim.h"

using namespace simstep;               // (and with it toysim)
using mpchost::DeviceGuard;
using simint::kSimThreads;
using simint::sim_grid;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

__global__ __launch_bounds__(kSimThreads) void friction_draw_kernel(int n, int k, const int *__restrict__ ids, float lo, float hi, int buckets, int resample,
                                                                    unsigned long long seed, unsigned *counter, double *mu, float *force, float *slip) {
  const int i = (int)(blockIdx.x * kSimThreads + threadIdx.x);
  if (i >= k) return;
  const int r = ids ? ids[i] : i;
  if (r < 0 || r >= n) return;
  if (force) {
#pragma unroll
    for (int j = 0; j < 12; ++j) force[(size_t)r * 12 + j] = 0.0f;
  }
  if (slip) {
#pragma unroll
    for (int j = 0; j < 4; ++j) slip[(size_t)r * 4 + j] = 0.0f;
  }
  if (!resample) return;
  const unsigned e = counter[r];
  mu[r] = (double)friction::draw_mu(seed, (uint32_t)r, e, lo, hi, buckets);
  counter[r] = e + 1u;
}

__global__ __launch_bounds__(kSimThreads) void friction_step_plane_kernel(Args a, CoulombModel m, PlaneSource g, const float *__restrict__ tau, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) step_robot(a, r, g, m, tau, dof, root);
}

__global__ __launch_bounds__(kSimThreads) void friction_step_field_kernel(Args a, CoulombModel m, FieldSource f, const float *__restrict__ tau, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) step_robot(a, r, f, m, tau, dof, root);
}

// the first entry of mu [n] that is negative or NaN, or -1
long bad_mu(const double *mu, size_t n) {
  for (size_t r = 0; r < n; ++r)
    if (!(mu[r] >= 0.0)) return (long)r;
  return -1;
}
}  // namespace

namespace simint {

hipError_t friction_launch_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, hipStream_t stream) {
  const CoulombModel m{s->d_plant, s->d_mu, s->d_force, s->d_slip};
  if (s->d_heights) hipLaunchKernelGGL(friction_step_field_kernel, sim_grid(s->n), dim3(kSimThreads), 0, stream, step_args(s), m, field_source(s), d_tau, d_dof, d_root);
  else hipLaunchKernelGGL(friction_step_plane_kernel, sim_grid(s->n), dim3(kSimThreads), 0, stream, step_args(s), m, plane_source(s), d_tau, d_dof, d_root);
  return hipGetLastError();
}

}  // namespace simint

struct mpc_friction {
  int n = 0, device = -1;                      // (the device is the bound sim's)
  unsigned long long seed = 0;
  mpc_sim *sim = nullptr;                      // the bound sim (null until mpc_friction_bind): it owns mu, its caller the force and slip rows
  mpchost::DeviceArray<unsigned> d_counter;    // [n] draws made so far
};

extern "C" {

const char *mpc_friction_last_error(void) { return g_err.c_str(); }

int mpc_friction_attach(mpc_sim *s, const double *h_mu, float *d_force, float *d_slip) {
  if (!s) return fail(MPC_E_ARG, "mpc_friction_attach: null sim handle");
  if (s->friction) return fail(MPC_E_ARG, "mpc_friction_attach: the sim has a friction record already");
  if (s->n < 1) return fail(MPC_E_ARG, "mpc_friction_attach: the sim holds no robots");
  const size_t n = (size_t)s->n;
  if (h_mu) {
    const long bad = bad_mu(h_mu, n);
    if (bad >= 0) return fail(MPC_E_ARG, "mpc_friction_attach: the mu of robot " + std::to_string(bad) + " is negative or NaN");
  }
  std::vector<double> mu(n, std::numeric_limits<double>::infinity());
  if (h_mu) mu.assign(h_mu, h_mu + n);
  DeviceGuard guard_(s->device);
  // built first: a failed attach leaves the sim without a record
  mpchost::DeviceArray<double> d_mu;
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess || (e = d_mu.alloc_copy(mu.data(), n)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
    return fail(MPC_E_HIP, std::string("mpc_friction_attach: ") + hipGetErrorString(e));
  s->d_mu = std::move(d_mu);
  s->d_force = d_force;
  s->d_slip = d_slip;
  s->friction = true;
  return MPC_OK;
}

void mpc_friction_destroy(mpc_friction *h) { mpchost::destroy_handle(h); }

int mpc_friction_create(mpc_friction **out, int n, unsigned long long seed) {
  if (!out) return fail(MPC_E_ARG, "mpc_friction_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_friction_create: n must be at least 1");
  mpc_friction *h = new mpc_friction();
  h->n = n;
  h->seed = seed;
  *out = h;
  return MPC_OK;
}

int mpc_friction_bind(mpc_friction *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_friction_bind: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_friction_bind: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_friction_bind: the sim has " + std::to_string(s->n) + " robots, the friction draw " + std::to_string(h->n) + " environments");
  if (h->sim) return fail(MPC_E_ARG, "mpc_friction_bind: the friction draw is bound to a sim already");
  if (!s->friction) return fail(MPC_E_ARG, "mpc_friction_bind: the sim has no friction record (mpc_friction_attach)");
  DeviceGuard guard_(s->device);
  mpchost::DeviceArray<unsigned> d_cnt;
  hipError_t e;
  if ((e = d_cnt.alloc_zero((size_t)h->n)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
    return fail(MPC_E_HIP, std::string("mpc_friction_bind: ") + hipGetErrorString(e));
  h->d_counter = std::move(d_cnt);
  h->device = s->device;
  h->sim = s;
  return MPC_OK;
}

int mpc_friction_draw(mpc_friction *h, const int *d_ids, int k, double lo, double hi, int buckets, int resample, void *stream) {
  // the range first: it can be refused without a handle
  const float flo = (float)lo, fhi = (float)hi;
  if (resample) {
    if (const char *why = friction::range_error(flo, fhi, buckets)) return fail(MPC_E_ARG, std::string("mpc_friction_draw: ") + why);
  }
  if (k < 0) return fail(MPC_E_ARG, "mpc_friction_draw: negative id count");
  if (!h) return fail(MPC_E_ARG, "mpc_friction_draw: null handle");
  if (!d_ids && k != h->n) return fail(MPC_E_ARG, "mpc_friction_draw: without ids k must be n (all environments)");
  if (!h->sim) return fail(MPC_E_ARG, "mpc_friction_draw: no sim bound (mpc_friction_bind)");
  if (k == 0) return MPC_OK;
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(friction_draw_kernel, sim_grid(k), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), h->n, k, d_ids, flo, fhi, buckets, resample,
                     h->seed, (unsigned *)h->d_counter, (double *)h->sim->d_mu, h->sim->d_force, h->sim->d_slip);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_friction_get_mu(mpc_friction *h, double *h_mu) {
  if (!h || !h_mu) return fail(MPC_E_ARG, "mpc_friction_get_mu: null argument");
  if (!h->sim) return fail(MPC_E_ARG, "mpc_friction_get_mu: no sim bound (mpc_friction_bind)");
  DeviceGuard guard_(h->device);
  HIP_TRY(mpchost::sync_copy(h_mu, h->sim->d_mu.get(), (size_t)h->n, hipMemcpyDeviceToHost));
  return MPC_OK;
}

int mpc_friction_set_mu(mpc_friction *h, const double *h_mu) {
  if (!h || !h_mu) return fail(MPC_E_ARG, "mpc_friction_set_mu: null argument");
  const long bad = bad_mu(h_mu, (size_t)h->n);
  if (bad >= 0) return fail(MPC_E_ARG, "mpc_friction_set_mu: the mu of robot " + std::to_string(bad) + " is negative or NaN");
  if (!h->sim) return fail(MPC_E_ARG, "mpc_friction_set_mu: no sim bound (mpc_friction_bind)");
  DeviceGuard guard_(h->device);
  HIP_TRY(mpchost::sync_copy(h->sim->d_mu.get(), h_mu, (size_t)h->n, hipMemcpyHostToDevice));
  return MPC_OK;
}

int mpc_friction_get_counters(mpc_friction *h, unsigned int *h_counters) {
  if (!h || !h_counters) return fail(MPC_E_ARG, "mpc_friction_get_counters: null argument");
  if (!h->sim) return fail(MPC_E_ARG, "mpc_friction_get_counters: no sim bound (mpc_friction_bind)");
  DeviceGuard guard_(h->device);
  HIP_TRY(mpchost::sync_copy(h_counters, h->d_counter.get(), (size_t)h->n, hipMemcpyDeviceToHost));
  return MPC_OK;
}

int mpc_friction_set_counters(mpc_friction *h, const unsigned int *h_counters) {
  if (!h || !h_counters) return fail(MPC_E_ARG, "mpc_friction_set_counters: null argument");
  if (!h->sim) return fail(MPC_E_ARG, "mpc_friction_set_counters: no sim bound (mpc_friction_bind)");
  DeviceGuard guard_(h->device);
  HIP_TRY(mpchost::sync_copy(h->d_counter.get(), h_counters, (size_t)h->n, hipMemcpyHostToDevice));
  return MPC_OK;
}

}  // extern "C"
