// mpc_terrain.hip -- the C ABI of include/mpc_terrain.h: toy_sim.h's HeightField instantiations of toy_init / toy_step on the device, one lane
// per robot as in mpc_sim.hip (sim_step.h's shell with its field source and the nominal plant), a point query of the surface, and the accessors
// of the origin array (mpc_curriculum.h).  The field is int16 in HBM, read with plain 2-byte loads (four per lookup): a 500 x 500 field is
// 500 KB and stays in the caches.  mpc_sim.hip owns the handle (mpc_sim_internal.h) and launches these through simint::terrain_launch_* once a
// terrain is attached.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mpc_terrain.h"
#include "mpc_curriculum.h"
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

// (re)initialise robots ids[0 .. k) (all n when ids is null) standing on the terrain
__global__ __launch_bounds__(kSimThreads) void terrain_init_kernel(Args a, FieldSource f, const double *yaw0, const int *ids, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) init_robot(a, i, ids, f, yaw0);
}

__global__ __launch_bounds__(kSimThreads) void terrain_step_kernel(Args a, FieldSource f, const float *__restrict__ tau, float *dof, float *root) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) step_robot(a, r, f, Nominal{}, tau, dof, root);
}

// the surface at k points of the terrain's own frame
__global__ __launch_bounds__(kSimThreads) void terrain_query_kernel(FieldSource f, const double *__restrict__ xy, int k, double *z, double *normal) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const HeightField g = f.at(0.0, 0.0);
  const double p[2] = {xy[2 * (size_t)i], xy[2 * (size_t)i + 1]};
  z[i] = g.height(p);
  if (normal) {
    double nn[3];
    g.normal(p, nn);
#pragma unroll
    for (int j = 0; j < 3; ++j) normal[3 * (size_t)i + j] = nn[j];
  }
}
}  // namespace

namespace simint {

hipError_t terrain_launch_init(mpc_sim *s, const int *d_ids, int k, hipStream_t stream) {
  hipLaunchKernelGGL(terrain_init_kernel, sim_grid(k), dim3(kSimThreads), 0, stream, step_args(s), field_source(s), (const double *)s->d_yaw, d_ids, k);
  return hipGetLastError();
}

hipError_t terrain_launch_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, hipStream_t stream) {
  hipLaunchKernelGGL(terrain_step_kernel, sim_grid(s->n), dim3(kSimThreads), 0, stream, step_args(s), field_source(s), d_tau, d_dof, d_root);
  return hipGetLastError();
}

}  // namespace simint

extern "C" {

const char *mpc_terrain_last_error(void) { return g_err.c_str(); }

int mpc_terrain_attach(mpc_sim *s, int rows, int cols, const short *h_heights, double hscale, double vscale, double x0, double y0,
                       const double *origin) {
  // everything that does not need the handle first, so that each check can be met without a device
  if (rows < MPC_TERRAIN_MIN_NODES || rows > MPC_TERRAIN_MAX_NODES || cols < MPC_TERRAIN_MIN_NODES || cols > MPC_TERRAIN_MAX_NODES)
    return fail(MPC_E_ARG, "mpc_terrain_attach: rows and cols must be in 2 .. 4096");
  if (!std::isfinite(hscale) || !(hscale > 0.0) || !std::isfinite(vscale) || !(vscale > 0.0))
    return fail(MPC_E_ARG, "mpc_terrain_attach: hscale and vscale must be finite and > 0");
  if (!std::isfinite(x0) || !std::isfinite(y0)) return fail(MPC_E_ARG, "mpc_terrain_attach: x0 and y0 must be finite");
  if (!h_heights) return fail(MPC_E_ARG, "mpc_terrain_attach: null heights");
  if (!s) return fail(MPC_E_ARG, "mpc_terrain_attach: null sim handle");
  const size_t n = (size_t)s->n, cells = (size_t)rows * (size_t)cols;
  std::vector<double> org(2 * n, 0.0);
  if (origin)
    for (size_t i = 0; i < org.size(); ++i) {
      if (!std::isfinite(origin[i])) return fail(MPC_E_ARG, "mpc_terrain_attach: origin of robot " + std::to_string(i / 2) + " is not finite");
      org[i] = origin[i];
    }
  DeviceGuard guard_(s->device);
  // both new arrays are built first: a failed attach leaves the terrain attached earlier in place (the temporaries free what they hold)
  mpchost::DeviceArray<short> d_h;
  mpchost::DeviceArray<double> d_o;
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess || (e = d_h.alloc_copy(h_heights, cells)) != hipSuccess ||
      (e = d_o.alloc_copy(org.data(), org.size())) != hipSuccess)
    return fail(MPC_E_HIP, std::string("mpc_terrain_attach: ") + hipGetErrorString(e));
  // (a terrain attached earlier is replaced and freed; the device is idle after the synchronisation above)
  s->d_heights = std::move(d_h); s->d_origin = std::move(d_o);
  s->rows = rows; s->cols = cols;
  s->hscale = hscale; s->vscale = vscale; s->x0 = x0; s->y0 = y0;
  HIP_TRY(simint::terrain_launch_init(s, nullptr, s->n, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return MPC_OK;
}

int mpc_terrain_query(mpc_sim *s, const double *d_xy, int k, double *d_z, double *d_normal, void *stream) {
  if (k < 0) return fail(MPC_E_ARG, "mpc_terrain_query: negative point count");
  if (!d_xy || !d_z) return fail(MPC_E_ARG, "mpc_terrain_query: null points or heights");
  if (!s) return fail(MPC_E_ARG, "mpc_terrain_query: null sim handle");
  if (!s->d_heights) return fail(MPC_E_ARG, "mpc_terrain_query: the sim has no terrain attached");
  if (k == 0) return MPC_OK;
  DeviceGuard guard_(s->device);
  hipLaunchKernelGGL(terrain_query_kernel, sim_grid(k), dim3(kSimThreads), 0, reinterpret_cast<hipStream_t>(stream), simint::field_source(s), d_xy, k, d_z, d_normal);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

// (declared in mpc_curriculum.h) the origin array of a sim with a terrain: its device address, and its contents on the host
int mpc_terrain_origins(mpc_sim *s, double **d_origin) {
  if (!d_origin) return fail(MPC_E_ARG, "mpc_terrain_origins: null result pointer");
  if (!s) return fail(MPC_E_ARG, "mpc_terrain_origins: null sim handle");
  if (!s->d_origin) return fail(MPC_E_ARG, "mpc_terrain_origins: the sim has no terrain attached");
  *d_origin = s->d_origin;
  return MPC_OK;
}

int mpc_terrain_get_origins(mpc_sim *s, double *h_origin) {
  if (!h_origin) return fail(MPC_E_ARG, "mpc_terrain_get_origins: null result pointer");
  if (!s) return fail(MPC_E_ARG, "mpc_terrain_get_origins: null sim handle");
  if (!s->d_origin) return fail(MPC_E_ARG, "mpc_terrain_get_origins: the sim has no terrain attached");
  DeviceGuard guard_(s->device);
  HIP_TRY(mpchost::sync_copy(h_origin, s->d_origin.get(), 2 * (size_t)s->n, hipMemcpyDeviceToHost));
  return MPC_OK;
}

}  // extern "C"
