// mpc_sim_internal.h -- what the library's other units may know of an mpc_sim (include/mpc_sim.h): its device buffers, once
// mpc_terrain_attach (include/mpc_terrain.h) has run its height field, once mpc_plant_rand_attach (mpc_plant_rand.h) has run its per-robot plant
// record, and once mpc_friction_attach (mpc_friction.h) has run its friction record.  The shell of every init and step kernel of the plant is
// sim_step.h's, and the builders of its arguments from a handle stand below.  Each unit holds the kernels of its own feature, a bounds check and
// one call into that shell each: mpc_sim.hip owns the handle and the plane kernels; mpc_terrain.hip holds the height-field kernels, which
// mpc_sim_step / mpc_sim_reset_device launch for a sim with a terrain; mpc_plant_rand.hip the step with a plant record on both grounds;
// mpc_friction.hip the Coulomb step on both grounds, with or without a plant record (a host-side branch on the handle).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "mpc_host.h"
#include "sim_step.h"
#include "toy_sim.h"

struct mpc_sim {
  int n = 0, device = 0;
  double dt = 0.0;
  mpchost::DeviceArray<double> d_f64;  // [kF64][n]
  mpchost::DeviceArray<int> d_i32, d_type;
  mpchost::DeviceArray<double> d_slope, d_yaw;
  mpchost::DeviceArray<toysim::Params> d_params;       // [n_types]
  // the terrain (null / 0 until mpc_terrain_attach): the sim's own copies
  mpchost::DeviceArray<short> d_heights;               // [rows][cols]
  mpchost::DeviceArray<double> d_origin;               // [n][2]
  int rows = 0, cols = 0;
  double hscale = 0.0, vscale = 0.0, x0 = 0.0, y0 = 0.0;
  // the per-robot plant record (null until mpc_plant_rand_attach): [kPlant][n], entry j of robot r at [j * n + r], like the state:
  // 0 payload [kg], 1 strength [factor], 2 grav_z [m/s^2, absolute]; neutral (0.0, 1.0, kGravZ)
  mpchost::DeviceArray<double> d_plant;
  // the friction record (friction false until mpc_friction_attach): the Coulomb coefficient of every robot's feet, >= 0, +inf = the anchor
  // holds; and the caller's output arrays of the step, either of which may be null
  bool friction = false;
  mpchost::DeviceArray<double> d_mu;                   // [n]
  float *d_force = nullptr;                            // [n][4][3] the ground reaction of the tick's last substep, world frame [N]
  float *d_slip = nullptr;                             // [n][4] the distance slid over the tick [m]
};

namespace simint {

constexpr int kSimThreads = 64;        // one wave per workgroup: 4096 robots are 64 waves on 64 CUs

inline dim3 sim_grid(int k) { return dim3((unsigned)((k + kSimThreads - 1) / kSimThreads)); }

// sim_step.h's launch arguments of a sim, and its two grounds (the field once a terrain is attached)
inline simstep::Args step_args(const mpc_sim *s) { return simstep::Args{s->n, s->dt, s->d_f64, s->d_i32, s->d_type, s->d_params}; }
inline simstep::PlaneSource plane_source(const mpc_sim *s) { return simstep::PlaneSource{s->d_slope}; }
inline simstep::FieldSource field_source(const mpc_sim *s) {
  return simstep::FieldSource{s->d_origin, s->d_heights, s->rows, s->cols, s->hscale, s->vscale, s->x0, s->y0};
}

// the terrain instantiations' launches (mpc_terrain.hip); the caller has set the device.  ids null = all n robots.
hipError_t terrain_launch_init(mpc_sim *s, const int *d_ids, int k, hipStream_t stream);
hipError_t terrain_launch_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, hipStream_t stream);
// the step of a sim with a plant record, on its plane or on its terrain (mpc_plant_rand.hip); the caller has set the device
hipError_t plant_launch_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, hipStream_t stream);
// the step of a sim with a friction record, on either ground, with its plant record or the neutral one (mpc_friction.hip); the caller has set the device
hipError_t friction_launch_step(mpc_sim *s, const float *d_tau, float *d_dof, float *d_root, hipStream_t stream);

}  // namespace simint
