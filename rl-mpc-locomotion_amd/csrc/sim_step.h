// sim_step.h -- the shell of the toy plant's init and step kernels, once: what every one of them does around toy_sim.h's arithmetic.  A step
// kernel of mpc_sim.hip, mpc_terrain.hip, mpc_plant_rand.hip or mpc_friction.hip is a bounds check and step_robot with a ground source (where
// robot r stands) and a plant model (what robot r steps with, and what the step publishes beside the state); an init kernel is init_robot with a
// source.  Header only, device code and plain structs: it needs toy_sim.h and no symbol of any unit.  (The host builders of Args and of the two
// sources read an mpc_sim and stand beside it in mpc_sim_internal.h.)  No LDS, no atomics, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "toy_sim.h"

namespace simstep {

using namespace toysim;

// what every kernel of the plant is launched with (the state is structure-of-arrays: entry j of robot r at [j * n + r])
struct Args {
  int n;
  double dt;
  double *f64;                       // [kF64][n]
  int *i32;                          // [kI32][n]
  const int *type;                   // [n]
  const Params *params;              // [n_types]
};

// ---- the ground sources: src(r) is the ground robot r stands on ----------------------------------------------------------------------------
struct PlaneSource {
  const double *slope;               // [n][2]
  __device__ __forceinline__ Plane operator()(int r) const { return Plane{slope[2 * r], slope[2 * r + 1]}; }
};

struct FieldSource {
  const double *origin;              // [n][2]
  const short *h;                    // [rows][cols]
  int rows, cols;
  double hscale, vscale, x0, y0;
  // the field sampled at local + (ox, oy); (0, 0): the terrain's own frame
  __device__ __forceinline__ HeightField at(double ox, double oy) const { return HeightField{h, rows, cols, hscale, vscale, x0, y0, ox, oy}; }
  __device__ __forceinline__ HeightField operator()(int r) const { return at(origin[2 * r], origin[2 * r + 1]); }
};

// ---- the plant models: what differs between the step kernels --------------------------------------------------------------------------------
// load(n, r) is what robot r steps with beside its state (read before the torques are widened) and step the tick; a model with kPublishes has
// publish, what the tick leaves beside the state (written after the state is packed), and idle, the same for a fallen robot, which does not step.
struct Nominal {                       // the robot table's plant
  static constexpr bool kPublishes = false;
  struct Record {};
  __device__ __forceinline__ Record load(size_t, int) const { return {}; }
  template <class Ground>
  __device__ __forceinline__ void step(State &s, const Params &P, const double *t, double dt, const Ground &g, Record &) const { toy_step(s, P, t, dt, g); }
};

struct PlantValues { double payload, strength, grav_z; };

// the record of robot r: one word per lane per entry, consecutive lanes on consecutive words
__device__ __forceinline__ PlantValues load_plant(const double *plant, size_t n, int r) {
  return PlantValues{plant[kPlantPayload * n + r], plant[kPlantStrength * n + r], plant[kPlantGravZ * n + r]};
}

struct PlantRecord {                   // each robot's own payload, motor strength and gravity
  static constexpr bool kPublishes = false;
  const double *plant;               // [kPlant][n]
  using Record = PlantValues;
  __device__ __forceinline__ Record load(size_t n, int r) const { return load_plant(plant, n, r); }
  template <class Ground>
  __device__ __forceinline__ void step(State &s, const Params &P, const double *t, double dt, const Ground &g, Record &p) const {
    toy_step_plant(s, P, t, dt, g, p.payload, p.strength, p.grav_z);
  }
};

struct CoulombModel {                  // ... and its own friction coefficient; publishes each foot's ground reaction and slip
  static constexpr bool kPublishes = true;
  const double *plant;              // [kPlant][n] or null: the neutral record
  const double *mu;                  // [n]
  float *force;                      // [n][4][3] or null
  float *slip;                       // [n][4] or null
  struct Record { PlantValues p; Coulomb c; };
  __device__ __forceinline__ Record load(size_t n, int r) const {
    Record rec;
    rec.p = plant ? load_plant(plant, n, r) : PlantValues{0.0, 1.0, kGravZ};   // (uniform over the launch)
    rec.c.mu = mu[r];
    return rec;
  }
  template <class Ground>
  __device__ __forceinline__ void step(State &s, const Params &P, const double *t, double dt, const Ground &g, Record &rec) const {
    toy_step_friction(s, P, t, dt, g, rec.p.payload, rec.p.strength, rec.p.grav_z, rec.c);
  }
  __device__ __forceinline__ void publish(int r, const Record &rec) const {
    if (force) {
#pragma unroll
      for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int i = 0; i < 3; ++i) force[(size_t)r * 12 + 3 * l + i] = (float)rec.c.force[l][i];
    }
    if (slip) {
#pragma unroll
      for (int l = 0; l < 4; ++l) slip[(size_t)r * 4 + l] = (float)rec.c.slip[l];
    }
  }
  __device__ __forceinline__ void idle(int r) const {
    if (force) {
#pragma unroll
      for (int j = 0; j < 12; ++j) force[(size_t)r * 12 + j] = 0.0f;
    }
    if (slip) {
#pragma unroll
      for (int j = 0; j < 4; ++j) slip[(size_t)r * 4 + j] = 0.0f;
    }
  }
};

// ---- the shell ------------------------------------------------------------------------------------------------------------------------------
// robot r's float32 observation rows (Isaac Gym's dof_state and root_states), either of which may be null
__device__ __forceinline__ void write_obs(const State &s, int r, float *dof, float *root) {
  float d[24], b[13];
  observe(s, d, b);
  if (dof) {
#pragma unroll
    for (int i = 0; i < 24; ++i) dof[(size_t)r * 24 + i] = d[i];
  }
  if (root) {
#pragma unroll
    for (int i = 0; i < 13; ++i) root[(size_t)r * 13 + i] = b[i];
  }
}

// one tick of robot r (r < a.n): a fallen robot is frozen, and observed like the others
template <class Source, class Model>
__device__ __forceinline__ void step_robot(const Args &a, int r, const Source &src, const Model &model, const float *__restrict__ tau, float *dof, float *root) {
  const auto g = src(r);                 // (in front of the state, where the plant-record and Coulomb kernels have always built it)
  State s;
  unpack(s, a.f64 + r, a.i32 + r, a.n);
  if (!s.fell) {
    typename Model::Record rec = model.load((size_t)a.n, r);
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = (double)tau[(size_t)r * 12 + i];
    model.step(s, a.params[a.type[r]], t, a.dt, g, rec);
    pack(s, a.f64 + r, a.i32 + r, a.n);
    if constexpr (Model::kPublishes) model.publish(r, rec);
  } else if constexpr (Model::kPublishes) {
    model.idle(r);
  }
  write_obs(s, r, dof, root);
}

// (re)initialise the robot in slot i (i < k) of ids (null: robot i), standing on its ground; an id outside 0 .. n - 1 names nobody
template <class Source>
__device__ __forceinline__ void init_robot(const Args &a, int i, const int *ids, const Source &src, const double *yaw0) {
  const int r = ids ? ids[i] : i;
  if (r < 0 || r >= a.n) return;
  State s;
  toy_init(s, a.params[a.type[r]], yaw0[r], src(r));
  pack(s, a.f64 + r, a.i32 + r, a.n);
}

}  // namespace simstep
