// plant_rand.h -- the arithmetic of the opt-in per-robot plant randomisation, shared by the device kernel (mpc_plant_rand.hip, mpc_plant_rand.h)
// and host C++ (the CPU tests compile this header with g++ and compare it with a numpy restatement, tests/plant_rand_ref.py).
//
// legged_gym's randomize_base_mass (added_mass_range) and the motor-strength and gravity randomisation of its descendants, by their published
// algorithms, on the toy plant's record (toy_sim.h: payload, strength, grav_z).  At a reset environment r draws, for its e-th draw,
//     v_axis = fminf(lo + (hi - lo) * uniform01(seed ^ kDomPlant, r, e, axis), hi)        axis 0 payload, 1 strength, 2 gravity offset
// in float32 -- the form rl_task.h draws its commands in and domain_rand.h its pushes -- and its record becomes
//     payload = (double)v0        strength = (double)v1        grav_z = kGravZ + (double)v2
// An axis without a range is not drawn and gets its neutral value (0.0, 1.0, kGravZ).  Counter-based: a draw is a function of (seed, r, e, axis)
// alone, depends on neither the batch size nor the other environments, and no generator state lives on the device beyond the draw counter e.
// Compile with -ffp-contract=off: no fused multiply-adds.
#pragma once

#include <math.h>
#include <stdint.h>

#include "domain_rand.h"
#include "rl_task.h"
#include "toy_sim.h"

namespace plantrand {

constexpr int kAxes = toysim::kPlant;  // payload, strength, gravity offset

struct Ranges {
  int present[kAxes];                  // 0: the axis is not randomised
  float lo[kAxes], hi[kAxes];
};

MPC_HD double neutral(int axis) { return axis == toysim::kPlantStrength ? 1.0 : (axis == toysim::kPlantGravZ ? toysim::kGravZ : 0.0); }

MPC_HD float draw_value(uint64_t seed, uint32_t env, uint32_t e, uint32_t axis, float lo, float hi) {
  return fminf(lo + (hi - lo) * rltask::uniform01(seed ^ drand::kDomPlant, env, e, axis), hi);
}

// environment env's record after its e-th draw: rec[kAxes]
MPC_HD void draw_record(uint64_t seed, uint32_t env, uint32_t e, const Ranges &rg, double *rec) {
#pragma unroll
  for (int a = 0; a < kAxes; ++a) {
    if (!rg.present[a]) {
      rec[a] = neutral(a);
      continue;
    }
    const double v = (double)draw_value(seed, env, e, (uint32_t)a, rg.lo[a], rg.hi[a]);
    rec[a] = a == toysim::kPlantGravZ ? toysim::kGravZ + v : v;
  }
}

}  // namespace plantrand
