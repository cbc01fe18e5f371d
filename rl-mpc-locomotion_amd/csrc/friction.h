// friction.h -- the arithmetic of the opt-in per-robot friction draw, shared by the device kernel (mpc_friction.hip, mpc_friction.h) and host
// C++ (the CPU tests compile this header with g++ and compare it with a numpy restatement, tests/friction_ref.py).
//
// legged_gym's randomize_friction (friction_range, 64 friction buckets) by its published algorithm, on the toy plant's Coulomb contact
// (toy_sim.h): at a draw environment r takes, for its e-th draw, u = uniform01(seed ^ kDomFriction, r, e, 0) and
//     buckets == 0     mu = fminf(lo + (hi - lo) * u, hi)
//     buckets >= 2     mu = fminf(lo + ((hi - lo) * floorf(u * buckets)) / (buckets - 1), hi)        (bucket 0 is lo, bucket buckets - 1 is hi)
// in float32 -- the form rl_task.h draws its commands in and plant_rand.h its records -- and the plant steps with (double)mu.  The clip at hi
// also takes the product u * buckets that rounds up to buckets.  Counter-based: a draw is a function of (seed, r, e) alone, depends on neither
// the batch size nor the other environments, and no generator state lives on the device beyond the draw counter e.
// Compile with -ffp-contract=off: no fused multiply-adds.
#pragma once

#include <math.h>
#include <stdint.h>

#include "domain_rand.h"
#include "rl_task.h"

namespace friction {

// 0 < lo is not asked: mu = 0 is a legal plant.  What a range must satisfy, as the float32 it is drawn in; the text of the refusal or null.
inline const char *range_error(float lo, float hi, int buckets) {
  if (!(lo >= 0.0f) || !isfinite(lo) || !isfinite(hi)) return "the friction range must be finite as float32 with lo >= 0";
  if (lo > hi) return "the friction range has lo > hi";
  if (buckets < 0 || buckets == 1) return "buckets must be 0 (a continuous draw) or at least 2";
  if (buckets > (1 << 24)) return "buckets must be at most 2^24";
  return nullptr;
}

MPC_HD float draw_mu(uint64_t seed, uint32_t env, uint32_t e, float lo, float hi, int buckets) {
  const float u = rltask::uniform01(seed ^ drand::kDomFriction, env, e, 0u);
  if (buckets > 0) return fminf(lo + ((hi - lo) * floorf(u * (float)buckets)) / (float)(buckets - 1), hi);
  return fminf(lo + (hi - lo) * u, hi);
}

}  // namespace friction
