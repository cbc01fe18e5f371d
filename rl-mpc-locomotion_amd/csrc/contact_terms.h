// contact_terms.h -- the arithmetic of the opt-in contact reward terms, of the reward they rewrite, of their per-term episode sums and of the critic's
// friction and ground-reaction columns, shared by the device kernels (mpc_contact_terms.hip, mpc_contact_terms.h) and host C++ (the CPU tests
// compile this header with g++ and compare it with tests/contact_terms_ref.py).
//
// What it restates, by their published formulas (legged_gym is not a dependency and nothing is checked against its source):
//   legged_gym  _reward_feet_contact_forces   sum((norm(contact_forces[:, feet], dim=-1) - max_contact_force).clip(min=0.))
//               _reward_feet_stumble          any(norm(contact_forces[:, feet, :2], dim=2) > 5 * abs(contact_forces[:, feet, 2]))
//   its descendants'  feet_slip               sum(square(norm(foot_velocities[:, :, :2], dim=2)) * contact_filt)
//               compute_reward                rew_buf = clip(sum of the scaled terms, min=0), then the termination term on top of the clip;
//                                             episode_sums[name] += rew
// The inputs are the plant's own outputs (toy_sim.h's Coulomb contact): F [4][3] the ground reaction of the tick's last substep, world frame,
// newtons, and S [4] the distance each foot slid over the tick, metres.
//
// Compile with -ffp-contract=off.  Everything per environment is float32, one rounding per written operation, sums left to right from +0; sqrtf and
// the division are IEEE.  Everything across environments is float64 in the one fixed order of episode_terms.h.
//   feet_slip            v_l = S[l] / dt;                              sum_l v_l * v_l
//   feet_contact_forces  m_l = sqrtf((Fx * Fx + Fy * Fy) + Fz * Fz);   sum_l fmaxf(m_l - max_contact_force, 0)
//   feet_stumble         1 where any leg has sqrtf(Fx * Fx + Fy * Fy) > 5 * fabsf(Fz), else 0
// each times its scale (the per-second value x dt, rounded to float32 once).
//
// Departures:
//   * feet_slip has no contact filter.  The published term multiplies by a filtered contact flag; the plant's force (and its contact flag) belongs
//     to the tick's last substep only, while S is the slide of the whole tick, and a foot that slid and then lifted within the tick must still count;
//   * feet_slip reads the plant's slide over the tick divided by dt, a mean speed, where the published term reads an instantaneous foot velocity;
//   * on a tick whose environment `begin` marked (reset_id >= 0) all three terms are 0, as the shaping terms treat their history on that tick (the
//     rows the terms would read are the zeros friction's draw has just written: the finished episode's last reaction is not charged to the new one);
//   * a term whose scale is 0 is not evaluated: it adds nothing to the reward (not even a +0) and its sum stays 0, so a NaN or an inf in an input
//     of a term that is switched off cannot reach the reward;
//   * fmaxf(NaN, 0) is 0: a NaN force gives feet_contact_forces a 0 and feet_stumble a false comparison, so it reaches neither; an inf force, and a
//     NaN or inf slide, do reach their terms, the reward is then fmaxf's 0 and the episode closes nothing (episode_terms.h);
//   * the contact terms sit inside legged_gym's clip and the shaping `termination` term stays on top of it.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "episode_terms.h"
#include "rl_task.h"

namespace cterms {

enum { kFeetSlip = 0, kFeetContactForces = 1, kFeetStumble = 2, kTerms = 3 };
constexpr int kLegs = rltask::kLegs;
constexpr int kTaskTerms = rltask::kRewTerms;
constexpr int kShapingTerms = 8;                   // reward_shaping.h's terms, as its `terms` tensor holds them
constexpr int kShapingTermination = 7;             // the one that stays on top of the clip
constexpr int kBlock = epterms::kBlock;            // environments per block of the reduction
constexpr int kPartial = 8;                        // doubles per block partial: the closed count, the three term sums, four words of padding (64 bytes a row)
constexpr int kWords = 1 + kTerms;                 // the live words of a partial, and the window accumulators
constexpr int kColumns = 16;                       // what the privileged row grows by: mu, twelve force components, three zeros
// what `summary` writes: closed in window, three window term sums, episode_length_s
enum { kSumClosed = 0, kSumTerms = 1, kSumEpisodeS = 1 + kTerms, kSummaryLen = 2 + kTerms };

struct Spec {
  float scale[kTerms];                 // per-second scale x dt, rounded to float32 once
  float max_contact_force, dt;
  float force_scale, mu_clip, clip_obs;        // the critic's columns
};

// the float32 scales of the reward shaping unit whose `terms` tensor the reward reads (live = 0: no shaping)
struct Shaping {
  int live;
  float scale[kShapingTerms];
};

// ---- one tick of one environment ------------------------------------------------------------------------------------------------------------
// F [4][3] and S [4] of the environment, reset_id as `begin` wrote it; e [kTerms] receives the scaled terms (0 for a scale of 0 and on a marked tick)
MPC_HD void tick_terms(const Spec &k, const float *F, const float *S, int reset_id, float *e) {
  const bool marked = reset_id >= 0;
#pragma unroll
  for (int i = 0; i < kTerms; ++i) e[i] = 0.0f;
  if (marked) return;
  if (k.scale[kFeetSlip] != 0.0f) {
    float s = 0.0f;
#pragma unroll
    for (int l = 0; l < kLegs; ++l) {
      const float v = S[l] / k.dt;
      s = s + v * v;
    }
    e[kFeetSlip] = s * k.scale[kFeetSlip];
  }
  if (k.scale[kFeetContactForces] != 0.0f) {
    float s = 0.0f;
#pragma unroll
    for (int l = 0; l < kLegs; ++l) {
      const float *f = F + 3 * l;
      const float m = sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
      s = s + fmaxf(m - k.max_contact_force, 0.0f);
    }
    e[kFeetContactForces] = s * k.scale[kFeetContactForces];
  }
  if (k.scale[kFeetStumble] != 0.0f) {
    bool any = false;
#pragma unroll
    for (int l = 0; l < kLegs; ++l) {
      const float *f = F + 3 * l;
      any = any || sqrtf(f[0] * f[0] + f[1] * f[1]) > 5.0f * fabsf(f[2]);
    }
    e[kFeetStumble] = (any ? 1.0f : 0.0f) * k.scale[kFeetStumble];
  }
}

// The unclipped chain the step without this unit clips: rltask::reward_from_terms' argument over the task's six terms t, and with a reward shaping
// unit rshape::reward_from's s over its live terms se [8] below `termination` (a scale of 0 adds nothing).
MPC_HD float chain_from(const Shaping &g, const float *t, const float *se) {
  float s = ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5];
  if (g.live) {
#pragma unroll
    for (int i = 0; i < kShapingTermination; ++i)
      if (g.scale[i] != 0.0f) s = s + se[i];
  }
  return s;
}

// rew = fmaxf(((s + k0) + k1) + k2, 0) over the live contact terms, plus the shaping termination term where that is live
MPC_HD float reward_from(const Spec &k, const Shaping &g, float s, const float *e, const float *se) {
#pragma unroll
  for (int i = 0; i < kTerms; ++i)
    if (k.scale[i] != 0.0f) s = s + e[i];
  float rew = fmaxf(s, 0.0f);
  if (g.live && g.scale[kShapingTermination] != 0.0f) rew = rew + se[kShapingTermination];
  return rew;
}

// episode_sums += the tick's terms, and the tick is counted
MPC_HD void accumulate_env(const float *e, float *sums, int &ticks) {
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sums[i] = sums[i] + e[i];
  ticks += 1;
}

// ---- the close --------------------------------------------------------------------------------------------------------------------------------
MPC_HD bool closes(int reset_id, int ticks, const float *sums) { return reset_id >= 0 && ticks > 0 && epterms::finite_sums_n<kTerms>(sums); }

// word j of one block's partial and the join's accumulator: episode_terms.h's order, with this unit's three terms and row length
MPC_HD double block_partial_word(int count, const int *closed, const float *sums, int stride, int j) {
  return epterms::block_partial_word_n<kTerms>(count, closed, sums, stride, j);
}
MPC_HD double join_word(double acc, int blocks, const double *partials, int j) { return epterms::join_word_n<kPartial>(acc, blocks, partials, j); }

// ---- the critic's columns ---------------------------------------------------------------------------------------------------------------------
// column j < kColumns past the assembled row: 0 the friction coefficient (>= 0, +inf allowed, never NaN) clipped from above, 1 .. 12 the ground
// reaction leg-major, scaled and clipped to the task's clip_observations, 13 .. 15 zeros
MPC_HD float column(const Spec &k, double mu, const float *F, int j) {
  if (j == 0) return fminf((float)mu, k.mu_clip);
  if (j <= 3 * kLegs) return fminf(fmaxf(F[j - 1] * k.force_scale, -k.clip_obs), k.clip_obs);
  return 0.0f;
}

}  // namespace cterms
