// reward_shaping.h -- the arithmetic of the opt-in reward shaping terms, of the reward they rewrite and of their per-term episode sums, shared by
// the device kernels (mpc_reward_shaping.hip, mpc_reward_shaping.h) and host C++ (the CPU tests compile this header with g++ and compare it with
// tests/reward_shaping_ref.py).
//
// What it restates, by their published formulas (legged_gym is not a dependency and nothing is checked against its source):
//   legged_gym  _reward_orientation     sum(square(projected_gravity[:, :2]))
//               _reward_base_height     square(mean(root_z - measured_heights) - base_height_target)
//               _reward_dof_vel         sum(square(dof_vel))
//               _reward_dof_acc         sum(square((last_dof_vel - dof_vel) / dt))
//               _reward_action_rate     sum(square(last_actions - actions))
//               _reward_feet_air_time   contact_filt = contact | last_contacts; first_contact = (feet_air_time > 0) * contact_filt; feet_air_time += dt;
//                                       sum((feet_air_time - 0.5) * first_contact) * (norm(commands[:, :2]) > 0.1); feet_air_time *= ~contact_filt
//               _reward_stand_still     sum(abs(dof_pos - default_dof_pos)) * (norm(commands[:, :2]) < 0.1)
//               _reward_termination     reset_buf * ~time_out_buf
//               compute_reward          rew_buf = clip(sum of the scaled terms, min=0), then the termination term on top of the clip;
//                                       episode_sums[name] += rew
// The task's own six terms are rltask::reward_terms (rl_task.h), called on what `finish` read and not restated.
//
// Compile with -ffp-contract=off.  Everything per environment is float32, one rounding per written operation, sums left to right from +0;
// everything across environments is float64 in the one fixed order of episode_terms.h (blocks of 64 environments in environment order, then
// the blocks in block order).
//
// The mean of base_height has ONE fixed order, so that a host restatement compares EQUAL.  With d[p] = root_z - heights[p], p < P:
//   lane l < 64 holds  s[l] = ((0 + d[l]) + d[l + 64]) + d[l + 128] ...   over the p = l + 64 k < P, k ascending (no such p: s[l] = 0);
//   the lanes are joined as a tree, six rounds with the strides 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + stride] for l < stride;
//   h = s[0] / (float)P.       P = 0: h = root_z (legged_gym's measured_heights of zeros).
// On the device a wave's 64 lanes sit on 64 consecutive heights of one row and the rounds are lane exchanges (height_join).
//
// Departures:
//   * this task resets first and pays the reward on the post-reset state, so the history is reset here and not in a reset_idx: on a tick whose
//     environment `begin` marked (reset_id >= 0) dof_acc, action_rate and feet_air_time are 0, air_time = 0 and last_contact = contact.  On every
//     tick the terms are taken first and then last_actions = actions and last_dof_vel = dof_vel; from the next tick on that is what legged_gym's
//     zero-then-overwrite amounts to;
//   * stand_still is paid while !moving with moving = norm > 0.1, the same flag feet_air_time uses (legged_gym's `< 0.1` differs at norm == 0.1);
//   * termination is 1 where the reset flag `finish` has just written is set and progress > max_episode_length is false: `finish`'s own time-out
//     clause, so a fall on the time-out tick counts as a time-out;
//   * a term whose scale is 0 is not evaluated: it adds nothing to the reward (not even a +0) and its sum stays 0, so a NaN in a term that is
//     switched off cannot reach the reward.  The history is kept whatever the scales are;
//   * an episode closes at the head of the tick that performs the reset, and one whose sums are not all finite closes nothing (episode_terms.h).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "episode_terms.h"
#include "rl_task.h"

namespace rshape {

enum { kOrientation = 0, kBaseHeight = 1, kDofVel = 2, kDofAcc = 3, kActionRate = 4, kFeetAirTime = 5, kStandStill = 6, kTermination = 7, kTerms = 8 };
constexpr int kTaskTerms = rltask::kRewTerms;
constexpr int kLegs = rltask::kLegs;
constexpr int kDof = 12;
constexpr int kBlock = epterms::kBlock;            // environments per block of the reduction
constexpr int kPartial = 16;                       // doubles per block partial: the closed count, the eight term sums, seven words of padding (128 bytes a row)
constexpr int kWords = 1 + kTerms;                 // the live words of a partial, and the window accumulators
constexpr int kLanes = 64;                         // lanes of the base-height mean
constexpr int kMaxPoints = 208;                    // height_scan.h's most points
// what `summary` writes: closed in window, eight window term sums, episode_length_s
enum { kSumClosed = 0, kSumTerms = 1, kSumEpisodeS = 1 + kTerms, kSummaryLen = 2 + kTerms };

struct Spec {
  float scale[kTerms];                 // per-second scale x dt, rounded to float32 once
  float base_height_target, air_time_target, dt;
};

// the history and the sums of one environment
struct Env {
  float last_actions[kDof], last_dof_vel[kDof], air_time[kLegs];
  int last_contact[kLegs];
  float sums[kTerms];
  int ticks;
};

MPC_HD bool moving(const float *commands) { return sqrtf(commands[0] * commands[0] + commands[1] * commands[1]) > 0.1f; }

// ---- the base-height mean ---------------------------------------------------------------------------------------------------------------
// lane l's strided partial over one row's P <= kMaxPoints heights (a fixed trip count: the kernel unrolls it and has every load in flight at once)
MPC_HD float height_lane_partial(float root_z, const float *heights, int P, int l) {
  float s = 0.0f;
#pragma unroll
  for (int q = 0; q < (kMaxPoints + kLanes - 1) / kLanes; ++q) {
    const int p = l + q * kLanes;
    if (p < P) s = s + (root_z - heights[p]);
  }
  return s;
}

// the tree over the 64 lane partials, in place; s[0] is the sum
MPC_HD void height_join(float *s) {
  for (int stride = kLanes / 2; stride >= 1; stride >>= 1)
    for (int l = 0; l < stride; ++l) s[l] = s[l] + s[l + stride];
}

MPC_HD float height_mean_from_sum(float sum, float root_z, int P) { return P > 0 ? sum / (float)P : root_z; }

// the whole mean on the host (the kernel runs the lanes in a wave and the tree as lane exchanges)
MPC_HD float height_mean(float root_z, const float *heights, int P) {
  float s[kLanes];
  for (int l = 0; l < kLanes; ++l) s[l] = height_lane_partial(root_z, heights, P, l);
  height_join(s);
  return height_mean_from_sum(s[0], root_z, P);
}

// ---- one tick of one environment ----------------------------------------------------------------------------------------------------------
// What `finish` read and wrote: root [13], dof [12][2], actions [12] (the clamped or noised ones), commands [3], the reset flag and progress
// AFTER finish; reset_id as `begin` wrote it; contact [4] the plant's foot flags; hbar the base-height mean.  e [kTerms] receives the scaled
// terms (0 for a scale of 0), and the history moves on.  Returns nothing: the reward is reward_from(task terms, e).
MPC_HD void tick_terms(const rltask::Config &c, const Spec &k, const float *root, const float *dof, const float *actions, const float *commands,
                       int reset_id, long long reset_flag, long long progress, const int *contact, float hbar, Env &env, float *e) {
  const bool marked = reset_id >= 0;
  const bool mv = moving(commands);
#pragma unroll
  for (int i = 0; i < kTerms; ++i) e[i] = 0.0f;
  if (k.scale[kOrientation] != 0.0f) {
    const float down[3] = {0.0f, 0.0f, -1.0f};
    float g[3];
    rltask::quat_rotate_inverse(root + 3, down, g);
    e[kOrientation] = (g[0] * g[0] + g[1] * g[1]) * k.scale[kOrientation];
  }
  if (k.scale[kBaseHeight] != 0.0f) {
    const float d = hbar - k.base_height_target;
    e[kBaseHeight] = (d * d) * k.scale[kBaseHeight];
  }
  if (k.scale[kDofVel] != 0.0f) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < kDof; ++i) s = s + dof[2 * i + 1] * dof[2 * i + 1];
    e[kDofVel] = s * k.scale[kDofVel];
  }
  if (k.scale[kDofAcc] != 0.0f && !marked) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
      const float a = (env.last_dof_vel[i] - dof[2 * i + 1]) / k.dt;
      s = s + a * a;
    }
    e[kDofAcc] = s * k.scale[kDofAcc];
  }
  if (k.scale[kActionRate] != 0.0f && !marked) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
      const float a = env.last_actions[i] - actions[i];
      s = s + a * a;
    }
    e[kActionRate] = s * k.scale[kActionRate];
  }
  // feet_air_time: the history moves whatever the scale is
  if (marked) {
#pragma unroll
    for (int l = 0; l < kLegs; ++l) {
      env.air_time[l] = 0.0f;
      env.last_contact[l] = contact[l] != 0 ? 1 : 0;
    }
  } else {
    float s = 0.0f;
#pragma unroll
    for (int l = 0; l < kLegs; ++l) {
      const bool now = contact[l] != 0;
      const bool filt = now || env.last_contact[l] != 0;
      env.last_contact[l] = now ? 1 : 0;
      const bool first = env.air_time[l] > 0.0f && filt;
      const float air = env.air_time[l] + k.dt;
      s = s + (air - k.air_time_target) * (first ? 1.0f : 0.0f);
      env.air_time[l] = air * (filt ? 0.0f : 1.0f);
    }
    if (k.scale[kFeetAirTime] != 0.0f) e[kFeetAirTime] = (mv ? s : 0.0f) * k.scale[kFeetAirTime];
  }
  if (k.scale[kStandStill] != 0.0f && !mv) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < kDof; ++i) s = s + fabsf(dof[2 * i] - c.default_dof_pos[i]);
    e[kStandStill] = s * k.scale[kStandStill];
  }
  if (k.scale[kTermination] != 0.0f) e[kTermination] = (reset_flag != 0 && !(progress > c.max_episode_length) ? 1.0f : 0.0f) * k.scale[kTermination];
#pragma unroll
  for (int i = 0; i < kDof; ++i) {
    env.last_actions[i] = actions[i];
    env.last_dof_vel[i] = dof[2 * i + 1];
  }
}

// rew = fmaxf((((((t0 + t1) + t2) + t3) + t4) + t5) + e0 + ... + e6, 0) + e7, left to right over the live terms: a scale of 0 adds nothing
MPC_HD float reward_from(const Spec &k, const float *t, const float *e) {
  float s = ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5];
#pragma unroll
  for (int i = 0; i < kTermination; ++i)
    if (k.scale[i] != 0.0f) s = s + e[i];
  float rew = fmaxf(s, 0.0f);
  if (k.scale[kTermination] != 0.0f) rew = rew + e[kTermination];
  return rew;
}

// episode_sums += the tick's terms, and the tick is counted
MPC_HD void accumulate_env(const float *e, float *sums, int &ticks) {
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sums[i] = sums[i] + e[i];
  ticks += 1;
}

// ---- the close -----------------------------------------------------------------------------------------------------------------------------
MPC_HD bool closes(int reset_id, int ticks, const float *sums) { return reset_id >= 0 && ticks > 0 && epterms::finite_sums_n<kTerms>(sums); }

// word j of one block's partial and the join's accumulator: episode_terms.h's order, with this unit's eight terms and row length
MPC_HD double block_partial_word(int count, const int *closed, const float *sums, int stride, int j) {
  return epterms::block_partial_word_n<kTerms>(count, closed, sums, stride, j);
}
MPC_HD double join_word(double acc, int blocks, const double *partials, int j) { return epterms::join_word_n<kPartial>(acc, blocks, partials, j); }

}  // namespace rshape
