// episode_terms.h -- the arithmetic of the per-term episode reward sums and of the command curriculum they drive, shared by the device kernels
// (mpc_episode_terms.hip, mpc_episode_terms.h) and host C++ (the CPU tests compile this header with g++ and compare it with
// tests/episode_terms_ref.py).
//
// What it restates, by their published algorithms (legged_gym and rsl_rl are not dependencies and nothing is checked against their source):
//   legged_gym  compute_reward               episode_sums[name] += rew                     one float32 add per term and tick
//               reset_idx                    extras["episode"]["rew_" + name] = mean(episode_sums[name][env_ids]) / max_episode_length_s,
//                                            then update_command_curriculum, then episode_sums[env_ids] = 0, then _resample_commands
//               update_command_curriculum    if mean(episode_sums["tracking_lin_vel"][env_ids]) / max_episode_length > 0.8 * reward_scale:
//                                              lin_vel_x[0] = clip(lin_vel_x[0] - 0.5, -max_curriculum, 0.)
//                                              lin_vel_x[1] = clip(lin_vel_x[1] + 0.5, 0., max_curriculum)
//                                            called when common_step_counter % max_episode_length == 0
//   rsl_rl      the runner's ep_infos        the mean of the "rew_<term>" entries over an iteration
// The six terms are rltask::reward_terms (rl_task.h), the function reward_reset itself sums; "tracking_lin_vel" is its lin_vel_xy.
//
// Compile with -ffp-contract=off.  The per-environment sums are float32, everything across environments is float64.
//
// The reduction over the closed environments has ONE fixed order, so that a host restatement compares EQUAL: environments in blocks of kBlock = 64
// consecutive indices; inside a block the closed environments' float32 sums are added in environment order, in float64; the block sums are added
// in block order, in float64.  The closed count follows the same rule (it is exact either way).
//
// Departures:
//   * the mean is that float64 blocked sum, not torch's float32 `mean`;
//   * the record (the window accumulators) is episode-weighted over an iteration: every closed episode counts once.  rsl_rl averages per-tick
//     means, and legged_gym re-reports a stale dictionary on ticks without resets;
//   * an episode is closed at the head of the tick that PERFORMS the reset (the task's `begin` has just marked it), one tick later than
//     legged_gym's same-tick reset_idx.  Its sums hold every tick of the episode either way;
//   * the command draws are rl_task.h's counter-based generator keyed by (seed, env, count, 4 + axis), `count` being this unit's own count of the
//     environment's resamples: parity with torch_rand_float is in distribution only (uniform in the current ranges);
//   * only the x range moves.  The y and yaw ranges stay the configured ones;
//   * an episode whose sums are not all finite is zeroed and resampled like any other but closes nothing: it is neither counted nor added.  A
//     plant state that has blown up gives NaN terms (the reward hides them: fmaxf(NaN, 0) is 0), and torch's mean over such an episode would be
//     NaN -- no widening on that tick, and a NaN record for the whole iteration.  The terrain curriculum and the observation normaliser leave
//     such rows out in the same way.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rl_task.h"

namespace epterms {

constexpr int kTerms = rltask::kRewTerms;
constexpr int kBlock = 64;             // environments per block of the reduction
constexpr int kPartial = 8;            // doubles per block partial: the closed count, the six term sums, one word of padding (64 bytes a row)
constexpr uint32_t kCommandAxis = 4;   // uniform01's axis tags 4, 5, 6: sample_commands uses 0, 1, 2 and the terrain curriculum's redraw 3

// the device-resident float64 state, one array: the three command ranges, the window accumulators, the widenings counter
enum { kGlobRanges = 0, kGlobWindow = 6, kGlobWidenings = 6 + 1 + kTerms, kGlobLen = 6 + 1 + kTerms + 1 };
// what `summary` writes: closed in window, six window term sums, x lo, x hi, widenings, max_episode_length_s
enum { kSumClosed = 0, kSumTerms = 1, kSumLo = 1 + kTerms, kSumHi = 2 + kTerms, kSumWidenings = 3 + kTerms, kSumEpisodeS = 4 + kTerms, kSummaryLen = 5 + kTerms };

// the six products of a tick and their clipped sum are the task's own (rl_task.h), so the sums of an episode add up to its reward by construction
using rltask::reward_from_terms;
using rltask::reward_terms;

// one tick of one environment: episode_sums += rew, and the tick is counted
MPC_HD void accumulate_env(const float *terms, float *sums, int &ticks) {
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sums[i] = sums[i] + terms[i];
  ticks += 1;
}

// false for NaN and +-inf in any of the kT sums (reward_shaping.h keeps eight)
template <int kT>
MPC_HD bool finite_sums_n(const float *sums) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < kT; ++i) ok = ok && fabsf(sums[i]) <= 3.402823466e+38f;
  return ok;
}

// false for NaN and +-inf in any of the six sums
MPC_HD bool finite_sums(const float *sums) { return finite_sums_n<kTerms>(sums); }

// An environment closes an episode when the task's `begin` has just marked it, its sums hold at least one tick (on the first tick every
// environment is marked and none has: nothing closes) and all six are finite.
MPC_HD bool closes(int reset_id, int ticks, const float *sums) { return reset_id >= 0 && ticks > 0 && finite_sums(sums); }

// Word j of one block's partial (0: the closed count, 1 + i: term i; the pad word is 0): the closed environments among the block's `count`, in
// environment order.  closed[e] != 0 and sums[e * stride + i] are the block's own (the kernel hands its LDS copy, the host the arrays).
// (the _n forms state the order once for any number of terms kT and any row length kP: reward_shaping.h reduces eight terms in rows of 16)
template <int kT>
MPC_HD double block_partial_word_n(int count, const int *closed, const float *sums, int stride, int j) {
  double acc = 0.0;
  if (j > kT) return acc;
  for (int e = 0; e < count; ++e)
    if (closed[e]) acc = acc + (j == 0 ? 1.0 : (double)sums[(size_t)e * stride + (j - 1)]);
  return acc;
}
MPC_HD double block_partial_word(int count, const int *closed, const float *sums, int stride, int j) {
  return block_partial_word_n<kTerms>(count, closed, sums, stride, j);
}

// the join's accumulator of word j over `blocks` partial rows, in block order, continuing from acc
template <int kP>
MPC_HD double join_word_n(double acc, int blocks, const double *partials, int j) {
  for (int b = 0; b < blocks; ++b) acc = acc + partials[(size_t)b * kP + j];
  return acc;
}
MPC_HD double join_word(double acc, int blocks, const double *partials, int j) { return join_word_n<kPartial>(acc, blocks, partials, j); }

// the command curriculum's numbers, as the kernel takes them
struct Curriculum {
  int enabled;                         // 0: close, zero and resample only; the decision is skipped
  long long tick, update_every;        // the decision runs on ticks with tick % update_every == 0
  double max_episode_length;           // the configured episode length in ticks
  double threshold, scale;             // 0.8 and (double)rew[kRewLinVelXY] (already multiplied by dt)
  double step, max_curriculum;
};

MPC_HD double clipd(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// update_command_curriculum on the joined sums S [kPartial] (S[0] the closed count): true when the x range was widened
MPC_HD bool decide(const Curriculum &k, const double *S) {
  if (!k.enabled || k.tick % k.update_every != 0) return false;
  if (!(S[0] > 0.0)) return false;
  return (S[1 + rltask::kRewLinVelXY] / S[0]) / k.max_episode_length > k.threshold * k.scale;
}

// The tail of the join: the decision, the range update and the window accumulators, on glob [kGlobLen].
MPC_HD void join_tail(const Curriculum &k, const double *S, double *glob) {
  if (decide(k, S)) {
    glob[kGlobRanges + 0] = clipd(glob[kGlobRanges + 0] - k.step, -k.max_curriculum, 0.0);
    glob[kGlobRanges + 1] = clipd(glob[kGlobRanges + 1] + k.step, 0.0, k.max_curriculum);
    glob[kGlobWidenings] = glob[kGlobWidenings] + 1.0;
  }
  for (int j = 0; j < 1 + kTerms; ++j) glob[kGlobWindow + j] = glob[kGlobWindow + j] + S[j];
}

// fresh commands of one marked environment from the current ranges [3][2]: a function of (seed, env, count, ranges) alone
MPC_HD void resample_env(unsigned long long seed, int env, int count, const double *ranges, float *commands) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = (float)ranges[2 * a], hi = (float)ranges[2 * a + 1];
    commands[a] = fminf(lo + (hi - lo) * rltask::uniform01(seed, (uint32_t)env, (uint32_t)count, kCommandAxis + (uint32_t)a), hi);
  }
}

}  // namespace epterms
