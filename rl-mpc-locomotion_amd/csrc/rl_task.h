// rl_task.h -- the per-environment arithmetic of the RL task's post-physics half, shared by the device kernels (mpc_task.hip, include/mpc_task.h)
// and host C++ (the CPU tests compile this header with g++ and compare it with the reference's own functions, tests/golden/rl_task_*.npz).
//
// What it restates (RL_Environment/tasks/aliengo.py, the same text in a1.py / go1.py, and tasks/base/vec_task.py):
//   observe        compute_robot_observations (aliengo.py:410-444) + the observation clip of VecTask.step (vec_task.py:337)
//   reward_reset   compute_robot_reward (aliengo.py:357-407): the six reward terms (:381-399) and the reset rule (:401-405)
//   begin_env      the time-out flag (vec_task.py:326), `progress_buf += 1` (aliengo.py:274) and what reset_idx does to the task's own buffers
//                  (aliengo.py:344-349)
// float32, the reference's operations in the reference's order (a Python float that meets a float32 tensor enters as its float32 value, as
// torch does it).  Compile with -ffp-contract=off: no fused multiply-adds.  Sums run left to right; torch's 12-term sum of squared torques may
// associate differently, and its exp is its own: those stay inside the reference's float32-vs-float64 gap that the tests allow.
//
// quat_rotate_inverse is Isaac Gym's (isaacgym.torch_utils) and is NOT in the reference tree: this one function is pinned by its published
// definition, a - b + c with a = v (2 w^2 - 1), b = 2 w (q x v), c = 2 q (q . v) for the quaternion (q, w) in xyzw order, not by reference source.
//
// Command sampling is NOT torch's generator: sample_commands is a counter-based generator keyed by (seed, env, episode index), so a reset draws
// the same commands whichever other environments reset with it and no generator state lives on the device.  Parity with the reference's
// torch_rand_float (aliengo.py:344-346) is in distribution only: uniform in the three configured ranges.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef MPC_HD
#if defined(__HIPCC__)
#define MPC_HD __host__ __device__ __forceinline__
#else
#define MPC_HD inline
#endif
#endif

namespace rltask {

constexpr int kObs = 48;               // pos3, body lin vel3, body ang vel3, commands3, dof pos12, dof vel12, actions12
constexpr int kLegs = 4;

// reward scales in the order of the sum at aliengo.py:398
enum { kRewLinVelXY = 0, kRewLinVelZ = 1, kRewAngVelXY = 2, kRewAngVelZ = 3, kRewTorque = 4, kRewCollision = 5, kRewTerms = 6 };

struct Config {
  float lin_vel_scale, ang_vel_scale, dof_pos_scale, dof_vel_scale;      // cfg learn.*Scale
  float rew[kRewTerms];                // cfg learn.*RewardScale, each already multiplied by dt (aliengo.py:78-79)
  float cmd_lo[3], cmd_hi[3];          // randomCommandVelocityRanges linear_x, linear_y, yaw
  float clip_obs;                      // clipObservations
  float default_dof_pos[12];           // defaultJointAngles in dof order
  long long max_episode_length;        // int(episodeLength_s / dt + 0.5), aliengo.py:74
  unsigned long long seed;
};

// Isaac Gym's quat_rotate_inverse by its published definition (see the head of this file); q = xyzw
MPC_HD void quat_rotate_inverse(const float *q, const float *v, float *out) {
  const float w = q[3];
  const float s = 2.0f * (w * w) - 1.0f;
  const float cx = q[1] * v[2] - q[2] * v[1];
  const float cy = q[2] * v[0] - q[0] * v[2];
  const float cz = q[0] * v[1] - q[1] * v[0];
  const float d = (q[0] * v[0] + q[1] * v[1]) + q[2] * v[2];
  out[0] = (v[0] * s - cx * w * 2.0f) + q[0] * d * 2.0f;
  out[1] = (v[1] * s - cy * w * 2.0f) + q[1] * d * 2.0f;
  out[2] = (v[2] * s - cz * w * 2.0f) + q[2] * d * 2.0f;
}

MPC_HD float clampf(float x, float c) { return fminf(fmaxf(x, -c), c); }

// compute_robot_observations, then the clip.  root [13], dof [12][2] (position, velocity), commands [3], actions [12]; obs[j * stride], j < 48.
MPC_HD void observe(const Config &c, const float *root, const float *dof, const float *commands, const float *actions, float *obs, int stride = 1) {
  float lin[3], ang[3];
  quat_rotate_inverse(root + 3, root + 7, lin);
  quat_rotate_inverse(root + 3, root + 10, ang);
  const float cs[3] = {c.lin_vel_scale, c.lin_vel_scale, c.ang_vel_scale};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    obs[(0 + i) * stride] = clampf(root[i], c.clip_obs);
    obs[(3 + i) * stride] = clampf(lin[i] * c.lin_vel_scale, c.clip_obs);
    obs[(6 + i) * stride] = clampf(ang[i] * c.ang_vel_scale, c.clip_obs);
    obs[(9 + i) * stride] = clampf(commands[i] * cs[i], c.clip_obs);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    obs[(12 + i) * stride] = clampf((dof[2 * i] - c.default_dof_pos[i]) * c.dof_pos_scale, c.clip_obs);
    obs[(24 + i) * stride] = clampf(dof[2 * i + 1] * c.dof_vel_scale, c.clip_obs);
    obs[(36 + i) * stride] = clampf(actions[i], c.clip_obs);
  }
}

// torch.norm(f) > 1. of one body's contact force
MPC_HD bool in_contact(const float *f) { return sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) > 1.0f; }

// What the contact-force tensor says about one environment: base / any hip over the threshold, and how many knees are.
struct Contacts {
  bool base, hip;
  int knees;
};

// contact_forces row [bodies][3] of one environment (aliengo.py:392, :401-403)
MPC_HD Contacts contacts_from_forces(const float *cf, int base_index, const int *knee_indices, const int *hip_indices) {
  Contacts k{in_contact(cf + 3 * base_index), false, 0};
#pragma unroll
  for (int l = 0; l < kLegs; ++l) {
    k.knees += in_contact(cf + 3 * knee_indices[l]) ? 1 : 0;
    k.hip = k.hip || in_contact(cf + 3 * hip_indices[l]);
  }
  return k;
}

// the toy plant's `fell` flag taken as base contact; it has no knee or hip contacts
MPC_HD Contacts contacts_from_fell(bool fell) { return Contacts{fell, false, 0}; }

// The six products of compute_robot_reward (aliengo.py:381-397) in the order of the enum above, the reference's operations in the reference's order.
// The terms are the unclipped products.  The reward itself is their sum clipped at 0, so the terms of a tick add up to less than the reward where
// the clip bit.  (The per-term episode sums, episode_terms.h, accumulate these same values: they are this function's, not a restatement of it.)
MPC_HD void reward_terms(const rltask::Config &c, const float *root, const float *commands, const float *torques, const rltask::Contacts &k,
                         float *terms) {
  using namespace rltask;
  float lin[3], ang[3];
  quat_rotate_inverse(root + 3, root + 7, lin);
  quat_rotate_inverse(root + 3, root + 10, ang);
  const float ex = commands[0] - lin[0], ey = commands[1] - lin[1], ez = commands[2] - ang[2];
  const float lin_vel_error = ex * ex + ey * ey;
  const float ang_vel_error = ez * ez;
  terms[kRewLinVelXY] = expf(-lin_vel_error / 0.25f) * c.rew[kRewLinVelXY];
  terms[kRewAngVelZ] = expf(-ang_vel_error / 0.25f) * c.rew[kRewAngVelZ];
  terms[kRewLinVelZ] = (lin[2] * lin[2]) * c.rew[kRewLinVelZ];
  terms[kRewAngVelXY] = (ang[0] * ang[0] + ang[1] * ang[1]) * c.rew[kRewAngVelXY];
  terms[kRewCollision] = (float)k.knees * c.rew[kRewCollision];
  float t2 = 0.0f;
#pragma unroll
  for (int i = 0; i < 12; ++i) t2 = t2 + torques[i] * torques[i];
  terms[kRewTorque] = t2 * c.rew[kRewTorque];
}

// the reward from its terms: the left-to-right sum (aliengo.py:398), clipped at 0 (torch.clip(total_reward, 0., None))
MPC_HD float reward_from_terms(const float *t) { return fmaxf(((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5], 0.0f); }

// compute_robot_reward: the reward, and through `reset` the next reset flag.  episode_length is progress_buf after begin_env.
MPC_HD float reward_reset(const Config &c, const float *root, const float *commands, const float *torques, const Contacts &k, long long episode_length,
                          bool &reset) {
  float terms[kRewTerms];
  reward_terms(c, root, commands, torques, k, terms);
  reset = k.base || k.knees > 0 || k.hip || episode_length > c.max_episode_length;
  return reward_from_terms(terms);
}

// ---- command sampling -----------------------------------------------------------------------------------------------------------------
MPC_HD uint64_t mix64(uint64_t x) {     // the splitmix64 finaliser
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// 24 random bits as a float32 in [0, 1): a function of (seed, env, episode, axis) alone
MPC_HD float uniform01(uint64_t seed, uint32_t env, uint32_t episode, uint32_t axis) {
  const uint64_t k = mix64(seed + 0x9E3779B97F4A7C15ull);
  const uint64_t x = mix64(k ^ mix64(((uint64_t)env << 32 | episode) + 0x9E3779B97F4A7C15ull * (axis + 1)));
  return (float)(uint32_t)(x >> 40) * (1.0f / 16777216.0f);
}

// uniform commands (vx, vy, yaw rate) in [lo, hi] of the configured ranges (aliengo.py:344-346, in distribution)
MPC_HD void sample_commands(const Config &c, uint32_t env, uint32_t episode, float *commands) {
#pragma unroll
  for (int a = 0; a < 3; ++a) commands[a] = fminf(c.cmd_lo[a] + (c.cmd_hi[a] - c.cmd_lo[a]) * uniform01(c.seed, env, episode, a), c.cmd_hi[a]);
}

// ---- the counter half of the tick ---------------------------------------------------------------------------------------------------------
// vec_task.py:326 (before the increment), aliengo.py:274, and for an environment whose reset flag is set aliengo.py:344-349.  Returns the
// environment's entry of the id array: env when it is being reset, -1 otherwise.
MPC_HD int begin_env(const Config &c, int env, long long &progress, long long &reset, long long &timeout, int &episode, float *commands) {
  timeout = progress >= c.max_episode_length - 1 ? 1 : 0;
  progress += 1;
  if (reset == 0) return -1;
  episode += 1;
  sample_commands(c, (uint32_t)env, (uint32_t)episode, commands);
  progress = 0;
  reset = 1;
  return env;
}

}  // namespace rltask
