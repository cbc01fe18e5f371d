// ppo_rollout.h -- the per-environment arithmetic of the collection half of a PPO iteration, shared by the device kernels (mpc_ppo.hip,
// include/mpc_ppo.h) and host C++ (the CPU tests compile this header with g++ and compare it with a torch restatement, tests/ppo_ref.py).
//
// What it restates: rsl_rl v1.0.2, the version the reference pins and trains through (RL_Environment/train.py:61-81).  rsl_rl's source is not in
// the reference tree (extern/rsl_rl is an empty submodule there): these are its published formulas.
//   sample_actions   ActorCritic.act: Normal(mean, std).sample(), and torch.distributions.Normal.log_prob summed over the twelve actions
//   bootstrap        PPO.process_env_step: rewards += gamma * (values * time_outs)
//   gae_column       RolloutStorage.compute_returns for one environment, t = T-1 .. 0; then advantages = returns - values
//   normalise_one    advantages = (advantages - mean) / (std + 1e-8), mean and unbiased std taken over all T N values by the caller in float64
// float32, rsl_rl's operations in rsl_rl's order (a Python float that meets a float32 tensor enters as its float32 value, as torch does it).
// Compile with -ffp-contract=off: no fused multiply-adds.  The bootstrap and the GAE recursion then reproduce the torch loop bit for bit; the
// log-prob's sum over the actions runs in index order from the first term (torch's reduction order is its own, and so is its log), which stays
// inside torch's float32-vs-float64 gap that the tests allow.
//
// The noise is NOT torch's generator: a counter-based generator (the splitmix64 finaliser of rl_task.h) keyed by (seed, environment, step, action
// pair), so a draw depends on neither the batch size nor the other environments and no generator state lives on the device.  One 64-bit word
// makes one Box-Muller pair, both outputs used: u1 = (24 bits + 1) / 2^24 in (0, 1], u2 = 24 bits / 2^24 in [0, 1).  The smallest u1 is 2^-24, so
// |eps| <= sqrt(-2 log 2^-24) = 5.768: the normal is truncated there (mass outside: 8e-9 per draw).  Parity with torch is in distribution only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rl_task.h"

namespace ppo {

constexpr int kActions = 12;
constexpr int kPairs = kActions / 2;
constexpr float kLogSqrt2Pi = 0.9189385332046727f;     // math.log(math.sqrt(2 * math.pi)) of Normal.log_prob, as the float32 it becomes
constexpr float kTwoPi = 6.283185307179586f;
constexpr uint64_t kNoiseDomain = 0x50504F5F4E4F4953ull;   // keeps these draws apart from rl_task.h's command draws of the same seed

// standard normals 2 * pair and 2 * pair + 1 of environment env at step `step`: a function of (seed, env, step, pair) alone
MPC_HD void normal_pair(uint64_t seed, uint32_t env, uint32_t step, uint32_t pair, float &z0, float &z1) {
  const uint64_t k = rltask::mix64((seed ^ kNoiseDomain) + 0x9E3779B97F4A7C15ull);
  const uint64_t x = rltask::mix64(k ^ rltask::mix64(((uint64_t)env << 32 | step) + 0x9E3779B97F4A7C15ull * (pair + 1)));
  const float u1 = (float)((uint32_t)(x >> 40) + 1u) * (1.0f / 16777216.0f);            // (0, 1]: log never sees 0
  const float u2 = (float)((uint32_t)(x >> 16) & 0xFFFFFFu) * (1.0f / 16777216.0f);     // [0, 1)
  const float r = sqrtf(-2.0f * logf(u1));
  const float th = kTwoPi * u2;
  z0 = r * cosf(th);
  z1 = r * sinf(th);
}

// Normal(mean, std).sample() with the given noise: a product, then a sum
MPC_HD float action_of(float mean, float std, float eps) { return mean + std * eps; }

// one term of Normal.log_prob: -((a - mean) ** 2) / (2 * std ** 2) - log(std) - log(sqrt(2 pi))
MPC_HD float log_prob_term(float a, float mean, float std) {
  const float d = a - mean;
  return (-(d * d) / (2.0f * (std * std)) - logf(std)) - kLogSqrt2Pi;
}

// ... summed over the actions in index order from the first term (get_actions_log_prob: log_prob(actions).sum(dim=-1))
MPC_HD float log_prob_sum(const float *terms, int stride = 1) {
  float s = terms[0];
#pragma unroll
  for (int k = 1; k < kActions; ++k) s = s + terms[k * stride];
  return s;
}

// ActorCritic.act for one environment: eps[12], actions[12] and the summed log-prob
MPC_HD float sample_actions(uint64_t seed, uint32_t env, uint32_t step, const float *mean, const float *std, float *eps, float *actions) {
  float terms[kActions];
#pragma unroll
  for (int p = 0; p < kPairs; ++p) normal_pair(seed, env, step, (uint32_t)p, eps[2 * p], eps[2 * p + 1]);
#pragma unroll
  for (int k = 0; k < kActions; ++k) {
    actions[k] = action_of(mean[k], std[k], eps[k]);
    terms[k] = log_prob_term(actions[k], mean[k], std[k]);
  }
  return log_prob_sum(terms);
}

// PPO.process_env_step: r' = r + gamma * (v * time_out), time_out in {0, 1}
MPC_HD float bootstrap(float r, float gamma, float v, float time_out) { return r + gamma * (v * time_out); }

// RolloutStorage.compute_returns for one environment whose T entries sit `stride` words apart; adv receives returns - values (un-normalised)
MPC_HD void gae_column(int T, size_t stride, const float *rewards, const float *dones, const float *values, float last_value, float gamma, float lam,
                       float *returns, float *adv) {
  float a = 0.0f, nv = last_value;
  for (int t = T - 1; t >= 0; --t) {
    const float v = values[t * stride];
    const float nnt = 1.0f - dones[t * stride];
    const float g = nnt * gamma;
    const float delta = (rewards[t * stride] + g * nv) - v;
    a = delta + (g * lam) * a;
    const float ret = a + v;
    returns[t * stride] = ret;
    adv[t * stride] = ret - v;
    nv = v;
  }
}

// (A - mean) / (std + 1e-8) with the float64 moments of the caller, rounded once
MPC_HD float normalise_one(float a, double mean, double std) { return (float)(((double)a - mean) / (std + 1e-8)); }

// mean and unbiased standard deviation (torch.Tensor.std) of m values in float64, two passes in index order: the host statement of what the
// device kernel computes as a fixed-order tree
inline void moments(const float *a, size_t m, double &mean, double &std) {
  double s = 0.0;
  for (size_t i = 0; i < m; ++i) s += (double)a[i];
  mean = s / (double)m;
  double q = 0.0;
  for (size_t i = 0; i < m; ++i) { const double d = (double)a[i] - mean; q += d * d; }
  std = sqrt(q / (double)(m - 1));
}

}  // namespace ppo
