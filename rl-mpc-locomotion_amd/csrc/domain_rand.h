// domain_rand.h -- the per-element arithmetic of the opt-in domain randomisation, shared by the device kernels (mpc_domain_rand.hip,
// mpc_domain_rand.h) and host C++ (the CPU tests compile this header with g++ and compare it with the reference's own noise lambdas,
// tests/golden/domain_rand.npz, and with a numpy restatement, tests/domain_rand_ref.py).
//
// What it restates:
//   apply          the noise lambdas that VecTask.apply_randomizations builds (RL_Environment/tasks/base/vec_task.py:563-571 gaussian,
//                  :590-597 uniform) and VecTask.step applies to the actions before their clamp (:308-312) and to the observations before
//                  theirs (:331-337), with the clamp:
//                      corr = zc * s_corr + m_corr            the persistent 'corr' (:565-569, :592-596)
//                      term = (corr + d * s) + m              :571 / :597
//                      term = term * col_scale                (1.0f without a column scale: legged_gym's noise_scale_vec form)
//                      y    = x + term  |  x * term           'additive' | 'scaling'
//                      out  = clamp(y, -clip, clip)           torch.clamp: a NaN stays a NaN
//                  gaussian: d standard normal, (m, s, m_corr, s_corr) = (mu, var, mu_corr, var_corr) -- the reference multiplies by what it
//                  calls var.  uniform: d uniform in [0, 1), s = hi - lo, m = lo; the correlated draw zc is STILL a standard normal, scaled by
//                  hi_corr - lo_corr plus lo_corr: that is what :594-596 does.  The schedule (:533-561, :579-588) is host Python
//                  (domain_rand.py): this header sees the scheduled values as the float32 they become when they meet a float32 tensor.
//   push_value     legged_gym's _push_robots by its published algorithm: the base's world x, y velocity becomes uniform in [-v, v].
// float32, one operation per arrow, the reference's order.  Compile with -ffp-contract=off: no fused multiply-adds.
//
// The draws are NOT torch's generator: counter-based (rl_task.h's splitmix64 finaliser and uniform01, ppo_rollout.h's Box-Muller pair), keyed by
// (seed ^ a domain constant, environment, tick, column or column pair).  A draw depends on neither the batch size, the row width nor the other
// environments, and no generator state lives on the device: zc, which the reference draws once and keeps, is a function of (seed, environment,
// column) alone and is recomputed every tick.  One Box-Muller pair serves columns 2p and 2p + 1.  Parity with torch is in distribution only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ppo_rollout.h"
#include "rl_task.h"

namespace drand {

// one constant per stream of draws, XORed into the seed: the draws of one seed stay apart from each other, from rl_task.h's commands and from
// ppo_rollout.h's action sampling
constexpr uint64_t kDomObsNoise = 0x44524F42534E4F49ull;
constexpr uint64_t kDomObsCorr = 0x44524F4253434F52ull;
constexpr uint64_t kDomActNoise = 0x44524143544E4F49ull;
constexpr uint64_t kDomActCorr = 0x4452414354434F52ull;
constexpr uint64_t kDomPush = 0x445250555348585Aull;
constexpr uint64_t kDomPlant = 0x4452504C414E5458ull;      // plant_rand.h's payload / motor strength / gravity draws
constexpr uint64_t kDomFriction = 0x4452465249435458ull;   // friction.h's coefficient draws ("DRFRICTX")

enum { kTargetObs = 0, kTargetAct = 1 };

struct Params {
  float m, s, m_corr, s_corr;          // see the head of this file
  float clip;
  int uniform;                         // 0 gaussian, 1 uniform
  int scaling;                         // 0 additive, 1 scaling
  int use_corr;                        // 0: s_corr == 0 && m_corr == 0, zc is not drawn and corr is +0
  int active;                          // columns c < active are drawn for; the rest of the row is a pad and is copied
  uint32_t tick;
  uint64_t seed_noise, seed_corr;      // seed ^ the target's two domain constants
};

MPC_HD Params make_params(int target, uint64_t seed, int uniform, int scaling, float m, float s, float m_corr, float s_corr, float clip, int active,
                          uint32_t tick) {
  Params p;
  p.m = m; p.s = s; p.m_corr = m_corr; p.s_corr = s_corr; p.clip = clip;
  p.uniform = uniform; p.scaling = scaling;
  p.use_corr = (s_corr == 0.0f && m_corr == 0.0f) ? 0 : 1;
  p.active = active; p.tick = tick;
  p.seed_noise = seed ^ (target == kTargetAct ? kDomActNoise : kDomObsNoise);
  p.seed_corr = seed ^ (target == kTargetAct ? kDomActCorr : kDomObsCorr);
  return p;
}

// torch.clamp(y, -c, c): comparisons, so a NaN passes through (fminf / fmaxf would return the bound)
MPC_HD float clamp_nan(float y, float c) { return y < -c ? -c : (y > c ? c : y); }

MPC_HD float apply(const Params &p, float x, float d, float zc, float col_scale) {
  const float corr = zc * p.s_corr + p.m_corr;
  float term = (corr + d * p.s) + p.m;
  term = term * col_scale;
  const float y = p.scaling ? x * term : x + term;
  return clamp_nan(y, p.clip);
}

// d of columns 2 * pair and 2 * pair + 1 of environment env at p.tick
MPC_HD void noise_pair(const Params &p, uint32_t env, uint32_t pair, float &d0, float &d1) {
  if (p.uniform) {
    d0 = rltask::uniform01(p.seed_noise, env, p.tick, 2u * pair);
    d1 = rltask::uniform01(p.seed_noise, env, p.tick, 2u * pair + 1u);
  } else {
    ppo::normal_pair(p.seed_noise, env, p.tick, pair, d0, d1);
  }
}

// zc of columns 2 * pair and 2 * pair + 1 of environment env: the same on every tick
MPC_HD void corr_pair(const Params &p, uint32_t env, uint32_t pair, float &z0, float &z1) {
  z0 = z1 = 0.0f;
  if (p.use_corr) ppo::normal_pair(p.seed_corr, env, 0u, pair, z0, z1);
}

// Columns 2 * pair and 2 * pair + 1 of environment env's row: x0, x1 in, y0, y1 out.  col_scale [>= active] or null; draws null or this
// environment's [active][2] (d, zc).  A pad column is copied and never drawn for; with an odd `active` the last pair's second draw is dropped.
MPC_HD void noise_columns(const Params &p, uint32_t env, uint32_t pair, const float *col_scale, float x0, float x1, float &y0, float &y1, float *draws) {
  const int c0 = 2 * (int)pair, c1 = c0 + 1;
  y0 = x0; y1 = x1;
  if (c0 >= p.active) return;
  float d0, d1, z0, z1;
  noise_pair(p, env, pair, d0, d1);
  corr_pair(p, env, pair, z0, z1);
  y0 = apply(p, x0, d0, z0, col_scale ? col_scale[c0] : 1.0f);
  if (draws) { draws[2 * c0] = d0; draws[2 * c0 + 1] = z0; }
  if (c1 < p.active) {
    y1 = apply(p, x1, d1, z1, col_scale ? col_scale[c1] : 1.0f);
    if (draws) { draws[2 * c1] = d1; draws[2 * c1 + 1] = z1; }
  }
}

// the host statement of the kernel: rows [n][W] (W even), in may be out
inline void noise_rows(const Params &p, int n, int W, const float *col_scale, const float *in, float *out, float *draws) {
  for (int r = 0; r < n; ++r)
    for (int pr = 0; pr < W / 2; ++pr) {
      const size_t at = (size_t)r * W + 2 * (size_t)pr;
      const float x0 = in[at], x1 = in[at + 1];
      noise_columns(p, (uint32_t)r, (uint32_t)pr, col_scale, x0, x1, out[at], out[at + 1], draws ? draws + (size_t)r * p.active * 2 : nullptr);
    }
}

// legged_gym's _push_robots: torch_rand_float(-v, v) for the base's world velocity along `axis` (0 x, 1 y), in the form rl_task.h draws its
// commands in: a function of (seed, env, push index, axis) alone
MPC_HD float push_value(uint64_t seed, uint32_t env, uint32_t push_index, uint32_t axis, float v) {
  return fminf(-v + (v - (-v)) * rltask::uniform01(seed ^ kDomPush, env, push_index, axis), v);
}

}  // namespace drand
