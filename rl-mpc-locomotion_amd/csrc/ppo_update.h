// ppo_update.h -- the scalar arithmetic of the update half of a PPO iteration, shared by the device kernels (mpc_ppo_update.hip,
// include/mpc_ppo_update.h) and host C++ (the CPU tests compile this header with g++ and compare it with float64 autograd and torch.optim.Adam,
// tests/test_ppo_update.py).  It restates rsl_rl v1.0.2's PPO.update as ppo.PPO.losses / update write it:
//   head_row        one row of the mini-batch: log-prob, ratio, clipped surrogate, clipped (or plain) value loss, kl; and the row's share of the
//                   gradient of  loss = surrogate + value_loss_coef * value_loss - entropy_coef * entropy  (means over the B rows of the mini-batch)
//                   with respect to the actor's mean, the critic's value and std
//   entropy_row     Normal.entropy summed over the actions (the same for every row: std does not depend on the observation)
//   bc_element      one element of the behaviour-cloning loss of policy distillation (mse or huber) and its gradient
//   adapt_lr        PPO.adapt_learning_rate on a float64 learning rate
//   adam_element    one element of torch.optim.Adam's step (no weight decay, no amsgrad), behind clip_grad_norm_'s multiplication
// float32 in rsl_rl's / torch's operation order; compile with -ffp-contract=off.
//
// The gradient of a max: torch.max(a, b) gives its incoming gradient to the larger argument and half to each where they are equal.  In the interior of
// the ratio clip both arguments are the same number and both derivatives are -A, so the halves add up to the unclipped derivative; outside it the clamp's
// derivative is zero.  The value clip is the same with one difference: v_old + (V - v_old) is V only up to a rounding, so torch's choice of the branch
// in the interior is a draw of that rounding while both derivatives are 2 (V - R) up to the same rounding; this header takes the unclipped derivative
// there.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ppo_rollout.h"

namespace ppo {

constexpr float kEntropyConst = 1.4189385332046727f;   // 0.5 + 0.5 * math.log(2 * math.pi) of Normal.entropy, as the float32 it becomes

struct HeadCfg {
  float clip;              // clip_param
  float value_coef;        // value_loss_coef
  float entropy_coef;
  int clipped_value;       // use_clipped_value_loss
  float inv_rows;          // 1 / B
};

struct HeadRow {
  float surrogate, value_loss, kl;       // this row's terms (their means over the rows are the loss terms)
  float dmu[kActions];                   // d loss / d mu of this row
  float dv;                              // d loss / d V of this row
  float dstd[kActions];                  // this row's share of d loss / d std through the log-prob (the entropy's share is entropy_dstd)
};

// one term of the kl of two diagonal normals as rsl_rl writes it: log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mu)^2) / (2 sigma^2) - 0.5
MPC_HD float kl_term(float mu, float sigma, float old_mu, float old_sigma) {
  const float d = old_mu - mu;
  return (logf(sigma / old_sigma + 1.e-5f) + (old_sigma * old_sigma + d * d) / (2.0f * (sigma * sigma))) - 0.5f;
}

MPC_HD float entropy_row(const float *std) {
  float s = kEntropyConst + logf(std[0]);
#pragma unroll
  for (int k = 1; k < kActions; ++k) s = s + (kEntropyConst + logf(std[k]));
  return s;
}

// d(-entropy_coef * mean entropy) / d std[k]
MPC_HD float entropy_dstd(float entropy_coef, float std_k) { return -entropy_coef / std_k; }

MPC_HD void head_row(const HeadCfg &c, const float *mu, float V, const float *std, const float *actions, float old_value, float adv, float ret,
                     float old_logp, const float *old_mu, const float *old_sigma, HeadRow &o) {
  float terms[kActions];
  float kl = 0.0f;
#pragma unroll
  for (int k = 0; k < kActions; ++k) {
    terms[k] = log_prob_term(actions[k], mu[k], std[k]);
    const float t = kl_term(mu[k], std[k], old_mu[k], old_sigma[k]);
    kl = k == 0 ? t : kl + t;
  }
  o.kl = kl;
  const float logp = log_prob_sum(terms);
  const float ratio = expf(logp - old_logp);
  const float na = -adv;
  const float s1 = na * ratio;
  const float s2 = na * fminf(fmaxf(ratio, 1.0f - c.clip), 1.0f + c.clip);
  o.surrogate = fmaxf(s1, s2);
  // s1 > s2: the unclipped branch; s1 == s2: the interior of the clip (halves of the same derivative) or A = 0; s1 < s2: clipped, no gradient
  const float dratio = s1 >= s2 ? na : 0.0f;
  const float dlogp = (dratio * ratio) * c.inv_rows;
#pragma unroll
  for (int k = 0; k < kActions; ++k) {
    const float d = actions[k] - mu[k];
    const float var = std[k] * std[k];
    o.dmu[k] = dlogp * (d / var);
    o.dstd[k] = dlogp * ((d * d) / (var * std[k]) - 1.0f / std[k]);
  }
  float dvl;
  if (c.clipped_value) {
    const float dv = V - old_value;
    const float clipped = old_value + fminf(fmaxf(dv, -c.clip), c.clip);
    const float e1 = V - ret, e2 = clipped - ret;
    const float t1 = e1 * e1, t2 = e2 * e2;
    o.value_loss = fmaxf(t1, t2);
    if (dv >= -c.clip && dv <= c.clip) dvl = 2.0f * e1;             // the interior: both branches are the unclipped one
    else dvl = t1 > t2 ? 2.0f * e1 : (t1 == t2 ? e1 : 0.0f);        // outside the clamp passes no gradient: only the unclipped branch has one
  } else {
    const float e = ret - V;
    o.value_loss = e * e;
    dvl = -2.0f * e;
  }
  o.dv = (c.value_coef * dvl) * c.inv_rows;
}

// ---- behaviour cloning (policy distillation): one element of torch.nn.functional.mse_loss / huber_loss (delta = 1) with mean reduction over the
// 12 B elements of a mini-batch, d = mu - target.  `value` is the element's term of the sum the mean is taken of; `grad` is d loss / d mu as
// torch's backward kernels write it: norm * d with norm = 2 / (12 B) for mse, norm * clamp(d, -1, 1) with norm = 1 / (12 B) for huber, norm the
// float32 value of the float64 quotient.
enum { kBcMse = 0, kBcHuber = 1 };

MPC_HD float bc_norm(int loss_type, int rows) { return (float)((loss_type == kBcMse ? 2.0 : 1.0) / (double)((long long)kActions * rows)); }

MPC_HD void bc_element(int loss_type, float norm, float mu, float target, float &value, float &grad, float &gap) {
  const float d = mu - target;
  gap = fabsf(d);
  if (loss_type == kBcMse) {
    value = d * d;
    grad = norm * d;
  } else {
    value = gap < 1.0f ? (0.5f * d) * d : gap - 0.5f;
    grad = d < -1.0f ? -norm : (d > 1.0f ? norm : norm * d);
  }
}

// PPO.adapt_learning_rate: lr / 1.5 (not below 1e-5) if kl > 2 desired_kl, lr * 1.5 (not above 1e-2) if 0 < kl < desired_kl / 2
MPC_HD double adapt_lr(double lr, double kl_mean, double desired_kl) {
  if (kl_mean > desired_kl * 2.0) return fmax(1e-5, lr / 1.5);
  if (kl_mean < desired_kl / 2.0 && kl_mean > 0.0) return fmin(1e-2, lr * 1.5);
  return lr;
}

// clip_grad_norm_'s coefficient: clamp(max_norm / (total_norm + 1e-6), max = 1), float32 as torch computes it on the norm tensor
MPC_HD float clip_coef(float total_norm, float max_norm) { return fminf(max_norm / (total_norm + 1.e-6f), 1.0f); }

struct AdamCfg {
  double beta1, beta2, eps;     // Python floats
  double bias_correction1;       // 1 - beta1 ** step
  double bias_correction2_sqrt;  // (1 - beta2 ** step) ** 0.5
};

// torch.optim.Adam's single-tensor step on one element, after grad.mul_(coef):
//   exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); param.addcdiv_(exp_avg, denom, value=-(lr / bias_correction1))
// The scalars are Python floats (float64) that enter a float32 kernel as their float32 values.
MPC_HD void adam_element(const AdamCfg &c, double lr, float coef, float &p, float &g, float &m, float &v) {
  g = g * coef;
  const float w = (float)(1.0 - c.beta1);
  m = m + w * (g - m);                                             // lerp with weight < 0.5
  v = v * (float)c.beta2 + ((float)(1.0 - c.beta2) * g) * g;
  const float denom = sqrtf(v) / (float)c.bias_correction2_sqrt + (float)c.eps;
  const float step_size = (float)(-(lr / c.bias_correction1));
  p = p + step_size * (m / denom);
}

}  // namespace ppo
