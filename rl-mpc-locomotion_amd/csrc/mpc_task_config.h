// mpc_task_config.h -- the one reading of an mpc_task_config (include/mpc_task.h) that every unit which takes one shares: the checks of what
// they all read and the conversion to the kernels' rltask::Config (rl_task.h).  mpc_task.hip and mpc_episode_terms.hip call these and keep no
// field-by-field copy, so a new reward term or config field is added here once.  Host only.  Not part of the C ABI.
#pragma once

#include <cmath>

#include "../../include/mpc_task.h"
#include "rl_task.h"

namespace taskcfg {

inline bool finite_all(const double *v, int k) {
  for (int i = 0; i < k; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}

// The first shared check a config fails, in the order the units report them.  Each unit words its own message, and checks on its own what
// only it reads (mpc_task_create: default_dof_pos and clip_observations).
enum Fault { kOk = 0, kNotFinite, kRangeOrder, kEpisodeLength };

inline Fault check(const mpc_task_config &cfg) {
  if (!finite_all(&cfg.lin_vel_scale, 4) || !finite_all(cfg.rew_scale, MPC_TASK_REW_TERMS) || !finite_all(&cfg.command_range[0][0], 6))
    return kNotFinite;                 // a scale or a command range
  for (int a = 0; a < 3; ++a)
    if (cfg.command_range[a][0] > cfg.command_range[a][1]) return kRangeOrder;
  if (cfg.max_episode_length < 1) return kEpisodeLength;
  return kOk;
}

// the kernels' float32 view of the config: every double rounded once, here
inline rltask::Config to_device_config(const mpc_task_config &cfg) {
  static_assert(MPC_TASK_REW_TERMS == rltask::kRewTerms, "include/mpc_task.h and rl_task.h disagree");
  rltask::Config c{};
  c.lin_vel_scale = (float)cfg.lin_vel_scale; c.ang_vel_scale = (float)cfg.ang_vel_scale;
  c.dof_pos_scale = (float)cfg.dof_pos_scale; c.dof_vel_scale = (float)cfg.dof_vel_scale;
  for (int i = 0; i < rltask::kRewTerms; ++i) c.rew[i] = (float)cfg.rew_scale[i];
  for (int a = 0; a < 3; ++a) { c.cmd_lo[a] = (float)cfg.command_range[a][0]; c.cmd_hi[a] = (float)cfg.command_range[a][1]; }
  c.clip_obs = (float)cfg.clip_observations;
  for (int i = 0; i < 12; ++i) c.default_dof_pos[i] = (float)cfg.default_dof_pos[i];
  c.max_episode_length = cfg.max_episode_length;
  c.seed = cfg.seed;
  return c;
}

}  // namespace taskcfg
