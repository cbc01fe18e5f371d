// terrain_curriculum.h -- the per-environment arithmetic of the terrain curriculum, shared by the device kernel (mpc_curriculum.hip,
// mpc_curriculum.h) and host C++ (the CPU tests compile this header with g++ and compare it with tests/curriculum_ref.py).
//
// What it restates: legged_gym's `_update_terrain_curriculum` by its published algorithm (legged_gym is not a dependency and nothing is checked
// against it).  For an environment that is about to be reset:
//   distance  = norm(root_states[:2] - env_origin[:2])               here the robot's coordinates are LOCAL: root_state[0], [1] is that difference
//   move_up   = distance > env_length / 2
//   move_down = (distance < norm(commands[:2]) * max_episode_length_s * 0.5) * ~move_up
//   level    += move_up - move_down
//   level     = level >= max_level ? randint(max_level) : clip(level, 0)
//   origin    = tile_origins[level][type]
// float32, in that operation order; compile with -ffp-contract=off.  The commands are the finished episode's (the caller runs this before the
// task's `begin` redraws them).
//
// Like legged_gym, `move_down` uses the CONFIGURED episode length, not the length the episode had: a robot that falls early has walked less than
// half of what its command asked of a whole episode and is demoted.
//
// One departure: a distance that is not finite (a NaN or infinite position, or squares that overflow float32) makes BOTH comparisons false and the
// robot keeps its level.  torch's `inf > env_length / 2` is true and would promote a robot whose state blew up; NaN compares false there too.
//
// The redraw is not torch's generator: rl_task.h's counter-based uniform01 keyed by (seed, env, k, kLevelAxis), k being the curriculum's own count
// of this environment's resets, so the draw does not depend on which other environments reset with it.  Parity with `randint_like` is in
// distribution only: uniform on 0 .. max_level - 1.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rl_task.h"

namespace curriculum {

constexpr uint32_t kLevelAxis = 3;     // uniform01's axis tag of the level redraw: sample_commands uses 0, 1, 2

struct Config {
  int num_levels, num_types;           // max_level = num_levels
  float half_len;                      // float32(env_length / 2)
  float episode_length_s;              // float32(episode_length_s)
  unsigned long long seed;
};

// the redraw: uniform on 0 .. max_level - 1, a function of (seed, env, k) alone
MPC_HD int draw_level(unsigned long long seed, int env, int k, int max_level) {
  const float u = rltask::uniform01(seed, (uint32_t)env, (uint32_t)k, kLevelAxis);
  const int l = (int)(u * (float)max_level);
  return l < max_level - 1 ? l : max_level - 1;
}

// +1 (promoted), -1 (demoted) or 0 for the position xy [2] (local: the distance from the origin) and the finished episode's commands [2]
MPC_HD int decide(const Config &c, const float *xy, const float *commands) {
  const float d = sqrtf(xy[0] * xy[0] + xy[1] * xy[1]);
  const bool finite = d <= 3.402823466e+38f;                             // false for NaN and +inf
  const bool up = finite && d > c.half_len;
  const bool down = finite && (d < (sqrtf(commands[0] * commands[0] + commands[1] * commands[1]) * c.episode_length_s) * 0.5f) && !up;
  return (up ? 1 : 0) - (down ? 1 : 0);
}

// One environment whose reset flag is set: the new level, the counter and the new origin [2].  tile_origins [num_levels][num_types][2].
// Returns the decision (+1, -1, 0) for the tests.
MPC_HD int update_env(const Config &c, int env, const float *xy, const float *commands, int type, const double *tile_origins, int &level, int &count,
                      double *origin) {
  const int move = decide(c, xy, commands);
  count += 1;
  int l = level + move;
  l = l >= c.num_levels ? draw_level(c.seed, env, count, c.num_levels) : (l > 0 ? l : 0);
  level = l;
  const double *o = tile_origins + ((size_t)l * (size_t)c.num_types + (size_t)type) * 2;
  origin[0] = o[0];
  origin[1] = o[1];
  return move;
}

}  // namespace curriculum
