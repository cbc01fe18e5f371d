// height_scan.h -- the per-(environment, point) arithmetic of the terrain height scan, shared by the device kernel (mpc_height_scan.hip,
// mpc_height_scan.h) and host C++ (the CPU tests compile this header with g++ and compare it with tests/height_scan_ref.py).
//
// What it restates: legged_gym's height measurements by their published algorithm (`_init_height_points`, `_get_heights`, `quat_apply_yaw`, and
// Isaac Gym's `quat_apply` and `normalize`; legged_gym is not a dependency and nothing is checked against it).  For environment r and point p:
//   points[p]  = (x[i], y[j]), p = i * len(y) + j                       meshgrid(x, y) flattened, x the outer index; float32 [P][2]
//   q          = root quaternion (xyzw) with x = y = 0, divided by max(sqrtf(z^2 + w^2), 1e-9f)          quat_apply_yaw's normalize
//   t          = 2 * (q.xyz x b),  b = (px, py, 0)                       quat_apply
//   rot        = b + q.w * t + q.xyz x t
//   world      = rot.xy + root.xy                                        the float32 sum, as legged_gym forms it
//   (i, j)     = toysim::terrain_index(world + origin[r])                the plant's own index: float64, clamped BEFORE the integer conversion
//   h          = float(min(H[i][j], H[i+1][j], H[i][j+1])) * float(vscale)      the minimum on the int16 values
//   obs        = clamp(clamp(((root.z - offset) - h), -clip, clip) * scale, -obs_clip, obs_clip)
// float32 in that operation order (the index alone is float64); compile with -ffp-contract=off.  The last clamp is the task's own
// clip_observations, as rl_task.h's observe applies it to its 48 columns.
//
// On the field the index is legged_gym's `(points + border_size) / horizontal_scale -> .long() -> clip(0, shape - 2)`: the truncation of a
// non-negative quotient, with x0 = -border_size.  Departures, all on inputs legged_gym leaves undefined or handles by accident:
//   * a NaN or infinite position or quaternion: torch's cast of such a value to an integer is undefined.  Here terrain_index clamps in floating
//     point first, as include/mpc_terrain.h states for the plant: NaN, -inf and every negative quotient land on cell 0, +inf and everything past the
//     last node on cell count - 2, so no lookup leaves the field whatever the input.
//   * a quotient in (-1, 0) truncates to 0 in torch too; below -1 torch's clip gives 0 as well, so negative finite values agree.
//   * the clamps are rl_task.h's clampf (fminf / fmaxf): a NaN root height gives -clip * scale where torch.clip would keep the NaN, like the
//     task's own columns.
//   * legged_gym measures BEFORE reset_idx, so an environment that has just been reset carries the old pose's heights against the new pose's
//     root height for one tick.  Here the scan runs after the reset and reads the same post-reset root state `finish` reads.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rl_task.h"
#include "toy_sim.h"

namespace hscan {

constexpr int kMaxPoints = 208;        // the largest P with roundup16(48 + P) <= 256 columns (MPC_OBSNORM_MAX_OBS)
constexpr float kNormEps = 1e-9f;      // Isaac Gym's normalize(eps=1e-9)

struct Config {
  float offset, clip, scale;           // legged_gym: 0.5, 1.0, obs_scales.height_measurements = 5.0
  float obs_clip;                      // the task's clip_observations
};

// the plant's height field (toysim::HeightField without the per-robot origin)
struct Field {
  const short *h;                      // [rows][cols]
  int rows, cols;
  double hscale, vscale, x0, y0;
};

MPC_HD int roundup16(int w) { return (w + 15) & ~15; }

// a x b, float32, Isaac Gym's torch.cross component order
MPC_HD void cross3(const float *a, const float *b, float *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// quat_apply_yaw(quat, (px, py, 0)): out [2], the rotated point's x and y (its z is 0 up to rounding and is not used)
MPC_HD void yaw_rotate(const float *quat, float px, float py, float *out) {
  const float z = quat[2], w = quat[3];
  const float nrm = fmaxf(sqrtf(z * z + w * w), kNormEps);
  const float a[3] = {0.0f, 0.0f, z / nrm};
  const float aw = w / nrm;
  const float b[3] = {px, py, 0.0f};
  float t[3], c[3];
  cross3(a, b, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = t[i] * 2.0f;
  cross3(a, t, c);
  out[0] = (b[0] + aw * t[0]) + c[0];
  out[1] = (b[1] + aw * t[1]) + c[1];
}

// the cell (i, j) under point (px, py) of a base at root [13] (position, xyzw quaternion, ...) standing at local + origin [2]
MPC_HD void cell_of(const Field &f, const float *root, const double *origin, float px, float py, int &i, int &j) {
  float rot[2];
  yaw_rotate(root + 3, px, py, rot);
  const float wx = rot[0] + root[0], wy = rot[1] + root[1];
  double frac;
  toysim::terrain_index((double)wx, origin[0], f.x0, f.hscale, f.rows, i, frac);
  toysim::terrain_index((double)wy, origin[1], f.y0, f.hscale, f.cols, j, frac);
}

// the measured height [m] of cell (i, j): 0 <= i <= rows - 2, 0 <= j <= cols - 2
MPC_HD float height_of(const Field &f, int i, int j) {
  const short *c = f.h + (size_t)i * (size_t)f.cols + (size_t)j;
  short m = c[0];
  const short h2 = c[f.cols], h3 = c[1];
  m = h2 < m ? h2 : m;
  m = h3 < m ? h3 : m;
  return (float)m * (float)f.vscale;
}

// the observation column of a measured height
MPC_HD float observe(const Config &c, float root_z, float h) {
  return rltask::clampf(rltask::clampf((root_z - c.offset) - h, c.clip) * c.scale, c.obs_clip);
}

// one (environment, point): the measured height and its observation
MPC_HD void scan_point(const Config &c, const Field &f, const float *root, const double *origin, const float *point, float &height, float &obs) {
  int i, j;
  cell_of(f, root, origin, point[0], point[1], i, j);
  height = height_of(f, i, j);
  obs = observe(c, root[2], height);
}

}  // namespace hscan
