/*
 * mpc_height_scan.h -- the C ABI of the terrain height scan (mpc_height_scan.hip, height_scan.h): legged_gym's measured heights as extra
 * observation columns.
 *
 * A scan holds P sample points in the base's yaw frame.  mpc_hscan_run takes the root states [n][13] and an observation buffer [n][in_width]
 * and writes a WIDE row per environment: the in_width columns copied, then the P scan values, then zeros up to the next multiple of 16
 * (mpc_policy_create and mpc_ac_create take layer input widths that are multiples of 16).  One kernel, one launch; the whole wide row is
 * written on every call, the pad included.  It reads the bound sim's height field and its origin array as they are on the stream at that
 * moment, so an origin the terrain curriculum has just rewritten is seen in the same tick.  Stream-ordered, no host read, no atomics.
 *
 * This header lives beside the sources and not under include/, like mpc_curriculum.h: tests/test_abi.py keeps a table of every header under
 * include/, and that table is fixed.
 *
 * Pointers named d_* are DEVICE pointers, h_* HOST pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_*
 * code of include/mpc_batch.h; mpc_hscan_last_error() gives the text.
 */
#ifndef MPC_HEIGHT_SCAN_H
#define MPC_HEIGHT_SCAN_H

#include "../../include/mpc_terrain.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_HSCAN_MAX_POINTS = 208 };   /* the largest P whose padded row beside 48 columns still fits MPC_OBSNORM_MAX_OBS = 256 */

typedef struct mpc_hscan mpc_hscan;

/* h_points [P][2] float32, in metres in the base's yaw frame.  offset, clip, scale: the column is clip(root_z - offset - h, -clip, clip) * scale
 * (legged_gym: 0.5, 1.0, 5.0), then clipped to +-obs_clip (the task's clip_observations).  MPC_E_ARG, before the device is touched, for a null
 * pointer, n < 1, P outside 1 .. MPC_HSCAN_MAX_POINTS, a point or a scalar that is not finite, or a clip or obs_clip below 0.  Synchronous. */
int mpc_hscan_create(mpc_hscan **out, int n, int P, const float *h_points, double offset, double clip, double scale, double obs_clip);
void mpc_hscan_destroy(mpc_hscan *h);
/* Keep s's height field, its scales, (x0, y0) and the device address of its origin array.  MPC_E_ARG for a sim without a terrain, of another
 * size or on another device.  A sim whose terrain is attached again has new arrays: bind again. */
int mpc_hscan_bind(mpc_hscan *h, mpc_sim *s);
/* d_root [n][13] float32, d_obs_in [n][in_width] float32 (may be NULL when in_width is 0), d_obs_out [n][mpc_hscan_width(in_width, P)] float32,
 * d_heights [n][P] float32 or NULL (the measured heights in metres).  d_obs_out must not be d_obs_in.  MPC_E_ARG for in_width < 0 or a width
 * mpc_hscan_width refuses, or without a bound sim. */
int mpc_hscan_run(mpc_hscan *h, const float *d_root, const float *d_obs_in, int in_width, float *d_obs_out, float *d_heights, void *stream);
/* roundup16(in_width + P), or MPC_E_ARG for in_width outside 0 .. 65536 or P outside 1 .. MPC_HSCAN_MAX_POINTS */
int mpc_hscan_width(int in_width, int P);
const char *mpc_hscan_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_HEIGHT_SCAN_H */
