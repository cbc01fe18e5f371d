/*
 * mpc_reward_shaping.h -- the C ABI of the opt-in reward shaping terms (mpc_reward_shaping.hip, reward_shaping.h).
 *
 * For n environments the unit evaluates eight more reward terms by legged_gym's published formulas -- orientation, base_height, dof_vel,
 * dof_acc, action_rate, feet_air_time, stand_still, termination --, adds them to the task's six and rewrites the reward, and keeps the running
 * float32 sum of each of the eight over the episode under way with, in float64, the window accumulators (closed episodes and their term sums
 * since the last mpc_shaping_new_window).  Per environment it holds the history the terms read: the last actions and joint velocities, the
 * feet's air time and last contact flags.
 *
 *   mpc_shaping_close   after the task's `begin`: closes the episodes of the environments `begin` has just marked (id >= 0, ticks > 0 and all
 *                       eight sums finite), reduces their sums in the fixed order of episode_terms.h, adds to the window, zeroes sums and ticks
 *                       of every marked environment.  Two launches.
 *   mpc_shaping_run     after the task's `finish` (and the height scan), on the tensors `finish` read and wrote: the eight terms, the reward,
 *                       the history, sums += terms, ticks += 1.  One launch.
 *
 * Stream-ordered, no host read, no atomics: a rerun from the same state is bit-identical.
 *
 * This header lives beside the sources and not under include/, like mpc_episode_terms.h: tests/test_abi.py keeps a table of every header under
 * include/.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_shaping_last_error() gives the text.  Every argument check comes before any launch.
 */
#ifndef MPC_REWARD_SHAPING_H
#define MPC_REWARD_SHAPING_H

#include "../../include/mpc_sim.h"
#include "../../include/mpc_task.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_shaping mpc_shaping;

enum { MPC_SHAPING_TERMS = 8, MPC_SHAPING_SUMMARY = 10, MPC_SHAPING_MAX_POINTS = 208 };

/* cfg is the task's own configuration (the six reward scales, default_dof_pos, max_episode_length).  scales [8] (host) are the eight terms'
 * scales, each already multiplied by dt, in the order orientation, base_height, dof_vel, dof_acc, action_rate, feet_air_time, stand_still,
 * termination; a scale of 0 switches its term off.  dt is the tick [s], episode_length_s what the record divides by.  MPC_E_ARG, before the
 * device is touched, for a null pointer, n < 1, a configuration mpc_task_create would refuse, a default_dof_pos, scale or target that is not
 * finite, air_time_target < 0, and a dt or episode_length_s that is not finite and > 0.  Synchronous. */
int mpc_shaping_create(mpc_shaping **out, int n, const mpc_task_config *cfg, const double *scales, double base_height_target, double air_time_target,
                       double dt, double episode_length_s);
void mpc_shaping_destroy(mpc_shaping *h);
/* keeps the address of the sim's int32 state record, whose first four words per robot are the foot-contact flags; the sim must outlive the
 * handle's launches and hold n robots */
int mpc_shaping_bind(mpc_shaping *h, mpc_sim *s);
/* d_reset_ids [n] int32 (what `begin` wrote: r or -1) */
int mpc_shaping_close(mpc_shaping *h, const int *d_reset_ids, void *stream);
/* d_root [n][13], d_dof [n][12][2], d_actions [n][12], d_commands [n][3], d_torques [n][12] float32 and d_fell [n] bytes (NULL: no contacts) as
 * `finish` read them; d_reset_ids [n] int32 as `begin` wrote them; d_reset, d_progress [n] int64 as `finish` left them; d_heights [n][P] float32
 * the measured heights in metres, 1 <= P <= 208, or NULL with P = 0; d_rew [n] float32 is rewritten; d_terms [n][8] float32 or NULL receives the
 * tick's eight terms. */
int mpc_shaping_run(mpc_shaping *h, const float *d_root, const float *d_dof, const float *d_actions, const float *d_commands, const float *d_torques,
                    const unsigned char *d_fell, const int *d_reset_ids, const long long *d_reset, const long long *d_progress, const float *d_heights,
                    int P, float *d_rew, float *d_terms, void *stream);
/* d_out [MPC_SHAPING_SUMMARY] float64: closed episodes in the window, the eight window term sums, episode_length_s */
int mpc_shaping_summary(mpc_shaping *h, double *d_out, void *stream);
/* zeroes the window accumulators, stream-ordered */
int mpc_shaping_new_window(mpc_shaping *h, void *stream);
/* the device arrays, for tensor views: last_actions [n][12], last_dof_vel [n][12], air_time [n][4] float32, last_contact [n][4] int32, sums [n][8]
 * float32, ticks [n] int32, window [9] float64 (the closed count and the eight sums) */
int mpc_shaping_arrays(mpc_shaping *h, float **d_last_actions, float **d_last_dof_vel, float **d_air_time, int **d_last_contact, float **d_sums,
                       int **d_ticks, double **d_window);
const char *mpc_shaping_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_REWARD_SHAPING_H */
