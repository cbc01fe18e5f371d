/*
 * mpc_episode_terms.h -- the C ABI of the per-term episode reward sums and the command curriculum they drive (mpc_episode_terms.hip,
 * episode_terms.h).
 *
 * For n environments the unit keeps the running float32 sum of each of the task's six reward terms over the episode under way (legged_gym's
 * episode_sums), the ticks held in those sums and a count of resamples; on the device, in float64, the three command ranges, the window
 * accumulators (closed episodes and their term sums since the last mpc_episode_terms_new_window) and a widenings counter.
 *
 *   mpc_episode_terms_close_and_resample   straight after the task's `begin`: closes the episodes of the environments `begin` has just marked
 *                                          (id >= 0, ticks > 0 and all six sums finite), reduces their sums in the fixed order of episode_terms.h, decides whether the x
 *                                          command range widens, adds to the window, zeroes sums and ticks of every marked environment, and --
 *                                          with a curriculum -- draws its commands afresh from the updated ranges.  Three launches with a
 *                                          curriculum, two without.
 *   mpc_episode_terms_accumulate           after the task's `finish`, on the tensors `finish` read: sums += terms, ticks += 1.  One launch.
 *
 * Stream-ordered, no host read, no atomics: a rerun from the same state is bit-identical.  Environments that are not marked are neither read
 * (beyond their id) nor written by close_and_resample.
 *
 * This header lives beside the sources and not under include/, like mpc_curriculum.h: tests/test_abi.py keeps a table of every header under
 * include/.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_episode_terms_last_error() gives the text.  Every argument check comes before any launch.
 */
#ifndef MPC_EPISODE_TERMS_H
#define MPC_EPISODE_TERMS_H

#include "../../include/mpc_task.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_episode_terms mpc_episode_terms;

enum { MPC_EPISODE_TERMS_SUMMARY = 11, MPC_EPISODE_TERMS_STATE = 14 };

/* cfg is the task's own configuration (the scales, the six reward scales, the three command ranges, max_episode_length, the seed);
 * episode_length_s is what the record divides by (legged_gym's max_episode_length_s).  curriculum 0: no command curriculum, the remaining
 * arguments are ignored and the commands are never written.  curriculum 1: the x range starts at (x_lo0, x_hi0) and widens by `step` on either
 * side, inside +-max_curriculum, when the closed episodes' mean lin_vel_xy sum per tick exceeds threshold x the term's scale, on ticks that are
 * multiples of update_every.  MPC_E_ARG, before the device is touched, for a null pointer, n < 1, a configuration mpc_task_create would refuse,
 * an episode_length_s that is not finite and > 0, and with a curriculum: x_lo0 <= 0 <= x_hi0 violated, max_curriculum below max(|x_lo0|, |x_hi0|)
 * or not finite, step not finite and > 0, threshold not finite, update_every < 1.  Synchronous. */
int mpc_episode_terms_create(mpc_episode_terms **out, int n, const mpc_task_config *cfg, double episode_length_s, int curriculum, double x_lo0,
                             double x_hi0, double step, double threshold, double max_curriculum, long long update_every);
void mpc_episode_terms_destroy(mpc_episode_terms *h);
/* d_reset_ids [n] int32 (what `begin` wrote: r or -1), d_commands [n][3] float32 (written for marked environments, with a curriculum only; may be
 * NULL without one), tick >= 0 the caller's count of ticks, curriculum_enabled 0 to skip the decision (an evaluation run). */
int mpc_episode_terms_close_and_resample(mpc_episode_terms *h, const int *d_reset_ids, float *d_commands, long long tick, int curriculum_enabled,
                                         void *stream);
/* d_root [n][13], d_commands [n][3], d_torques [n][12] float32 and d_fell [n] bytes (NULL: no contacts) as `finish` read them; d_terms [n][6]
 * float32 or NULL receives the tick's six terms. */
int mpc_episode_terms_accumulate(mpc_episode_terms *h, const float *d_root, const float *d_commands, const float *d_torques,
                                 const unsigned char *d_fell, float *d_terms, void *stream);
/* d_out [MPC_EPISODE_TERMS_SUMMARY] float64: closed episodes in the window, the six window term sums, x lo, x hi, widenings,
 * episode_length_s */
int mpc_episode_terms_summary(mpc_episode_terms *h, double *d_out, void *stream);
/* zeroes the window accumulators, stream-ordered */
int mpc_episode_terms_new_window(mpc_episode_terms *h, void *stream);
/* the device arrays, for tensor views: sums [n][6] float32, ticks [n] int32, counts [n] int32, state [MPC_EPISODE_TERMS_STATE] float64 (the
 * ranges [3][2], the window's closed count and six sums, the widenings) */
int mpc_episode_terms_arrays(mpc_episode_terms *h, float **d_sums, int **d_ticks, int **d_counts, double **d_state);
const char *mpc_episode_terms_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_EPISODE_TERMS_H */
