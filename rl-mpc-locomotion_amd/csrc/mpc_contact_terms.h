/*
 * mpc_contact_terms.h -- the C ABI of the opt-in contact reward terms and of the critic's friction columns (mpc_contact_terms.hip, contact_terms.h).
 *
 * For n environments on a plant with a friction record (mpc_friction.h) the unit reads what the plant's step publishes -- each foot's ground
 * reaction and the distance it slid over the tick -- and the friction coefficients themselves.  It evaluates three more reward terms by their
 * published formulas -- feet_slip, feet_contact_forces, feet_stumble --, puts them inside the reward's clip, keeps the running float32 sum of each
 * over the episode under way with, in float64, the window accumulators (closed episodes and their term sums since the last
 * mpc_contact_new_window), and widens the critic's privileged row by sixteen columns: the coefficient, the twelve force components, three zeros.
 *
 *   mpc_contact_close    after the task's `begin`: closes the episodes of the environments `begin` has just marked (id >= 0, ticks > 0 and all
 *                        three sums finite), reduces their sums in the fixed order of episode_terms.h, adds to the window, zeroes sums and ticks
 *                        of every marked environment.  Two launches.
 *   mpc_contact_run      after the task's `finish` and, where there is one, after mpc_shaping_run: the three terms, the reward rewritten from the
 *                        task's six terms (and the shaping unit's eight), sums += terms, ticks += 1.  One launch.
 *   mpc_contact_extend   after mpc_privileged_assemble: the assembled row copied into a row sixteen columns wider, and the sixteen.  One launch.
 *
 * Stream-ordered, no host read, no atomics: a rerun from the same state is bit-identical.
 *
 * The handle is host memory until mpc_contact_bind, which puts its arrays on the sim's device.  This header lives beside the sources and not under
 * include/, like mpc_reward_shaping.h: tests/test_abi.py keeps a table of every header under include/.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_contact_last_error() gives the text.  Every argument check comes before any launch.
 */
#ifndef MPC_CONTACT_TERMS_H
#define MPC_CONTACT_TERMS_H

#include "../../include/mpc_sim.h"
#include "../../include/mpc_task.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_contact mpc_contact;

enum { MPC_CONTACT_TERMS = 3, MPC_CONTACT_SUMMARY = 5, MPC_CONTACT_COLUMNS = 16, MPC_CONTACT_SHAPING_TERMS = 8 };

/* cfg is the task's own configuration (the six reward scales and clip_observations, which clips the force columns).  scales [3] (host) are the three
 * terms' scales, each already multiplied by dt, in the order feet_slip, feet_contact_forces, feet_stumble; a scale of 0 switches its term off.
 * max_contact_force [N] is what feet_contact_forces pays above; force_scale and mu_clip shape the critic's columns; dt is the tick [s],
 * episode_length_s what the record divides by.  MPC_E_ARG, for a null pointer, n < 1, a configuration mpc_task_create would refuse, a scale that
 * is not finite, a max_contact_force that is not finite and >= 0, and a force_scale, mu_clip, dt or episode_length_s that is not finite and > 0.
 * Touches no device. */
int mpc_contact_create(mpc_contact **out, int n, const mpc_task_config *cfg, const double *scales, double max_contact_force, double force_scale,
                       double mu_clip, double dt, double episode_length_s);
void mpc_contact_destroy(mpc_contact *h);
/* keeps the addresses of the sim's friction coefficients and of the force and slip rows its step fills, and allocates the handle's own arrays on the
 * sim's device; the sim must outlive the handle's launches, hold n robots and have a friction record with both output rows (mpc_friction_attach).
 * Once per handle.  Synchronous. */
int mpc_contact_bind(mpc_contact *h, mpc_sim *s);
/* d_reset_ids [n] int32 (what `begin` wrote: r or -1) */
int mpc_contact_close(mpc_contact *h, const int *d_reset_ids, void *stream);
/* d_root [n][13], d_commands [n][3], d_torques [n][12] float32 and d_fell [n] bytes (NULL: no contacts) as `finish` read them; d_reset_ids [n] int32
 * as `begin` wrote them.  d_shaping_terms [n][8] float32 is what mpc_shaping_run has just written and shaping_scales [8] (host) the scales that unit
 * was created with; both NULL without reward shaping.  d_rew [n] float32 is rewritten; d_terms [n][3] float32 or NULL receives the tick's three
 * terms. */
int mpc_contact_run(mpc_contact *h, const float *d_root, const float *d_commands, const float *d_torques, const unsigned char *d_fell,
                    const int *d_reset_ids, const float *d_shaping_terms, const double *shaping_scales, float *d_rew, float *d_terms, void *stream);
/* d_priv [n][Wp] float32 is the assembled privileged row, Wp >= 16 a multiple of 16; d_out [n][Wp + 16] float32 receives it with the sixteen
 * columns behind it.  Both 16-byte aligned and distinct. */
int mpc_contact_extend(mpc_contact *h, const float *d_priv, int Wp, float *d_out, void *stream);
/* d_out [MPC_CONTACT_SUMMARY] float64: closed episodes in the window, the three window term sums, episode_length_s */
int mpc_contact_summary(mpc_contact *h, double *d_out, void *stream);
/* zeroes the window accumulators, stream-ordered */
int mpc_contact_new_window(mpc_contact *h, void *stream);
/* the device arrays, for tensor views: sums [n][3] float32, ticks [n] int32, window [4] float64 (the closed count and the three sums) */
int mpc_contact_arrays(mpc_contact *h, float **d_sums, int **d_ticks, double **d_window);
const char *mpc_contact_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_CONTACT_TERMS_H */
