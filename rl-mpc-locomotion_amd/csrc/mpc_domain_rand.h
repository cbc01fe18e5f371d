/*
 * mpc_domain_rand.h -- the C ABI of the opt-in domain randomisation (mpc_domain_rand.hip, domain_rand.h): noise on the observations and on
 * the actions in the form of the reference's VecTask.apply_randomizations, and legged_gym's random pushes of the base.
 *
 * mpc_drand_noise is one kernel on a row-major float32 matrix [n][W]: out = clamp(x (+ | *) term, -clip, clip) with
 * term = ((zc * s_corr + m_corr) + d * s + m) * col_scale for the columns below `active`, a copy for the rest (the height scan's pad).
 * d is drawn per (seed, environment, tick, column), zc per (seed, environment, column): counter-based draws, no device state, nothing
 * depends on n or W.  mpc_drand_push is one kernel with one lane per robot of the bound sim.  Both are stream-ordered; no host read, no
 * atomics, no LDS.  The schedule of the reference (linear / constant, frequency) is the caller's: the ABI takes the scheduled values.
 *
 * This header lives beside the sources and not under include/, like mpc_height_scan.h.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_drand_last_error() gives the text.
 */
#ifndef MPC_DOMAIN_RAND_H
#define MPC_DOMAIN_RAND_H

#include "../../include/mpc_terrain.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_DRAND_OBSERVATIONS = 0, MPC_DRAND_ACTIONS = 1 };        /* target: which pair of draw domains */
enum { MPC_DRAND_GAUSSIAN = 0, MPC_DRAND_UNIFORM = 1 };            /* distribution */
enum { MPC_DRAND_ADDITIVE = 0, MPC_DRAND_SCALING = 1 };            /* operation */

typedef struct mpc_drand mpc_drand;

/* n environments, the seed of every draw.  MPC_E_ARG, before the device is touched, for a null pointer or n < 1. */
int mpc_drand_create(mpc_drand **out, int n, unsigned long long seed);
void mpc_drand_destroy(mpc_drand *h);
/* Keep the device addresses of s's state record (the pushes write it).  MPC_E_ARG for a sim of another size or on another device. */
int mpc_drand_bind(mpc_drand *h, mpc_sim *s);
/* d_in, d_out [n][W] float32, 8-byte aligned, W even, n * W / 2 below 2^31; d_in may be d_out.  0 <= active <= W.  m, s, m_corr, s_corr are
 * rounded to float32 (gaussian: mu, var, mu_corr, var_corr; uniform: lo, hi - lo, lo_corr, hi_corr - lo_corr) and must be finite; clip must
 * be >= 0 (it may be +inf).  d_col_scale [W] float32 or NULL (1).  d_draws [n][active][2] float32 or NULL: (d, zc) of every drawn column.
 * tick in 0 .. 2^32 - 1.  When s_corr and m_corr are both 0 as float32, zc is not drawn (and written as 0). */
int mpc_drand_noise(mpc_drand *h, int target, int distribution, int operation, double m, double s, double m_corr, double s_corr, double clip,
                    const float *d_col_scale, const float *d_in, float *d_out, int W, int active, long long tick, float *d_draws, void *stream);
/* For every robot of the bound sim that has not fallen: world x, y velocity = uniform in [-max_vel, max_vel], written as a double into the
 * sim's state and as the float32 into d_root [n][13] columns 7, 8.  max_vel finite and >= 0, push_index in 0 .. 2^32 - 1. */
int mpc_drand_push(mpc_drand *h, float *d_root, double max_vel, long long push_index, void *stream);
const char *mpc_drand_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_DOMAIN_RAND_H */
