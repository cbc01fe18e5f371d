/*
 * include/mpc_ppo_update.h -- C ABI of the update half of a PPO iteration (rsl_rl v1.0.2's PPO.update, as rl_mpc_locomotion_amd.ppo.PPO.losses /
 * update state it) on the device: for one mini-batch after another on one stream, with no host synchronisation, no atomics and no graph capture.
 *
 *   mpc_ppo_update_grads   forward of both nets over the rows named by an index slice (read straight from the rollout storage), the loss head, the
 *                          backward pass: the gradient of  surrogate + value_loss_coef * value_loss - entropy_coef * entropy  into the bound .grad
 *                          tensors, the four loss terms, and the adaptive schedule's decision applied to a float64 learning rate on the device
 *   mpc_ppo_update_apply   the total gradient norm, clip_grad_norm_'s coefficient and torch.optim.Adam's step over all parameter tensors, the
 *                          learning rate read from the device
 *   mpc_ppo_update_grads_sequence   the same for a recurrent actor-critic, whose nets read dense rows that two memories wrote: it also writes
 *                          d loss / d rows for the memories' backward pass, and mpc_ppo_update_bind_extra puts the memories' parameters behind the
 *                          mpc_ac's in mpc_ppo_update_apply (the end of this file)
 *   mpc_ppo_update_grads_distill / mpc_ppo_update_apply_actor   policy distillation: the actor alone, a behaviour-cloning loss against a teacher's
 *                          actions (mpc_ppo_update_set_distill_targets), and the clip and Adam over the actor's tensors alone (the end of this file)
 *
 * The GEMMs run on the exact-fp32 MFMA pipe (rl-mpc-locomotion_amd/csrc/ppo_gemm.h); the scalar arithmetic is csrc/ppo_update.h, float32 in
 * rsl_rl's and torch's operation order.  Every sum over rows or elements is taken in a fixed order: a rerun is bit-identical.
 *
 * Nothing is copied: the parameters are read and written at the addresses the mpc_ac holds (mpc_ac_bind), so mpc_ac_act sees an update at once; the
 * gradients and Adam's moments are the caller's tensors (mpc_ppo_update_bind), so torch's optimizer.state_dict() stays the checkpoint.
 *
 * All pointers named d_* are DEVICE pointers; `stream` is a hipStream_t (0 = default stream).  Functions return 0 (MPC_OK) on success, a negative
 * MPC_E_* code of include/mpc_batch.h otherwise; mpc_ppo_last_error() (include/mpc_ppo.h) gives the text.  Every call validates its arguments before
 * the device is touched, and none synchronises.
 */
#ifndef MPC_PPO_UPDATE_H
#define MPC_PPO_UPDATE_H

#include "mpc_ppo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_ppo_update mpc_ppo_update;

/* A handle over an existing, bound mpc_ac (which must outlive it), on the mpc_ac's device.  It owns the workspace for mini-batches of up to max_rows
 * rows: the activations and their gradients, the per-chunk weight-gradient partials, the reduction partials. */
int mpc_ppo_update_create(mpc_ppo_update **out, mpc_ac *ac, int max_rows);
void mpc_ppo_update_destroy(mpc_ppo_update *u);
/* Number of parameter tensors: 2 (actor layers + critic layers) + 1, in mpc_ac_bind's order: actor weights, actor biases, critic weights, critic
 * biases, std.  -1 for a null handle. */
int mpc_ppo_update_tensors(const mpc_ppo_update *u);
/* Bytes of device memory the handle owns: the workspace of mpc_ppo_update_create and the norm's partials of mpc_ppo_update_bind_extra.  -1 for a null
 * handle. */
long long mpc_ppo_update_workspace_bytes(const mpc_ppo_update *u);
/* For tests: *d_out = the workspace's d loss / d (output of `layer` of net 0 = actor, 1 = critic) as the last grads call left it, [rows][*ld] floats (the
 * last layer's 12 or 1 columns in a row of 16), valid while the handle lives.  No device call. */
int mpc_ppo_update_layer_gradient(const mpc_ppo_update *u, int net, int layer, float **d_out, int *ld);
/* The gradient tensors and Adam's moments (exp_avg, exp_avg_sq), each a host array of mpc_ppo_update_tensors() DEVICE pointers in that order, shaped
 * like their parameters, non-null and 16-byte aligned.  Kept, not copied.  d_exp_avg and d_exp_avg_sq may both be NULL: mpc_ppo_update_apply then
 * refuses. */
int mpc_ppo_update_bind(mpc_ppo_update *u, float *const *d_grads, float *const *d_exp_avg, float *const *d_exp_avg_sq);
/* The flat rollout storage, total_rows = T N rows: d_obs [.][actor_dims[0]], d_actions, d_mu, d_sigma [.][12], d_values, d_advantages, d_returns,
 * d_log_prob [.]. */
int mpc_ppo_update_set_storage(mpc_ppo_update *u, long long total_rows, const float *d_obs, const float *d_actions, const float *d_values,
                               const float *d_advantages, const float *d_returns, const float *d_log_prob, const float *d_mu, const float *d_sigma);
/* The critic's rows of an asymmetric actor-critic (mpc_ac_create_asymmetric): d_critic_obs [total_rows][critic_dims[0]], 16-byte aligned, indexed by
 * the same d_idx as the rest of the storage; the critic's first layer reads it, forward and backward, in place of d_obs.  NULL clears it.  An
 * asymmetric mpc_ac without it is refused by mpc_ppo_update_grads with MPC_E_ARG. */
int mpc_ppo_update_set_critic_storage(mpc_ppo_update *u, const float *d_critic_obs);
/* One mini-batch: rows 1 .. max_rows, d_idx [rows] int64 row numbers into the storage (values outside [0, total_rows) are clamped into it).  Writes the
 * bound gradients, d_terms [4] = (surrogate, value loss, mean entropy, mean kl) as float32, and, if adaptive != 0, *d_lr (float64) by
 * PPO.adapt_learning_rate's rule with desired_kl > 0.  clip_param > 0. */
int mpc_ppo_update_grads(mpc_ppo_update *u, int rows, const long long *d_idx, double clip_param, double value_loss_coef, double entropy_coef,
                         int use_clipped_value_loss, int adaptive, double desired_kl, double *d_lr, float *d_terms, void *stream);
/* clip_grad_norm_(max_norm) over the bound gradients (they are scaled in place, as torch scales them), then Adam's step number `step` (>= 1, the
 * host's count) with the learning rate *d_lr. */
int mpc_ppo_update_apply(mpc_ppo_update *u, double max_norm, double beta1, double beta2, double eps, int step, const double *d_lr, void *stream);

/* ---- a recurrent actor-critic: the mpc_ac's nets read the outputs of two memories (csrc/mpc_recurrent_bptt.h), whose parameters are updated with them */
enum { MPC_PPO_UPDATE_MAX_EXTRA = 8 };
/* The dense rows [max_rows][actor_dims[0]] and [max_rows][critic_dims[0]] that the two first layers read in mpc_ppo_update_grads_sequence, and the
 * buffers of the same shapes that receive d loss / d rows.  Kept by pointer, 16-byte aligned; the two gradient buffers overlap neither each other nor
 * the rows.  Four NULLs clear them. */
int mpc_ppo_update_set_sequence_rows(mpc_ppo_update *u, const float *d_rows_actor, const float *d_rows_critic, float *d_drows_actor,
                                     float *d_drows_critic);
/* mpc_ppo_update_grads for one mini-batch of dense rows: row r of the buffers above goes with storage row d_idx[r].  Layer 0 of both nets reads the
 * dense rows, forward and in its weight gradient, with no index; the loss head reads the storage through d_idx; after layer 0's weight gradient one
 * more launch writes d rows_k = dY_0 W_0 (no activation factor) into rows 0 .. rows of the gradient buffers.  Means are over `rows`.  The storage's
 * d_obs and the critic's storage are not read.  The other arguments, outputs and launches are mpc_ppo_update_grads'. */
int mpc_ppo_update_grads_sequence(mpc_ppo_update *u, int rows, const long long *d_idx, double clip_param, double value_loss_coef, double entropy_coef,
                                  int use_clipped_value_loss, int adaptive, double desired_kl, double *d_lr, float *d_terms, void *stream);
/* count (0 .. MPC_PPO_UPDATE_MAX_EXTRA) more parameter tensors of numel[t] floats each, with their gradients and Adam's moments (host arrays of DEVICE
 * pointers, non-null and 16-byte aligned, kept; both moment arrays may be NULL: mpc_ppo_update_apply then refuses), which mpc_ppo_update_apply takes
 * into the total norm, the clip and Adam's step after the mpc_ac's tensors, in the order given.  After mpc_ppo_update_bind.  count = 0 clears them, and
 * apply is then what it is without this call, bit for bit.  Allocates the norm's partials for the longer list (the one device call, after every
 * refusal). */
int mpc_ppo_update_bind_extra(mpc_ppo_update *u, int count, float *const *d_params, float *const *d_grads, float *const *d_exp_avg,
                              float *const *d_exp_avg_sq, const int *numel);

/* ---- policy distillation: behaviour cloning of a teacher's actions into the ACTOR of the (student's) mpc_ac, on this handle's workspace, bound
 * gradients and moments.  The critic's tensors and std, their gradients and their moments are neither read nor written by the two calls below. */
/* The labels: d_teacher_actions [total_rows][12], 16-byte aligned, indexed by d_idx like the storage's d_obs (mpc_ac_act_distill writes a slot of
 * it per tick).  Kept by pointer; NULL clears it. */
int mpc_ppo_update_set_distill_targets(mpc_ppo_update *u, const float *d_teacher_actions);
/* One mini-batch: the forward pass of the actor alone over the rows d_idx names in the storage's d_obs (the GEMM launches of mpc_ppo_update_grads with
 * the critic's slot empty), the behaviour-cloning head, the actor's backward pass into its bound gradients.  With d = mu[r][k] - target[d_idx[r]][k]
 * over the 12 rows elements: loss_type 0 (mse): loss = mean d^2, d loss / d mu = 2 d / (12 rows); 1 (huber, delta = 1): the mean of 0.5 d^2 where
 * |d| <= 1 and |d| - 0.5 otherwise, d loss / d mu = clamp(d, -1, 1) / (12 rows).  Elements in float32 as torch's mse_loss / huber_loss take them;
 * the sums in float64 in a fixed order, no atomics.  d_terms [2] = (loss, mean |d|) as float32.  Refused with MPC_E_ARG, before the device is touched:
 * rows outside 1 .. max_rows, an unknown loss_type, no gradients bound, no storage set, no targets set. */
int mpc_ppo_update_grads_distill(mpc_ppo_update *u, int rows, const long long *d_idx, int loss_type, float *d_terms, void *stream);
/* mpc_ppo_update_apply over the actor's weight and bias tensors alone: clip_grad_norm_(max_norm) and torch.optim.Adam's step over
 * actor.parameters().  Refused without gradients and moments bound. */
int mpc_ppo_update_apply_actor(mpc_ppo_update *u, double max_norm, double beta1, double beta2, double eps, int step, const double *d_lr, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MPC_PPO_UPDATE_H */
