/*
 * include/mpc_ppo.h -- C ABI of the collection half of a PPO iteration (rsl_rl v1.0.2, which the reference trains through,
 * RL_Environment/train.py:61-81): what runs once per environment tick and once per iteration before the update, for N environments on the
 * device, stream-ordered and with no host synchronisation.
 *
 *   mpc_ac_act            ActorCritic.act + evaluate: actor and critic MLPs in ONE launch, the actor half ending in the sampling / log-prob
 *                         epilogue.  Every output pointer is the caller's and may point straight into slot t of its rollout storage.
 *   mpc_ac_act_asymmetric the same launch for an asymmetric actor-critic: the critic reads privileged rows of its own width
 *   mpc_ac_evaluate       the critic alone (the iteration's last_values)
 *   mpc_ac_act_inference  the actor's mean alone (ActorCritic.act_inference)
 *   mpc_ac_act_distill    the same launch over two handles: a student's actor samples, a teacher's actor labels the rows with its mean
 *   mpc_rollout_add       PPO.process_env_step: the time-out bootstrap r' = r + gamma (v to) and the done flag into slot t, read from the task's own
 *                         int64 reset / time-out buffers
 *   mpc_rollout_returns   RolloutStorage.compute_returns over [T][N] storage, then advantages = (A - mean) / (std + 1e-8)
 *
 * The arithmetic is rl-mpc-locomotion_amd/csrc/ppo_rollout.h: float32 in rsl_rl's operation order; the MLP layers are policy_mlp.h's, so the
 * mean equals mpc_policy_step's raw action bit for bit.  The noise is a counter-based generator keyed by (seed, environment, step, action
 * pair), not torch's: parity with torch.distributions.Normal.sample is in distribution only, and |eps| <= 5.768.
 *
 * The weights are NOT copied: mpc_ac_bind keeps the caller's device pointers and every launch reads the parameters where they are, so an
 * optimiser that updates them in place is seen by the next launch and no weight copy is ever made.
 *
 * All pointers named d_* are DEVICE pointers; `stream` is a hipStream_t (0 = default stream).  Functions return 0 (MPC_OK) on success, a
 * negative MPC_E_* code of include/mpc_batch.h otherwise; mpc_ppo_last_error() gives the text.  Every call validates its arguments before the
 * device is touched, and none synchronises.
 */
#ifndef MPC_PPO_H
#define MPC_PPO_H

#include "mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_ac mpc_ac;

enum { MPC_AC_MAX_LAYERS = 8, MPC_AC_ACTIONS = 12 };

/* Two Linear / ELU stacks (ELU after every layer but the last): the actor, actor_dims[0] -> ... -> actor_dims[n_actor_layers] = 12, and the critic,
 * critic_dims[0] -> ... -> critic_dims[n_critic_layers] = 1, over the same observations (actor_dims[0] == critic_dims[0]).  Depths and widths may
 * differ otherwise.  Limits of mpc_policy_create: 1 .. 8 layers, every layer input width a positive multiple of 16, at most 16 outputs.  Host-only:
 * no device is needed until mpc_ac_bind. */
int mpc_ac_create(mpc_ac **out, int n_actor_layers, const int *actor_dims, int n_critic_layers, const int *critic_dims);
/* The asymmetric actor-critic (rsl_rl's num_critic_obs): the same two stacks with the same limits per stack, but the critic reads rows of its own,
 * so actor_dims[0] and critic_dims[0] are independent (the LDS limit holds for the wider of the two nets).  On such a handle the critic's
 * observations are an argument of their own (mpc_ac_act_asymmetric), mpc_ac_evaluate reads rows of width critic_dims[0] and mpc_ac_act_inference
 * rows of width actor_dims[0]; the plain mpc_ac_act is refused with MPC_E_ARG, before the device is touched, when the two widths differ. */
int mpc_ac_create_asymmetric(mpc_ac **out, int n_actor_layers, const int *actor_dims, int n_critic_layers, const int *critic_dims);
void mpc_ac_destroy(mpc_ac *ac);
/* The parameters, on the current HIP device: per layer a DEVICE pointer to its weight [out][in] row-major (torch Linear.weight) and to its bias [out],
 * given as host arrays of n_actor_layers / n_critic_layers pointers, and d_std [12].  Every pointer must be non-null and 16-byte aligned.  Kept, not
 * copied; may be called again (after the parameters have moved). */
int mpc_ac_bind(mpc_ac *ac, const float *const *d_actor_weights, const float *const *d_actor_biases, const float *const *d_critic_weights,
                const float *const *d_critic_biases, const float *d_std);
/* d_obs [n][actor_dims[0]] -> d_actions [n][12] = mean + std * eps, d_log_prob [n], d_values [n], d_mean [n][12], d_sigma [n][12] (std, broadcast:
 * rsl_rl's action_sigma) and, unless NULL, d_eps [n][12] (the noise, for tests).  eps of environment r is a function of (seed, r, step) alone. */
int mpc_ac_act(mpc_ac *ac, int n, const float *d_obs, unsigned long long seed, unsigned int step, float *d_actions, float *d_log_prob, float *d_values,
               float *d_mean, float *d_sigma, float *d_eps, void *stream);
/* The same single launch with the critic's rows given apart: d_obs [n][actor_dims[0]] feeds the actor, d_critic_obs [n][critic_dims[0]] (non-null)
 * the critic.  The actor's outputs are bit for bit those of the plain call on the same actor and d_obs; d_values those of mpc_ac_evaluate on
 * d_critic_obs. */
int mpc_ac_act_asymmetric(mpc_ac *ac, int n, const float *d_obs, const float *d_critic_obs, unsigned long long seed, unsigned int step, float *d_actions,
                          float *d_log_prob, float *d_values, float *d_mean, float *d_sigma, float *d_eps, void *stream);
int mpc_ac_evaluate(mpc_ac *ac, int n, const float *d_obs, float *d_values, void *stream);
int mpc_ac_act_inference(mpc_ac *ac, int n, const float *d_obs, float *d_mean, void *stream);
/* Collection for policy distillation, still ONE launch on a grid of (ceil(n / 16), 2): the student's actor acts on d_obs [n][student actor_dims[0]]
 * and samples (d_actions, d_mean, d_sigma and, unless NULL, d_eps as mpc_ac_act writes them, bit for bit, with the same (seed, environment, step,
 * pair) key; no log-prob and no value), and beside it the TEACHER's actor reads d_teacher_obs [n][teacher actor_dims[0]] and writes its mean, the
 * label, to d_teacher_actions [n][12]: bit for bit mpc_ac_act_inference(teacher, d_teacher_obs).  Two handles, both bound, on one device; depths and
 * widths are independent and neither critic is read.  The teacher's parameters are only read. */
int mpc_ac_act_distill(mpc_ac *student, mpc_ac *teacher, int n, const float *d_obs, const float *d_teacher_obs, unsigned long long seed, unsigned int step,
                       float *d_actions, float *d_mean, float *d_sigma, float *d_teacher_actions, float *d_eps, void *stream);
/* d_rew [n] float32, d_reset [n] and d_timeout [n] int64 (0 / 1; the task's buffers as they are), d_values_t [n] (slot t, as written by mpc_ac_act)
 * -> d_rewards_t [n] = r + gamma (v to), d_dones_t [n] = reset != 0 as float32.  gamma in [0, 1], used as its float32 value. */
int mpc_rollout_add(int n, double gamma, const float *d_rew, const long long *d_reset, const long long *d_timeout, const float *d_values_t,
                    float *d_rewards_t, float *d_dones_t, void *stream);
/* d_rewards, d_dones, d_values [T][n] and d_last_values [n] -> d_returns [T][n] and d_advantages [T][n], normalised over all T n values (mean and
 * unbiased standard deviation accumulated in float64 in a fixed order, no atomics: a rerun is bit-identical; T n = 1 gives NaN, as torch's std does).
 * gamma and lam in [0, 1], used as their float32 values. */
int mpc_rollout_returns(int n, int T, double gamma, double lam, const float *d_rewards, const float *d_dones, const float *d_values,
                        const float *d_last_values, float *d_returns, float *d_advantages, void *stream);
const char *mpc_ppo_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_PPO_H */
