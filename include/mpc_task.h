/*
 * include/mpc_task.h -- C ABI of the RL task's post-physics half: what VecTask.step does after the simulator has stepped
 * (RL_Environment/tasks/base/vec_task.py:326-337) and the task's post_physics_step (RL_Environment/tasks/aliengo.py:273-349, the same text
 * in a1.py / go1.py), for N environments on the device, in two stream-ordered kernels and with no host synchronisation.
 *
 *   mpc_task_begin    the time-out flag, the episode counter, and for every environment whose reset flag is set: its id into the id array,
 *                     fresh commands, progress = 0.  The id array has one entry per environment (the id itself, or -1): hand it with k = n
 *                     to mpc_ctrl_reset_device / mpc_ctrl_fsm_reset_device / mpc_sim_reset_device / mpc_batch_reset_device, which ignore ids
 *                     outside [0, n).  So no `reset_buf.nonzero()` and no count ever reaches the host.
 *   (the caller resets its simulator and controllers with the id array)
 *   mpc_task_finish   the 48 observations (clipped), the reward and the next reset flags.
 *
 * The arithmetic is rl-mpc-locomotion_amd/csrc/rl_task.h: float32 in the reference's operation order.  Commands are drawn by a counter-based
 * generator keyed by (seed, environment, episode index), not by torch's generator: parity with the reference there is in distribution only.
 *
 * All pointers named d_* are DEVICE pointers; `stream` is a hipStream_t (0 = default stream).  Functions return 0 (MPC_OK) on success, a
 * negative MPC_E_* code of include/mpc_batch.h otherwise; mpc_task_last_error() gives the text.
 */
#ifndef MPC_TASK_H
#define MPC_TASK_H

#include "mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_task mpc_task;

enum { MPC_TASK_OBS = 48, MPC_TASK_REW_TERMS = 6 };

/* cfg/task/Aliengo.yaml (A1.yaml, Go1.yaml) as numbers.  Every value is rounded to float32 where the reference's float32 tensors meet it. */
typedef struct mpc_task_config {
  double lin_vel_scale, ang_vel_scale, dof_pos_scale, dof_vel_scale;   /* learn.linearVelocityScale ... dofVelocityScale */
  double rew_scale[MPC_TASK_REW_TERMS]; /* lin_vel_xy, lin_vel_z, ang_vel_xy, ang_vel_z, torque, collision (the order of the sum at aliengo.py:398),
                                           each ALREADY multiplied by dt (aliengo.py:78-79) */
  double command_range[3][2];           /* randomCommandVelocityRanges linear_x, linear_y, yaw: (min, max) */
  double clip_observations;             /* clipObservations, > 0 */
  double default_dof_pos[12];           /* defaultJointAngles in dof order */
  long long max_episode_length;         /* int(episodeLength_s / dt + 0.5), >= 1 (aliengo.py:73-74) */
  unsigned long long seed;              /* of the command generator */
} mpc_task_config;

/* The buffers of the task, owned by the caller (the reference's public tensors, vec_task.py:232-246 and aliengo.py:109). */
typedef struct mpc_task_buffer_set {
  long long *d_progress;                /* [n] progress_buf */
  long long *d_reset;                   /* [n] reset_buf (0 / 1) */
  long long *d_timeout;                 /* [n] timeout_buf (0 / 1) */
  int *d_reset_ids;                     /* [n] written by begin: r where environment r is being reset, -1 elsewhere */
  float *d_commands;                    /* [n][3] vx, vy, yaw rate; rewritten by begin for the environments being reset, otherwise the caller's */
  float *d_obs;                         /* [n][48] obs_buf, clipped */
  float *d_rew;                         /* [n] rew_buf */
} mpc_task_buffer_set;

/* n environments on the current HIP device.  Replaces the configuration reading of Aliengo.__init__ (aliengo.py:28-47, :73-79, :113-118).
 * Arguments are validated before the device is touched. */
int mpc_task_create(mpc_task **out, int n, const mpc_task_config *cfg);
void mpc_task_destroy(mpc_task *t);
/* binds the caller's buffers (all seven required); nothing is written */
int mpc_task_buffers(mpc_task *t, const mpc_task_buffer_set *buffers);
/* vec_task.py:326, aliengo.py:274-278 and the task-buffer part of reset_idx (aliengo.py:344-349) */
int mpc_task_begin(mpc_task *t, void *stream);
/* compute_observations + compute_reward (aliengo.py:280-319, :357-444) and the observation clip (vec_task.py:337).
 * d_root [n][13], d_dof [n][12][2], d_actions [n][12], d_torques [n][12].  Contacts in two optional forms (both NULL: no contacts; both given:
 * either one counts):
 *   d_contact_forces [n][bodies][3] with base_index, knee_indices [4], hip_indices [4] (host arrays): Isaac Gym's net contact force tensor;
 *   d_fell [n], one byte per environment (0 / 1): taken as base contact (the toy plant of include/mpc_sim.h). */
int mpc_task_finish(mpc_task *t, const float *d_root, const float *d_dof, const float *d_actions, const float *d_torques,
                    const float *d_contact_forces, int bodies, int base_index, const int *knee_indices, const int *hip_indices,
                    const unsigned char *d_fell, void *stream);
const char *mpc_task_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_TASK_H */
