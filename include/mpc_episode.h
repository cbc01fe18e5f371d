/*
 * include/mpc_episode.h -- C ABI of the device-side episode statistics: what rsl_rl v1.0.2's OnPolicyRunner.learn keeps per tick on the host
 * (cur_reward_sum += rewards, cur_episode_length += 1, and for dones.nonzero() an extend of two deque(maxlen=100) and the zeroing), kept on the
 * device for N environments, stream-ordered and with no host synchronisation, plus running totals overall and per group of environments.
 *
 *   mpc_episode_add              one tick: accumulate, then append every finished environment's (return, length, timed out) to the window in
 *                                ascending environment index, add it to the totals, zero its accumulators
 *   mpc_episode_summary          window count / mean return / mean length / timed-out count and all totals into the float64 summary
 *   mpc_episode_restart          zero the in-flight accumulators (window and totals stay)
 *   mpc_episode_clear            zero everything
 *   mpc_episode_random_progress  rsl_rl's init_at_random_ep_len: progress[i] uniform on [0, max_len), a function of (seed, i) alone
 *
 * The arithmetic and the slot rule are rl-mpc-locomotion_amd/csrc/episode_stats.h.  The window is collections.deque(maxlen=cap) extended in
 * (tick, environment) order, stored as a ring: the environment with `rank` finished environments of lower index before it on a tick that finishes
 * `total` writes slot (head + rank) mod cap, unless rank < total - cap (a tick that finishes more than cap episodes keeps the last cap by
 * environment index: every slot has one writer); head advances by total.  No atomics, no workgroup waits on another, every sum runs in a fixed
 * order: a rerun is bit-identical.
 *
 * All buffers are the CALLER's device memory (mpc_episode_bind keeps the pointers); the handle owns only a workspace of per-workgroup partials.
 * All pointers named d_* are DEVICE pointers; `stream` is a hipStream_t (0 = default stream).  Functions return 0 (MPC_OK) on success, a negative
 * MPC_E_* code of include/mpc_batch.h otherwise; mpc_episode_last_error() gives the text.  Every call validates its arguments before the device is
 * touched, and none synchronises.
 */
#ifndef MPC_EPISODE_H
#define MPC_EPISODE_H

#include "mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_episode mpc_episode;

enum { MPC_EPISODE_MAX_GROUPS = 64 };

/* d_counters [MPC_EPISODE_COUNTERS + MPC_EPISODE_COUNTER_STRIDE * (1 + G)] int64: head (the next slot), the window's count, then per block
 * (block 0 overall, block 1 + g group g) episodes finished, of those timed out, sum of lengths. */
enum { MPC_EPISODE_HEAD = 0, MPC_EPISODE_COUNT = 1, MPC_EPISODE_COUNTERS = 2, MPC_EPISODE_COUNTER_STRIDE = 3 };
enum { MPC_EPISODE_C_EPISODES = 0, MPC_EPISODE_C_TIMEOUTS = 1, MPC_EPISODE_C_SUM_LENGTH = 2 };

/* d_summary [MPC_EPISODE_SUMMARY_TOTALS + MPC_EPISODE_SUMMARY_STRIDE * (1 + G)] float64: the window's count, mean return, mean length (float64
 * sums over the window's slots -- lane t of 256 adds slots t, t + 256, ... in ascending index, a fixed tree joins the lanes -- divided by the count; 0.0, never NaN, when the window is empty), timed-out count; then per block (0 overall, 1 + g
 * group g) episodes, timed out, sum of returns, sum of lengths. */
enum { MPC_EPISODE_S_WINDOW_COUNT = 0, MPC_EPISODE_S_MEAN_RETURN = 1, MPC_EPISODE_S_MEAN_LENGTH = 2, MPC_EPISODE_S_WINDOW_TIMEOUTS = 3,
       MPC_EPISODE_SUMMARY_TOTALS = 4, MPC_EPISODE_SUMMARY_STRIDE = 4 };
enum { MPC_EPISODE_T_EPISODES = 0, MPC_EPISODE_T_TIMEOUTS = 1, MPC_EPISODE_T_SUM_RETURN = 2, MPC_EPISODE_T_SUM_LENGTH = 3 };

typedef struct {
  float *d_cur_return;        /* [n]   the in-flight return of each environment */
  int *d_cur_length;          /* [n]   its length so far */
  float *d_win_return;        /* [cap] the ring */
  int *d_win_length;          /* [cap] */
  int *d_win_timed_out;       /* [cap] 0 / 1 */
  long long *d_counters;      /* see MPC_EPISODE_HEAD */
  double *d_sums;             /* [1 + G] float64 sum of returns: overall, then per group */
  double *d_summary;          /* see MPC_EPISODE_S_WINDOW_COUNT */
  const int *d_groups;        /* [n] group of each environment, or NULL: all in group 0.  An id outside [0, G) counts overall only. */
} mpc_episode_buffers_t;

/* n >= 1 environments, a window of cap >= 1 entries, 1 <= num_groups <= MPC_EPISODE_MAX_GROUPS.  Host-only: no device is needed until
 * mpc_episode_bind. */
int mpc_episode_create(mpc_episode **out, int n, int cap, int num_groups);
void mpc_episode_destroy(mpc_episode *ep);
/* The buffers, on the current HIP device (every pointer but d_groups non-null).  Kept, not copied, not initialised: the caller zeroes them or calls
 * mpc_episode_clear.  Allocates the workspace. */
int mpc_episode_bind(mpc_episode *ep, const mpc_episode_buffers_t *buffers);
/* One tick, three launches: a grid over n accumulates and writes per-workgroup partials, one workgroup scans them in index order, a grid over n
 * places the entries.  d_rew [n] float32, d_reset [n] and d_timeout [n] int64 (the task's buffers as they are): finished = reset > 0, timed out = finished and
 * timeout > 0. */
int mpc_episode_add(mpc_episode *ep, const float *d_rew, const long long *d_reset, const long long *d_timeout, void *stream);
int mpc_episode_summary(mpc_episode *ep, void *stream);
int mpc_episode_restart(mpc_episode *ep, void *stream);
int mpc_episode_clear(mpc_episode *ep, void *stream);
/* d_progress [n] int64 <- an integer uniform on [0, max_len), 1 <= max_len <= 2^31; environment i's value does not depend on n. */
int mpc_episode_random_progress(long long *d_progress, int n, long long max_len, unsigned long long seed, void *stream);
const char *mpc_episode_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_EPISODE_H */
