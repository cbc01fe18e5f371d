/*
 * include/mpc_obs_norm.h -- C ABI of the running observation normaliser: rsl_rl 2.x's EmpiricalNormalization (per column of [n, D] float32
 * observations a running mean, population variance and row count; y = (x - mean) / (std + eps)), kept on the device, stream-ordered and with no
 * host synchronisation and no host read.
 *
 *   mpc_obsnorm_apply    one call per batch: with update != 0 the batch is first merged into the running state and the float32 buffers are
 *                        republished, then the batch is normalised with them; with update == 0 it is normalised only
 *   mpc_obsnorm_clear    back to the fresh state: count 0, mean 0, var 1 (rsl_rl's initial buffers)
 *
 * The arithmetic is rl-mpc-locomotion_amd/csrc/obs_norm.h.  The state is float64 (d_state: D means, then D variances) with an int64 row count;
 * batch statistics are float64, two-pass inside blocks of 32 rows, the blocks joined in index order by the pooled-moments formula; no sum of squares
 * of raw values, no atomics, every sum in a fixed order: a rerun is bit-identical.  The published buffers d_mean, d_var, d_std [D] float32 are the
 * roundings of mean, var and sqrt(var); normalisation is float32 on them (one subtraction, one addition std + eps, one division).  A row with
 * any non-finite entry is left out of the update and is not counted; it is normalised as arithmetic leaves it.  `until` >= 0: an update that finds
 * count >= until is skipped -- decided on the device from the device's count.
 *
 * All buffers are the CALLER's device memory (mpc_obsnorm_bind keeps the pointers); the handle owns only a workspace of per-block partials, which
 * grows (one allocation, outside the stream's order) the first time a batch has more rows than any before it.  All pointers named d_* are DEVICE
 * pointers; `stream` is a hipStream_t (0 = default stream).  Functions return 0 (MPC_OK) on success, a negative MPC_E_* code of
 * include/mpc_batch.h otherwise; mpc_obsnorm_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_OBS_NORM_H
#define MPC_OBS_NORM_H

#include "mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_obsnorm mpc_obsnorm;

enum { MPC_OBSNORM_MAX_OBS = 256, MPC_OBSNORM_BLOCK_ROWS = 32 };

typedef struct {
  double *d_state;            /* [2 * D] float64: mean[D], then var[D] */
  long long *d_count;         /* [1] int64: rows used so far */
  float *d_mean;              /* [D] float32 (float)mean */
  float *d_var;               /* [D] float32 (float)var */
  float *d_std;               /* [D] float32 (float)sqrt(var) */
} mpc_obsnorm_buffers_t;

/* 1 <= num_obs <= MPC_OBSNORM_MAX_OBS columns, eps finite and >= 0, until < 0 for none.  Host-only: no device is needed until mpc_obsnorm_bind. */
int mpc_obsnorm_create(mpc_obsnorm **out, int num_obs, float eps, long long until);
void mpc_obsnorm_destroy(mpc_obsnorm *h);
/* The buffers, on the current HIP device (every pointer non-null).  Kept, not copied, not initialised: the caller calls mpc_obsnorm_clear or
 * fills them. */
int mpc_obsnorm_bind(mpc_obsnorm *h, const mpc_obsnorm_buffers_t *buffers);
/* d_x [n, D] float32 contiguous -> d_y [n, D] float32 contiguous; d_y may be d_x (in place) or any buffer that does not otherwise overlap it.
 * n >= 1.  update != 0: three launches (a grid over blocks of 32 rows writes per-block partials; one workgroup joins them in index order, merges
 * and publishes; a grid normalises).  update == 0: the last launch alone. */
int mpc_obsnorm_apply(mpc_obsnorm *h, const float *d_x, float *d_y, long long n, int update, void *stream);
int mpc_obsnorm_clear(mpc_obsnorm *h, void *stream);
const char *mpc_obsnorm_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_OBS_NORM_H */
