/*
 * mpc_recurrent_policy.h -- the C ABI of a deployed recurrent weight policy (mpc_recurrent_policy.hip, recurrent_policy.h): one tick for n robots
 * in ONE launch -- the actor's memory (one LSTM layer, torch's nn.LSTM parameter layout), the actor's MLP on h', clamp and the affine map to MPC
 * weights.
 *
 *   gates = x W_ih^T + b_ih + h W_hh^T + b_hh        W_ih [4H][I], W_hh [4H][H], rows in torch's order i, f, g, o
 *   i, f, o = sigmoid, g = tanh;   c' = f c + i g;   h' = o tanh(c')
 *   a = actor(h')  (Linear / ELU stack, dims[0] = H);   weights = clamp(a, -1, 1) * act_scale + act_const          float32 throughout
 *
 * The entry points: mpc_recurrent_policy_create, mpc_recurrent_policy_step, mpc_recurrent_policy_destroy, mpc_recurrent_policy_last_error.
 *
 * A handle owns a device copy of the parameters, made once by create (a deployed policy's parameters do not change; mpc_policy_create's rule).  The
 * state h, c [n][H] lives with the caller and is updated in place by every step; where d_reset[r] != 0 the state of row r is taken as zero before
 * the step (rsl_rl's Memory.reset(dones) of the tick before, folded into this step), the row's observation is read as it is.
 *
 * This header lives beside the sources and not under include/, like mpc_recurrent.h.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_recurrent_policy_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_RECURRENT_POLICY_H
#define MPC_RECURRENT_POLICY_H

#include "../../include/mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_RECURRENT_POLICY_MAX_LDS = 160 * 1024 };

typedef struct mpc_recurrent_policy mpc_recurrent_policy;

/* All arrays are HOST float32 in torch's layouts, copied to the device once: w_ih [4H][I], w_hh [4H][H], b_ih, b_hh [4H]; dims [n_layers + 1];
 * weights[l] [dims[l+1]][dims[l]], biases[l] [dims[l+1]]; act_scale, act_const [dims[n_layers]].  MPC_E_ARG, before the device is touched, for: a null
 * pointer; I or H that is not a positive multiple of 16; n_layers outside 1 .. 8; dims[0] != H; dims[n_layers] outside 1 .. 16; a hidden width
 * dims[1 .. n_layers-1] that is not a positive multiple of 16; 16 rows of x, h and the MLP's two buffers above 160 KB of LDS.  MPC_E_NODEVICE
 * without a HIP device.  The handle lives on the caller's current device. */
int mpc_recurrent_policy_create(mpc_recurrent_policy **out, int I, int H, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int n_layers,
                                const int *dims, const float *const *weights, const float *const *biases, const float *act_scale, const float *act_const);
void mpc_recurrent_policy_destroy(mpc_recurrent_policy *p);
/* One launch, stream-ordered, no synchronisation.  d_obs [n][I]; d_h, d_c [n][H] read and overwritten; d_reset [n] int64 or NULL; d_actions
 * [n][dims[n_layers]] or NULL (the actor's raw output); d_weights [n][dims[n_layers]].  MPC_E_ARG, before the device is touched and before the handle
 * is looked at, for: a null d_obs, d_h, d_c or d_weights; n < 1; a float pointer that is not 16-byte aligned or a d_reset that is not 8-byte
 * aligned; d_h == d_c; then for a null handle. */
int mpc_recurrent_policy_step(mpc_recurrent_policy *p, int n, const float *d_obs, float *d_h, float *d_c, const long long *d_reset, float *d_actions, float *d_weights,
                              void *stream);
const char *mpc_recurrent_policy_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_RECURRENT_POLICY_H */
