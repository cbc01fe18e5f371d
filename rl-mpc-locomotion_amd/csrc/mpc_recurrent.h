/*
 * mpc_recurrent.h -- the C ABI of the recurrent actor-critic's memories (mpc_recurrent.hip, recurrent_cell.h): one LSTM step (one layer, torch's
 * nn.LSTM parameter layout) for n environments, for the actor's memory and the critic's in ONE launch.
 *
 *   gates = x W_ih^T + b_ih + h W_hh^T + b_hh        W_ih [4H][I], W_hh [4H][H], rows in torch's order i, f, g, o
 *   i, f, o = sigmoid, g = tanh;   c' = f c + i g;   h' = o tanh(c')                    float32 throughout
 *
 * A handle holds one or two memories, each with its own I and H (mpc_recurrent_create), its own parameters (mpc_recurrent_bind: by pointer, never
 * copied -- an optimiser's in-place step is seen by the next launch) and, per call, its own rows and state (mpc_recurrent_io).  The state lives
 * with the caller; the handle owns no device memory.
 *
 * mpc_recurrent_step, per memory: where d_reset[r] != 0 the state of row r is taken as zero before the step (rsl_rl's Memory.reset(dones) of the
 * tick before, folded into this step); d_h_saved / d_c_saved receive the state the step started from, after that zeroing (what a rollout
 * storage keeps for the slot: the pointers may point straight into it); d_h_out receives h'; with commit != 0, d_h / d_c are overwritten
 * with h' / c', with commit == 0 they are left untouched and d_h_out alone is written.
 *
 * This header lives beside the sources and not under include/, like mpc_plant_rand.h.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_recurrent_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_RECURRENT_H
#define MPC_RECURRENT_H

#include "../../include/mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_RECURRENT_MEMORIES = 2, MPC_RECURRENT_MAX_LDS = 160 * 1024 };

typedef struct mpc_recurrent mpc_recurrent;

/* What one memory reads and writes in a step.  Every pointer 16-byte aligned; d_h_saved, d_c_saved and d_h_out may be NULL; the arrays must not
 * overlap one another. */
typedef struct {
  const float *d_x;            /* [n][I] */
  float *d_h, *d_c;            /* [n][H] the persistent state */
  float *d_h_saved, *d_c_saved;/* [n][H] or NULL */
  float *d_h_out;              /* [n][H] or NULL */
} mpc_recurrent_io;

/* memories (1 or 2) cells of input_sizes[k] inputs and hidden_sizes[k] state elements.  MPC_E_ARG, before the device is touched, for a null
 * pointer, an I or H that is not a positive multiple of 16, and a cell whose 16 (I + H + 8) floats of LDS exceed 160 KB. */
int mpc_recurrent_create(mpc_recurrent **out, int memories, const int *input_sizes, const int *hidden_sizes);
void mpc_recurrent_destroy(mpc_recurrent *h);
/* Arrays of `memories` device pointers each: weight_ih [4H][I], weight_hh [4H][H], bias_ih [4H], bias_hh [4H], float32.  MPC_E_ARG for a
 * pointer that is null or not 16-byte aligned; the handle lives on the caller's current device from here on. */
int mpc_recurrent_bind(mpc_recurrent *h, const float *const *d_w_ih, const float *const *d_w_hh, const float *const *d_b_ih, const float *const *d_b_hh);
/* One launch that steps the memories first .. first + count - 1 of the handle on n >= 1 rows; io [count], one record per stepped memory.
 * d_reset [n] int64 or NULL (8-byte aligned): the same flags for every stepped memory. */
int mpc_recurrent_step(mpc_recurrent *h, int n, int first, int count, const mpc_recurrent_io *io, const long long *d_reset, int commit, void *stream);
const char *mpc_recurrent_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_RECURRENT_H */
