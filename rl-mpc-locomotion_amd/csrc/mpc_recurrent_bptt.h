/*
 * mpc_recurrent_bptt.h -- the C ABI of the recurrent actor-critic's update through time (mpc_recurrent_bptt.hip, recurrent_bptt.h): mpc_recurrent.h's
 * LSTM step rolled over the T slots of a rollout for a block of B environments, and its backward pass, for the actor's memory and the critic's
 * together.  One layer, torch's nn.LSTM parameter layout and gate order i, f, g, o, float32 throughout.
 *
 * Forward, per memory, for t = 0 .. T-1: where d_reset[t][b] != 0 the state of row b is taken as zero; the step of mpc_recurrent.h runs from that
 * state on row x[t][b]; y[t][b] = h'.  Equal to T calls of mpc_recurrent_step bit for bit.
 *
 * Backward, given dY [T][B][H], with carries dh_rec = dc_rec = 0, for t = T-1 .. 0:
 *     dh  = dY[t] + dh_rec                  tc = tanh(c'[t])
 *     do~ = dh tc o(1-o)                    dc  = dc_rec + dh o (1 - tc^2)
 *     di~ = dc g i(1-i)    df~ = dc c_used[t] f(1-f)    dg~ = dc i (1 - g^2)           dG[t] = (di~, df~, dg~, do~)  [B][4H]
 *     dh_rec = dG[t] W_hh,  dc_rec = dc f;  both zero on rows where d_reset[t][b] != 0
 * and then, over all T B rows, dW_ih = dG^T X, dW_hh = dG^T h_used, db_ih = db_hh = the column sums of dG.  The four outputs are OVERWRITTEN (not
 * accumulated into).  Gradients with respect to x, h0 and c0 are not produced: they are data.  No atomics: a rerun is bit-identical.
 *
 * A handle is made for one or two memories, at most max_steps slots and at most max_rows environments per call.  mpc_recurrent_bptt_create is host
 * only; mpc_recurrent_bptt_bind takes the parameters BY POINTER (never copied: an optimiser's in-place step is seen by the next call; W_hh is
 * transposed anew in every backward call) and allocates the workspace on the caller's current device.  With R = max_steps max_rows and
 * C = ceil(R / 256), memory k of the handle owns
 *     4 (11 H R  +  4 H roundup(H, 64)  +  C (4 H I + 4 H H + 4 H))  +  8 R   bytes
 * (gate activations 4H, c', h_used, c_used, dG 4H per row; W_hh^T; the weight-gradient GEMMs' chunk partials; the x row index) and the handle 4 R
 * more for the reset flags: mpc_recurrent_bptt_workspace_bytes gives the sum.  At I = 48, H = 256, R = 24 x 1024 that is 398 MB per memory.
 *
 * This header lives beside the sources and not under include/, like mpc_recurrent.h.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_recurrent_bptt_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_RECURRENT_BPTT_H
#define MPC_RECURRENT_BPTT_H

#include "../../include/mpc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_RECURRENT_BPTT_MEMORIES = 2, MPC_RECURRENT_BPTT_MAX_LDS = 160 * 1024 };

typedef struct mpc_recurrent_bptt mpc_recurrent_bptt;

/* What one memory reads and writes in a forward call.  Every pointer 16-byte aligned; d_c_last may be NULL; d_y and d_c_last must not overlap each
 * other or another memory's. */
typedef struct {
  const float *d_x;            /* row (t, b) at d_x + t x_stride + b I: the block's rows read in place from a [T][N][I] storage (x_stride = N I) */
  long long x_stride;          /* floats between two slots: at least I, a multiple of 4 */
  const float *d_h0, *d_c0;    /* [B][H] */
  float *d_y;                  /* [T][B][H] */
  float *d_c_last;             /* [B][H] or NULL: c' of step T - 1 (h' of that step is d_y[T-1]) */
} mpc_recurrent_bptt_io;

/* What one memory reads and writes in a backward call.  The x rows are those of the matching forward call (its row index is kept in the
 * workspace).  Every pointer non-null and 16-byte aligned; the outputs must not overlap one another or another memory's. */
typedef struct {
  const float *d_dy;           /* [T][B][H] */
  float *d_w_ih, *d_w_hh;      /* [4H][I], [4H][H] */
  float *d_b_ih, *d_b_hh;      /* [4H] each (the same values) */
} mpc_recurrent_bptt_grads;

/* memories (1 or 2) cells of input_sizes[k] inputs and hidden_sizes[k] state elements, for calls of 1 .. max_steps slots and 1 .. max_rows
 * environments.  Host only.  MPC_E_ARG for a null pointer, an I or H that is not a positive multiple of 16, max_steps or max_rows below 1 (or
 * max_steps max_rows above 2^31 / 4H rows), and a cell whose forward pass (32 (I + H + 8) floats) or backward pass (16 (4 H + 4) floats) needs more
 * than 160 KB of LDS. */
int mpc_recurrent_bptt_create(mpc_recurrent_bptt **out, int memories, const int *input_sizes, const int *hidden_sizes, int max_steps, int max_rows);
void mpc_recurrent_bptt_destroy(mpc_recurrent_bptt *h);
long long mpc_recurrent_bptt_workspace_bytes(const mpc_recurrent_bptt *h);      /* -1 for a null handle */
/* Arrays of `memories` device pointers each, as mpc_recurrent_bind takes them.  MPC_E_ARG for a pointer that is null or not 16-byte aligned; the
 * first successful call allocates the workspace and the handle lives on the caller's current device from there on. */
int mpc_recurrent_bptt_bind(mpc_recurrent_bptt *h, const float *const *d_w_ih, const float *const *d_w_hh, const float *const *d_b_ih, const float *const *d_b_hh);
/* ONE launch that rolls the memories first .. first + count - 1 of the handle over T slots of B rows; io [count].  d_reset [T][B] int64 or NULL
 * (8-byte aligned): the same flags for every memory. */
int mpc_recurrent_bptt_forward(mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_io *io, const long long *d_reset, void *stream);
/* The backward pass of the handle's last forward call: a transposition of W_hh, ONE launch through time, two weight-gradient GEMM launches, the
 * column sums of dG (float64 per chunk of 256 rows) and one reduction, all memories side by side.  MPC_E_ARG where T, B, first or count differ from that forward call's, or there was none. */
int mpc_recurrent_bptt_backward(mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_grads *grads, void *stream);
/* The second half of mpc_recurrent_bptt_backward alone, on the dG that call left: the two GEMM launches, the column sums and the reduction (what a measurement times
 * on its own).  The same arguments and refusals; MPC_E_ARG also where no backward call followed the last forward call. */
int mpc_recurrent_bptt_weight_gradients(mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_grads *grads, void *stream);
/* Where the last backward call left dG, rows (t, b) at t B + b of that call, [T B][4H]: the handle's memory, valid until the handle is destroyed and
 * rewritten by the next backward call.  MPC_E_ARG for a null pointer, a memory the handle does not have, and a handle that was never bound. */
int mpc_recurrent_bptt_dgates(const mpc_recurrent_bptt *h, int memory, const float **d_dg);
const char *mpc_recurrent_bptt_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_RECURRENT_BPTT_H */
