/*
 * mpc_privileged_obs.h -- the C ABI of the critic's privileged observation row (mpc_privileged_obs.hip, privileged_obs.h): asymmetric
 * actor-critic training, where the critic reads a noise-free, wider row than the actor.
 *
 * mpc_privobs_run takes the task's wide observation row [n][obs_width] as it stands BEFORE the observation noise, the bound sim's int32 state
 * record (its four foot-contact flags) and the task's int64 episode counter, and writes one row [n][mpc_privobs_width(P)] per environment: the
 * 48 + P live columns copied, the four contact flags as 0.0 / 1.0, the episode phase float32(progress) * inv_len, zeros up to the next multiple
 * of 16.  One kernel, one launch; the whole row is written on every call, the pad included.  Stream-ordered, no host read, no atomics, no LDS.
 *
 * This header lives beside the sources and not under include/, like mpc_height_scan.h: tests/test_abi.py keeps a table of every header under
 * include/, and that table is fixed.
 *
 * Pointers named d_* are DEVICE pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code of
 * include/mpc_batch.h; mpc_privobs_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_PRIVILEGED_OBS_H
#define MPC_PRIVILEGED_OBS_H

#include "../../include/mpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_PRIVOBS_TASK_OBS = 48, MPC_PRIVOBS_CONTACTS = 4, MPC_PRIVOBS_MAX_SCAN = 208 };

typedef struct mpc_privobs mpc_privobs;

/* 16 * ceil((48 + P + 5) / 16), or MPC_E_ARG for P outside 0 .. MPC_PRIVOBS_MAX_SCAN.  Needs no device. */
int mpc_privobs_width(int P);
/* A handle for n environments.  Host-only: the device is the bound sim's.  MPC_E_ARG for a null pointer or n < 1. */
int mpc_privobs_create(mpc_privobs **out, int n);
void mpc_privobs_destroy(mpc_privobs *h);
/* Keep the device address of s's int32 state record (contact4 lift4 fell, [9][n]) and its device.  MPC_E_ARG for a null handle or a sim of
 * another size. */
int mpc_privobs_bind(mpc_privobs *h, mpc_sim *s);
/* d_obs [n][obs_width] float32 (obs_width a multiple of 4, at least 48 + P; only its first 48 + P columns are read), d_progress [n] int64,
 * inv_len used as its float32 value, d_out [n][mpc_privobs_width(P)] float32.  d_obs and d_out must be non-null, 16-byte aligned and not the same
 * buffer.  MPC_E_ARG otherwise, for an inv_len that is not finite, or without a bound sim. */
int mpc_privobs_run(mpc_privobs *h, const float *d_obs, int obs_width, int P, const long long *d_progress, double inv_len, float *d_out,
                    void *stream);
/* The row with the plant's per-robot record (mpc_plant_rand.h): three more columns after the phase -- (float)payload, (float)(strength - 1.0),
 * (float)(grav_z + 9.81), each one float64 subtraction (none for the first) and one conversion -- and a width of 16 * ceil((48 + P + 5 + 3) / 16).
 * mpc_privobs_bind_plant keeps the device address of s's plant record: after mpc_privobs_bind of the same sim, and MPC_E_ARG for a sim that
 * has none.  mpc_privobs_run_plant is mpc_privobs_run on that row: d_out [n][mpc_privobs_width_plant(P)]; MPC_E_ARG without a bound record. */
int mpc_privobs_width_plant(int P);
int mpc_privobs_bind_plant(mpc_privobs *h, mpc_sim *s);
int mpc_privobs_run_plant(mpc_privobs *h, const float *d_obs, int obs_width, int P, const long long *d_progress, double inv_len, float *d_out,
                          void *stream);
const char *mpc_privobs_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_PRIVILEGED_OBS_H */
