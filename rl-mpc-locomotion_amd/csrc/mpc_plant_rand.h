/*
 * mpc_plant_rand.h -- the C ABI of the opt-in per-robot plant randomisation (mpc_plant_rand.hip, plant_rand.h): every robot of a toy-plant sim
 * gets a payload, a motor strength and a gravity of its own, drawn on the device at reset and consumed by the plant's step kernel.
 *
 * mpc_plant_rand_attach gives a sim (include/mpc_sim.h) its plant record [3][n] float64 (entry j of robot r at [j * n + r]: 0 payload in kg,
 * 1 strength as a factor, 2 grav_z in m/s^2, absolute), neutral (0, 1, -9.81), and from then on mpc_sim_step launches the parametrised step
 * kernel of the sim's ground: mass + payload, every torque times strength, the robot's own gravity.  The inertia is not changed.  A sim without
 * a record launches the kernels it launched before.  With the neutral record the parametrised kernel computes what the plain one computes, bit
 * for bit.
 *
 * mpc_plant_rand_draw is one kernel with one lane per slot of d_ids: environment r takes e = counter[r], draws
 * v = fminf(lo + (hi - lo) * uniform01(seed ^ domain, r, e, axis), hi) in float32 for each present axis, writes
 * payload = (double)v0, strength = (double)v1, grav_z = -9.81 + (double)v2 (an absent axis: its neutral value, no draw), and stores
 * counter[r] = e + 1.  Counter-based draws: nothing depends on n.  Stream-ordered; no host read, no atomics, no LDS.
 *
 * This header lives beside the sources and not under include/, like mpc_domain_rand.h.
 *
 * Pointers named d_* are DEVICE pointers, h_* HOST pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code
 * of include/mpc_batch.h; mpc_plant_rand_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_PLANT_RAND_H
#define MPC_PLANT_RAND_H

#include "../../include/mpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_PLANT_PAYLOAD = 0, MPC_PLANT_STRENGTH = 1, MPC_PLANT_GRAVITY = 2, MPC_PLANT_AXES = 3 };

typedef struct mpc_plant_rand mpc_plant_rand;

/* n environments, the seed of every draw.  MPC_E_ARG, before the device is touched, for a null pointer or n < 1. */
int mpc_plant_rand_create(mpc_plant_rand **out, int n, unsigned long long seed);
void mpc_plant_rand_destroy(mpc_plant_rand *h);
/* Allocate s's plant record (owned by the sim), neutral, and this handle's draw counters uint32 [n] (owned by the handle), zero.  MPC_E_ARG
 * for a sim of another size or on another device, for a handle that is attached already and for a sim that has a record already. */
int mpc_plant_rand_attach(mpc_plant_rand *h, mpc_sim *s);
/* d_ids [k] int32: r where environment r draws, anything outside [0, n) (the task's -1) is skipped; NULL: all n environments (k must be n).
 * The ids must be distinct, as the task's are (two lanes on one environment would race on its counter).  present [3]: non-zero where the axis is randomised; ranges [3][2]:
 * (lo, hi) of payload [kg], strength [factor] and the gravity OFFSET [m/s^2], read for the present axes only, rounded to float32, finite,
 * lo <= hi, strength lo >= 0: checked first, before the handle is looked at.  MPC_E_ARG otherwise, and before mpc_plant_rand_attach. */
int mpc_plant_rand_draw(mpc_plant_rand *h, const int *d_ids, int k, const int *present, const double *ranges, void *stream);
/* The record as a host array [n][3] (payload, strength, grav_z) and the draw counters [n]; synchronous.  set_params refuses a record that is
 * not finite, a strength below 0 and, with a mass table (h_mass [n]: each robot's nominal mass; NULL: unchecked), a payload that leaves a mass
 * that is not positive. */
int mpc_plant_rand_get_params(mpc_plant_rand *h, double *h_params);
int mpc_plant_rand_set_params(mpc_plant_rand *h, const double *h_params, const double *h_mass);
int mpc_plant_rand_get_counters(mpc_plant_rand *h, unsigned int *h_counters);
int mpc_plant_rand_set_counters(mpc_plant_rand *h, const unsigned int *h_counters);
const char *mpc_plant_rand_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_PLANT_RAND_H */
