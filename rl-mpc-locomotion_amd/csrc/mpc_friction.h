/*
 * mpc_friction.h -- the C ABI of the opt-in Coulomb friction of the toy plant (mpc_friction.hip, friction.h, toy_sim.h's Coulomb contact): every
 * robot of a toy-plant sim gets a friction coefficient of its own, its stance feet slide where the leg asks for more tangential force than
 * mu times the normal force, and the step publishes each foot's ground reaction and slip.
 *
 * mpc_friction_attach gives a sim (include/mpc_sim.h) its friction record, mu float64 [n] (+inf: the anchor holds, the plant of a sim without
 * the record), and from then on mpc_sim_step launches the Coulomb step kernel of the sim's ground.  That kernel steps with the sim's plant
 * record (mpc_plant_rand.h) where one is attached -- before or after this call -- and with the neutral one (0, 1, -9.81) where not.  With
 * mu = +inf it computes what the sim's previous kernel computes, bit for bit.  A sim without a friction record launches the kernels it launched
 * before.  Every step also writes, where the caller gave the arrays, d_force float32 [n][4][3] -- the world-frame ground reaction on each foot
 * in the tick's last substep, in newtons; zero for a leg in the air, a leg that let go and a leg that would pull -- and d_slip float32 [n][4],
 * the distance each foot slid over the tick's substeps, in metres.  A fallen (frozen) robot's rows are written as zeros.
 *
 * An mpc_friction handle owns the seed and the draw counters.  mpc_friction_draw is one kernel with one lane per slot of d_ids: a listed
 * environment r has its force and slip rows zeroed and, where `resample` is set, takes e = counter[r], draws
 *     u = uniform01(seed ^ domain, r, e, 0)
 *     mu = fminf(lo + (hi - lo) * u, hi)                                          buckets == 0
 *     mu = fminf(lo + ((hi - lo) * floorf(u * buckets)) / (buckets - 1), hi)      buckets >= 2 (legged_gym's friction buckets)
 * in float32, stores (double)mu and counter[r] = e + 1.  Counter-based draws: nothing depends on n.  Stream-ordered; no host read, no atomics,
 * no LDS.
 *
 * This header lives beside the sources and not under include/, like mpc_plant_rand.h.
 *
 * Pointers named d_* are DEVICE pointers, h_* HOST pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_* code
 * of include/mpc_batch.h; mpc_friction_last_error() gives the text.  Every call validates its arguments before the device is touched.
 */
#ifndef MPC_FRICTION_H
#define MPC_FRICTION_H

#include "../../include/mpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_friction mpc_friction;

/* Give s its friction record: h_mu [n] float64, each >= 0 and not NaN (+inf allowed), or NULL for +inf everywhere; d_force [n][4][3] and
 * d_slip [n][4] float32, the caller's, either may be NULL, and must outlive the sim's last step.  Once per sim: MPC_E_ARG for a sim that has a
 * record already, a null sim, a negative or NaN mu. */
int mpc_friction_attach(mpc_sim *s, const double *h_mu, float *d_force, float *d_slip);
/* n environments, the seed of every draw.  A host-only handle until mpc_friction_bind.  MPC_E_ARG for a null pointer or n < 1. */
int mpc_friction_create(mpc_friction **out, int n, unsigned long long seed);
void mpc_friction_destroy(mpc_friction *h);
/* Point the handle at s's friction record (s must outlive the handle's last call) and allocate its draw counters uint32 [n], zero.  MPC_E_ARG
 * for a sim of another size, a sim without a friction record and a handle that is bound already. */
int mpc_friction_bind(mpc_friction *h, mpc_sim *s);
/* d_ids [k] int32: r where environment r is listed, anything outside [0, n) (the task's -1) is skipped; NULL: all n environments (k must be n).
 * The ids must be distinct.  lo, hi: the range, rounded to float32, finite, 0 <= lo <= hi; buckets: 0 or >= 2; both read only where resample
 * is non-zero, and checked first, before the handle is looked at.  MPC_E_ARG otherwise, and before mpc_friction_bind. */
int mpc_friction_draw(mpc_friction *h, const int *d_ids, int k, double lo, double hi, int buckets, int resample, void *stream);
/* mu as a host array [n] and the draw counters [n]; synchronous.  set_mu refuses a negative or NaN entry. */
int mpc_friction_get_mu(mpc_friction *h, double *h_mu);
int mpc_friction_set_mu(mpc_friction *h, const double *h_mu);
int mpc_friction_get_counters(mpc_friction *h, unsigned int *h_counters);
int mpc_friction_set_counters(mpc_friction *h, const unsigned int *h_counters);
const char *mpc_friction_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MPC_FRICTION_H */
