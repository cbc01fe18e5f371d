/*
 * mpc_curriculum.h -- the C ABI of the device-side terrain curriculum (mpc_curriculum.hip, terrain_curriculum.h), and the two entry points
 * that hand out an mpc_sim's origin array (mpc_terrain.hip).
 *
 * A curriculum holds, for n environments on a grid of num_levels x num_types terrain tiles, each environment's level and type and the tiles'
 * centres.  mpc_curriculum_update runs between the plant's step and the task's `begin`: for every environment whose reset flag is set it
 * promotes or demotes the level by how far the robot has walked (terrain_curriculum.h) and writes the new tile's centre into the bound sim's
 * origin array, so that the reset which follows re-initialises the robot standing there.  Environments whose flag is clear are neither read nor
 * written.  Stream-ordered, no host read, no atomics.
 *
 * This header lives beside the sources and not under include/: tests/test_abi.py keeps a table of every header under include/ and
 * tests/test_toy_terrain.py counts the entry points of include/mpc_terrain.h, and both are fixed.
 *
 * Pointers named d_* are DEVICE pointers, h_* HOST pointers; `stream` is a hipStream_t.  Functions return 0 (MPC_OK) or a negative MPC_E_*
 * code of include/mpc_batch.h; mpc_curriculum_last_error() (mpc_terrain_last_error() for the two mpc_terrain_* entry points) gives the text.
 */
#ifndef MPC_CURRICULUM_H
#define MPC_CURRICULUM_H

#include "../../include/mpc_terrain.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_curriculum mpc_curriculum;

/* h_tile_origins [num_levels][num_types][2], h_levels0 [n] in [0, num_levels), h_types [n] in [0, num_types).  MPC_E_ARG, before the device is
 * touched, for a null pointer, n < 1, num_levels < 1, num_types < 1, a level or type out of range, an origin that is not finite, an
 * env_length that is not finite and > 0, or an episode_length_s that is not finite and >= 0 (0: nobody is ever demoted).  Synchronous. */
int mpc_curriculum_create(mpc_curriculum **out, int n, int num_levels, int num_types, const double *h_tile_origins, const int *h_levels0,
                          const int *h_types, double env_length, double episode_length_s, unsigned long long seed);
void mpc_curriculum_destroy(mpc_curriculum *c);
/* Keep the device address of s's own origin array.  MPC_E_ARG for a sim without a terrain, of another size or on another device.  A sim
 * whose terrain is attached again has a new array: bind again. */
int mpc_curriculum_bind(mpc_curriculum *c, mpc_sim *s);
/* d_reset [n] int64 (the flags `begin` is about to consume), d_root [n][13] float32 (the plant's root states, before the reset), d_commands
 * [n][3] float32 (the finished episode's). */
int mpc_curriculum_update(mpc_curriculum *c, const long long *d_reset, const float *d_root, const float *d_commands, void *stream);
/* d_out [2 + 2 num_types] float64: n, the mean level, then per type the count of its environments and then per type their mean level (0.0
 * for a type without environments).  Integer sums, so exact. */
int mpc_curriculum_summary(mpc_curriculum *c, double *d_out, void *stream);
/* the device array of levels [n] int32, for a tensor view */
int mpc_curriculum_levels(mpc_curriculum *c, int **d_levels);
/* the device array of reset counters [n] int32 (how many resets the curriculum has seen of each environment: the redraw's key), for tests */
int mpc_curriculum_counts(mpc_curriculum *c, int **d_counts);
const char *mpc_curriculum_last_error(void);

/* (mpc_terrain.hip) the device address of s's origin array [n][2] float64; MPC_E_ARG for a sim without a terrain */
int mpc_terrain_origins(mpc_sim *s, double **d_origin);
/* the origins on the host, h_origin [n][2]; synchronous (waits for the device) */
int mpc_terrain_get_origins(mpc_sim *s, double *h_origin);

#ifdef __cplusplus
}
#endif

#endif /* MPC_CURRICULUM_H */
