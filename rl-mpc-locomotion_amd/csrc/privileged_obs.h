// privileged_obs.h -- the arithmetic of the critic's privileged observation row (mpc_privileged_obs.h), for the device kernel and for a host compiler.
//
// legged_gym's privileged observations restated for this task: what the critic may see and the actor may not.  One float32 row per environment:
//
//   columns 0 .. 47            the task's 48 observation columns, as they stood BEFORE any observation noise
//   columns 48 .. 48 + P - 1   the height scan's P columns as the scan wrote them into the wide row, before noise (P = 0 without a scan)
//   four columns               the plant's foot-contact flags FL FR RL RR as 0.0 / 1.0
//   one column                 the episode phase: float32(progress) * inv_len, inv_len = float32(1 / max_episode_length) computed by the host
//                              (a multiply, not a divide: the same bits whatever the build does with divisions)
//   zeros                      up to width(P) = 16 * ceil((48 + P + 5) / 16)
//
// With the plant's per-robot record (mpc_plant_rand.h: payload, strength, grav_z as float64 [3][n]) three columns follow the phase:
//   (float)payload    (float)(strength - 1.0)    (float)(grav_z - kGravZ)          one float64 subtraction (none for the first), one conversion
// and the zeros run up to width_plant(P) = 16 * ceil((48 + P + 5 + 3) / 16).
//
// The first 48 + P columns are copies and the rest are conversions and one correctly rounded product, so the row is restated bit for bit in numpy
// (tests/privileged_obs_ref.py).
#pragma once

#ifdef __HIPCC__
#define PRIVOBS_HD __host__ __device__
#else
#define PRIVOBS_HD
#endif

namespace privobs {

constexpr int kTaskObs = 48;           // rl_task.h's observation row
constexpr int kContacts = 4;           // FL FR RL RR
constexpr int kExtra = kContacts + 1;  // the contacts and the phase
constexpr int kMaxScan = 208;          // MPC_HSCAN_MAX_POINTS
constexpr int kPlantCols = 3;          // payload, strength - 1, grav_z - kGravZ
constexpr double kGravZ = -9.81;       // toy_sim.h's

PRIVOBS_HD inline int width(int P) { return 16 * ((kTaskObs + P + kExtra + 15) / 16); }

PRIVOBS_HD inline float contact_flag(int contact) { return contact != 0 ? 1.0f : 0.0f; }

PRIVOBS_HD inline float phase(long long progress, float inv_len) { return (float)progress * inv_len; }

// Column `col` >= live (= 48 + P) of environment r's row: `contact` is the sim's int32 record [..][n] (entry l of robot r at contact[l * n + r])
PRIVOBS_HD inline float tail_column(int col, int live, const int *contact, int n, int r, long long progress, float inv_len) {
  const int k = col - live;
  if (k < kContacts) return contact_flag(contact[(long)k * n + r]);
  if (k == kContacts) return phase(progress, inv_len);
  return 0.0f;                         // the pad
}

PRIVOBS_HD inline int width_plant(int P) { return 16 * ((kTaskObs + P + kExtra + kPlantCols + 15) / 16); }

// Plant column j of environment r: `plant` is the sim's float64 record [3][n] (entry j of robot r at plant[j * n + r])
PRIVOBS_HD inline float plant_column(int j, const double *plant, int n, int r) {
  const double v = plant[(long)j * n + r];
  return j == 0 ? (float)v : (j == 1 ? (float)(v - 1.0) : (float)(v - kGravZ));
}

// tail_column for a row with the plant columns
PRIVOBS_HD inline float tail_column_plant(int col, int live, const int *contact, const double *plant, int n, int r, long long progress, float inv_len) {
  const int k = col - live;
  if (k < kExtra) return tail_column(col, live, contact, n, r, progress, inv_len);
  if (k < kExtra + kPlantCols) return plant_column(k - kExtra, plant, n, r);
  return 0.0f;                         // the pad
}

}  // namespace privobs
