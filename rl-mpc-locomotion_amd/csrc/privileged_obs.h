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

}  // namespace privobs
