// episode_stats.h -- the per-environment arithmetic and the slot rule of the device-side episode statistics, shared by the device kernels
// (mpc_episode.hip, include/mpc_episode.h) and host C++ (the CPU tests compile this header with g++ and drive it against tests/episode_ref.py).
//
// What it restates: the bookkeeping of rsl_rl v1.0.2's OnPolicyRunner.learn, by its published lines (rsl_rl's source is not in the reference tree):
//   cur_reward_sum += rewards; cur_episode_length += 1
//   new_ids = (dones > 0).nonzero(); rewbuffer.extend(cur_reward_sum[new_ids]...); lenbuffer.extend(cur_episode_length[new_ids]...)
//   cur_reward_sum[new_ids] = 0; cur_episode_length[new_ids] = 0
// with rewbuffer / lenbuffer = deque(maxlen=cap).  The return is one float32 add per tick, the length an integer.
//
// The deque as a ring: `head` is the slot the next entry goes to.  On a tick that finishes `total` environments, the one with `rank` finished
// environments of lower index before it goes to (head + rank) mod cap -- unless rank < total - cap: a deque extended by more than maxlen keeps
// the last maxlen, and dropping the others here gives every slot exactly one writer.  Then head = (head + total) mod cap and the count grows by
// total up to cap.  In deque order the window is slots 0 .. count-1 while count < cap and head, head + 1, ... (mod cap) once it is full.
//
// random_progress is rsl_rl's init_at_random_ep_len (torch.randint_like(episode_length_buf, high=max_episode_length)) through rl_task.h's
// counter-based generator: a function of (seed, environment) alone, so a draw does not depend on the batch size; parity with torch in
// distribution only.
#pragma once

#include <stdint.h>

#include "rl_task.h"

namespace episode {

constexpr uint64_t kProgressDomain = 0x45505F50524F4752ull;   // keeps these draws apart from the command and the noise draws of the same seed

// cur_reward_sum += rewards; cur_episode_length += 1
MPC_HD void accumulate(float &cur_return, int &cur_length, float rew) {
  cur_return = cur_return + rew;
  cur_length = cur_length + 1;
}

MPC_HD bool finished(long long reset) { return reset > 0; }
MPC_HD bool timed_out(long long reset, long long time_out) { return reset > 0 && time_out > 0; }

// the totals block an environment counts in besides the overall one: 1 + g, or 0 (none) for a group id outside [0, G)
MPC_HD int group_block(int g, int num_groups) { return (g >= 0 && g < num_groups) ? 1 + g : 0; }

// the ring slot of the finished environment of rank `rank` (0 <= rank < total) on a tick that finishes `total`, or -1 when the deque would have
// pushed it out again within the same extend
MPC_HD long long slot_of(long long head, long long rank, long long total, long long cap) {
  if (rank < total - cap) return -1;
  return (head + rank) % cap;
}

MPC_HD long long next_head(long long head, long long total, long long cap) { return (head + total) % cap; }
MPC_HD long long next_count(long long count, long long total, long long cap) { return count + total < cap ? count + total : cap; }

// an integer uniform on [0, max_len), 1 <= max_len <= 2^31: the high 32 bits of one 64-bit word, multiplied and shifted (the bias of a value is
// below max_len / 2^32)
MPC_HD long long random_progress(uint64_t seed, uint32_t env, long long max_len) {
  const uint64_t k = rltask::mix64((seed ^ kProgressDomain) + 0x9E3779B97F4A7C15ull);
  const uint64_t x = rltask::mix64(k ^ rltask::mix64((uint64_t)env + 0x9E3779B97F4A7C15ull));
  return (long long)(((x >> 32) * (uint64_t)max_len) >> 32);
}

// ---- the host statement of one tick: what the device kernels compute in three phases, walked serially ---------------------------------------
struct Totals {
  long long episodes, timeouts, sum_length;
  double sum_return;
};

struct State {
  int n, cap, num_groups;
  float *cur_return;          // [n]
  int *cur_length;            // [n]
  float *win_return;          // [cap]
  int *win_length, *win_timed_out;
  long long head, count;
  Totals *totals;             // [1 + num_groups]: overall, then per group
  const int *groups;          // [n] or null
};

inline void tick(State &s, const float *rew, const long long *reset, const long long *time_outs) {
  long long total = 0;
  for (int i = 0; i < s.n; ++i) {
    accumulate(s.cur_return[i], s.cur_length[i], rew[i]);
    total += finished(reset[i]) ? 1 : 0;
  }
  long long rank = 0;
  for (int i = 0; i < s.n; ++i) {
    if (!finished(reset[i])) continue;
    const bool to = timed_out(reset[i], time_outs[i]);
    const int blocks[2] = {0, group_block(s.groups ? s.groups[i] : 0, s.num_groups)};
    for (int b = 0; b < 2; ++b) {
      if (b == 1 && blocks[b] == 0) continue;
      Totals &t = s.totals[blocks[b]];
      t.episodes += 1;
      t.timeouts += to ? 1 : 0;
      t.sum_length += s.cur_length[i];
      t.sum_return += (double)s.cur_return[i];
    }
    const long long slot = slot_of(s.head, rank, total, s.cap);
    if (slot >= 0) {
      s.win_return[slot] = s.cur_return[i];
      s.win_length[slot] = s.cur_length[i];
      s.win_timed_out[slot] = to ? 1 : 0;
    }
    s.cur_return[i] = 0.0f;
    s.cur_length[i] = 0;
    ++rank;
  }
  s.head = next_head(s.head, total, s.cap);
  s.count = next_count(s.count, total, s.cap);
}

}  // namespace episode
