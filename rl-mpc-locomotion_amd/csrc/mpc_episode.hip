// mpc_episode.hip -- the C ABI of include/mpc_episode.h: rsl_rl's per-tick episode bookkeeping (episode_stats.h) on the device.  A tick is an
// ordered compaction into a ring: every finished environment needs the tick's total and its own rank before anything is written, so the work
// is three phases with a dependency between workgroups at each boundary, and the boundaries are launch boundaries (no atomics, no workgroup
// waits on another):
//   phase a   one lane per environment: the two accumulations; per wave a ballot of the finished lanes, then per totals block (overall, each
//             group) popcounts and a fixed butterfly sum of return (float64) and length (int64); the waves of a workgroup are joined in wave order
//             through LDS and the workgroup writes one partial per block to the workspace.  A wave with nobody finished (most waves of most
//             ticks) only writes zeros.
//   phase b   ONE workgroup, lane s owns totals block s: it walks the workgroups' partials in index order, adds them to the totals and (lane 0)
//             publishes each workgroup's offset, the tick's total and the head before the tick, then advances head and count.
//   phase c   one lane per environment: rank = workgroup offset + waves before it + lanes before it (ballot), slot by episode::slot_of, the entry,
//             and the zeroing.  A tick with total 0 returns at once.
// accumulate_kernel / scan_kernel / place_kernel are the three launches (one workgroup walking n twice through the same phases was measured and is
// slower at n = 4096: tools/variants/).  summary_kernel (one workgroup) is launched when the summary is asked for, not per tick.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mpc_episode.h"
#include "episode_stats.h"
#include "mpc_host.h"

using mpchost::DeviceGuard;
using mpchost::round16;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kWave = 64;
constexpr int kGridThreads = 256;      // 4096 environments are 16 workgroups
constexpr int kWaves = kGridThreads / kWave;
constexpr int kSummaryThreads = 256;
constexpr int kBlocks = 1 + MPC_EPISODE_MAX_GROUPS;

// what one wave / one workgroup found finished on this tick, for one totals block
struct Part {
  long long sum_length;
  double sum_return;
  int count, timeouts;
};

struct Tick {
  int n, cap, num_groups;
  mpc_episode_buffers_t buf;
  const float *rew;
  const long long *reset, *timeout;
  Part *parts;                         // workspace [workgroups][1 + G]
  int *offsets;                        // workspace [workgroups]: finished environments in the workgroups before this one
  long long *tick;                     // workspace [2]: the head before this tick, the tick's total
};

// butterfly sums: every lane ends with the same value, the order is fixed
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__global__ __launch_bounds__(kGridThreads) void accumulate_kernel(Tick a) {
  __shared__ Part parts[kWaves][kBlocks];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, vb = blockIdx.x;
  const long long i = (long long)vb * kGridThreads + tid;
  bool done = false, to = false;
  float r = 0.0f;
  int len = 0, block = 0;
  if (i < a.n) {
    r = a.buf.d_cur_return[i];
    len = a.buf.d_cur_length[i];
    episode::accumulate(r, len, a.rew[i]);
    a.buf.d_cur_return[i] = r;
    a.buf.d_cur_length[i] = len;
    const long long rs = a.reset[i];
    done = episode::finished(rs);
    to = episode::timed_out(rs, a.timeout[i]);
    block = episode::group_block(a.buf.d_groups ? a.buf.d_groups[i] : 0, a.num_groups);
  }
  const unsigned long long any = __ballot(done);
  if (any == 0) {
    for (int s = lane; s <= a.num_groups; s += kWave) parts[wave][s] = Part{0, 0.0, 0, 0};
  } else {
    for (int s = 0; s <= a.num_groups; ++s) {
      const bool p = done && (s == 0 || block == s);
      const unsigned long long m = __ballot(p);
      Part q{0, 0.0, 0, 0};
      if (m != 0) {                    // (wave-uniform)
        q.count = __popcll(m);
        q.timeouts = __popcll(__ballot(p && to));
        q.sum_length = wave_sum(p ? (long long)len : 0ll);
        q.sum_return = wave_sum(p ? (double)r : 0.0);
      }
      if (lane == 0) parts[wave][s] = q;
    }
  }
  __syncthreads();
  for (int s = tid; s <= a.num_groups; s += kGridThreads) {
    Part q = parts[0][s];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const Part &o = parts[w][s];
      q.count += o.count; q.timeouts += o.timeouts; q.sum_length += o.sum_length; q.sum_return += o.sum_return;
    }
    a.parts[(size_t)vb * (a.num_groups + 1) + s] = q;
  }
}

__global__ __launch_bounds__(kGridThreads) void scan_kernel(Tick a, int blocks) {
  for (int s = threadIdx.x; s <= a.num_groups; s += kGridThreads) {
    long long c = 0, t = 0, l = 0;
    double r = 0.0;
    for (int vb = 0; vb < blocks; ++vb) {
      const Part q = a.parts[(size_t)vb * (a.num_groups + 1) + s];
      if (s == 0) a.offsets[vb] = (int)c;
      c += q.count; t += q.timeouts; l += q.sum_length; r += q.sum_return;
    }
    long long *k = a.buf.d_counters + MPC_EPISODE_COUNTERS + MPC_EPISODE_COUNTER_STRIDE * s;
    k[MPC_EPISODE_C_EPISODES] += c;
    k[MPC_EPISODE_C_TIMEOUTS] += t;
    k[MPC_EPISODE_C_SUM_LENGTH] += l;
    a.buf.d_sums[s] += r;
    if (s == 0) {
      const long long head = a.buf.d_counters[MPC_EPISODE_HEAD];
      a.tick[0] = head;
      a.tick[1] = c;
      a.buf.d_counters[MPC_EPISODE_HEAD] = episode::next_head(head, c, a.cap);
      a.buf.d_counters[MPC_EPISODE_COUNT] = episode::next_count(a.buf.d_counters[MPC_EPISODE_COUNT], c, a.cap);
    }
  }
}

__global__ __launch_bounds__(kGridThreads) void place_kernel(Tick a) {
  __shared__ int wave_count[kWaves];
  const long long total = a.tick[1], head = a.tick[0];
  if (total == 0) return;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, vb = blockIdx.x;
  const long long i = (long long)vb * kGridThreads + tid;
  long long rs = 0;
  if (i < a.n) rs = a.reset[i];
  const bool done = episode::finished(rs);
  const unsigned long long m = __ballot(done);
  if (lane == 0) wave_count[wave] = __popcll(m);
  __syncthreads();
  if (done) {
    long long rank = a.offsets[vb];
    for (int w = 0; w < wave; ++w) rank += wave_count[w];
    rank += __popcll(m & ((1ull << lane) - 1ull));
    const long long slot = episode::slot_of(head, rank, total, a.cap);
    if (slot >= 0 && rank < total) {
      a.buf.d_win_return[slot] = a.buf.d_cur_return[i];
      a.buf.d_win_length[slot] = a.buf.d_cur_length[i];
      a.buf.d_win_timed_out[slot] = episode::timed_out(rs, a.timeout[i]) ? 1 : 0;
    }
    a.buf.d_cur_return[i] = 0.0f;
    a.buf.d_cur_length[i] = 0;
  }
}

// one workgroup: lane t sums slots t, t + 256, ... of the window in ascending slot index, a fixed-order LDS tree joins the 256 lanes (a fixed order,
// not one chain from slot 0 to the last)
__global__ __launch_bounds__(kSummaryThreads) void summary_kernel(int num_groups, mpc_episode_buffers_t buf) {
  __shared__ double tr[kSummaryThreads];
  __shared__ long long tl[kSummaryThreads], tt[kSummaryThreads];
  const int tid = threadIdx.x;
  const long long count = buf.d_counters[MPC_EPISODE_COUNT];
  double r = 0.0;
  long long l = 0, t = 0;
  for (long long s = tid; s < count; s += kSummaryThreads) {
    r += (double)buf.d_win_return[s];
    l += buf.d_win_length[s];
    t += buf.d_win_timed_out[s];
  }
  tr[tid] = r; tl[tid] = l; tt[tid] = t;
  __syncthreads();
  for (int s = kSummaryThreads / 2; s > 0; s >>= 1) {
    if (tid < s) { tr[tid] += tr[tid + s]; tl[tid] += tl[tid + s]; tt[tid] += tt[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    buf.d_summary[MPC_EPISODE_S_WINDOW_COUNT] = (double)count;
    buf.d_summary[MPC_EPISODE_S_MEAN_RETURN] = count > 0 ? tr[0] / (double)count : 0.0;
    buf.d_summary[MPC_EPISODE_S_MEAN_LENGTH] = count > 0 ? (double)tl[0] / (double)count : 0.0;
    buf.d_summary[MPC_EPISODE_S_WINDOW_TIMEOUTS] = (double)tt[0];
  }
  for (int s = tid; s <= num_groups; s += kSummaryThreads) {
    const long long *k = buf.d_counters + MPC_EPISODE_COUNTERS + MPC_EPISODE_COUNTER_STRIDE * s;
    double *o = buf.d_summary + MPC_EPISODE_SUMMARY_TOTALS + MPC_EPISODE_SUMMARY_STRIDE * s;
    o[MPC_EPISODE_T_EPISODES] = (double)k[MPC_EPISODE_C_EPISODES];
    o[MPC_EPISODE_T_TIMEOUTS] = (double)k[MPC_EPISODE_C_TIMEOUTS];
    o[MPC_EPISODE_T_SUM_RETURN] = buf.d_sums[s];
    o[MPC_EPISODE_T_SUM_LENGTH] = (double)k[MPC_EPISODE_C_SUM_LENGTH];
  }
}

__global__ __launch_bounds__(kGridThreads) void random_progress_kernel(long long *__restrict__ progress, int n, long long max_len, unsigned long long seed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) progress[i] = episode::random_progress(seed, (uint32_t)i, max_len);
}

}  // namespace

struct mpc_episode {
  int n = 0, cap = 0, num_groups = 0;
  mpc_episode_buffers_t buf{};
  mpchost::DeviceArray<char> workspace;        // one allocation, on `device`; the three below point into it
  Part *parts = nullptr;
  int *offsets = nullptr;
  long long *tick = nullptr;
  int device = -1;
  bool bound = false;
};

extern "C" {

const char *mpc_episode_last_error(void) { return g_err.c_str(); }

int mpc_episode_create(mpc_episode **out, int n, int cap, int num_groups) {
  if (!out) return fail(MPC_E_ARG, "mpc_episode_create: bad argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_episode_create: n must be at least 1");
  if (cap < 1) return fail(MPC_E_ARG, "mpc_episode_create: the window holds at least one entry");
  if (num_groups < 1 || num_groups > MPC_EPISODE_MAX_GROUPS) return fail(MPC_E_ARG, "mpc_episode_create: 1 .. 64 groups");
  mpc_episode *ep = new mpc_episode();
  ep->n = n; ep->cap = cap; ep->num_groups = num_groups;
  *out = ep;
  return MPC_OK;
}

void mpc_episode_destroy(mpc_episode *ep) { mpchost::destroy_handle(ep); }

int mpc_episode_bind(mpc_episode *ep, const mpc_episode_buffers_t *b) {
  if (!ep || !b) return fail(MPC_E_ARG, "mpc_episode_bind: bad argument");
  if (!b->d_cur_return || !b->d_cur_length || !b->d_win_return || !b->d_win_length || !b->d_win_timed_out || !b->d_counters || !b->d_sums || !b->d_summary)
    return fail(MPC_E_ARG, "mpc_episode_bind: every buffer but d_groups must be non-null");
  const int dev = mpchost::current_device();
  if (dev < 0) return fail(MPC_E_NODEVICE, "mpc_episode_bind: no HIP device");
  if (ep->workspace && ep->device != dev) {
    DeviceGuard guard_(ep->device);
    ep->workspace.reset();
  }
  if (!ep->workspace) {
    const size_t blocks = ((size_t)ep->n + kGridThreads - 1) / kGridThreads;
    const size_t parts = round16(blocks * (size_t)(ep->num_groups + 1) * sizeof(Part)), offsets = round16(blocks * sizeof(int));
    HIP_TRY(ep->workspace.alloc(parts + offsets + 2 * sizeof(long long)));
    char *w = ep->workspace;
    ep->parts = reinterpret_cast<Part *>(w);
    ep->offsets = reinterpret_cast<int *>(w + parts);
    ep->tick = reinterpret_cast<long long *>(w + parts + offsets);
  }
  ep->buf = *b;
  ep->device = dev;
  ep->bound = true;
  return MPC_OK;
}

int mpc_episode_add(mpc_episode *ep, const float *d_rew, const long long *d_reset, const long long *d_timeout, void *stream) {
  if (!ep || !d_rew || !d_reset || !d_timeout) return fail(MPC_E_ARG, "mpc_episode_add: bad argument");
  if (!ep->bound) return fail(MPC_E_ARG, "mpc_episode_add: no buffers bound (mpc_episode_bind)");
  DeviceGuard guard_(ep->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Tick a{ep->n, ep->cap, ep->num_groups, ep->buf, d_rew, d_reset, d_timeout, ep->parts, ep->offsets, ep->tick};
  const int blocks = (ep->n + kGridThreads - 1) / kGridThreads;
  hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)blocks), dim3(kGridThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kGridThreads), 0, s, a, blocks);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(place_kernel, dim3((unsigned)blocks), dim3(kGridThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_episode_summary(mpc_episode *ep, void *stream) {
  if (!ep) return fail(MPC_E_ARG, "mpc_episode_summary: bad argument");
  if (!ep->bound) return fail(MPC_E_ARG, "mpc_episode_summary: no buffers bound (mpc_episode_bind)");
  DeviceGuard guard_(ep->device);
  hipLaunchKernelGGL(summary_kernel, dim3(1), dim3(kSummaryThreads), 0, reinterpret_cast<hipStream_t>(stream), ep->num_groups, ep->buf);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_episode_restart(mpc_episode *ep, void *stream) {
  if (!ep) return fail(MPC_E_ARG, "mpc_episode_restart: bad argument");
  if (!ep->bound) return fail(MPC_E_ARG, "mpc_episode_restart: no buffers bound (mpc_episode_bind)");
  DeviceGuard guard_(ep->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(ep->buf.d_cur_return, 0, (size_t)ep->n * sizeof(float), s));
  HIP_TRY(hipMemsetAsync(ep->buf.d_cur_length, 0, (size_t)ep->n * sizeof(int), s));
  return MPC_OK;
}

int mpc_episode_clear(mpc_episode *ep, void *stream) {
  if (int rc = mpc_episode_restart(ep, stream))          // (a HIP error keeps its own text)
    return rc == MPC_E_ARG ? fail(rc, "mpc_episode_clear: bad argument or no buffers bound (mpc_episode_bind)") : rc;
  DeviceGuard guard_(ep->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t blocks = (size_t)ep->num_groups + 1;
  HIP_TRY(hipMemsetAsync(ep->buf.d_win_return, 0, (size_t)ep->cap * sizeof(float), s));
  HIP_TRY(hipMemsetAsync(ep->buf.d_win_length, 0, (size_t)ep->cap * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(ep->buf.d_win_timed_out, 0, (size_t)ep->cap * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(ep->buf.d_counters, 0, (MPC_EPISODE_COUNTERS + MPC_EPISODE_COUNTER_STRIDE * blocks) * sizeof(long long), s));
  HIP_TRY(hipMemsetAsync(ep->buf.d_sums, 0, blocks * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(ep->buf.d_summary, 0, (MPC_EPISODE_SUMMARY_TOTALS + MPC_EPISODE_SUMMARY_STRIDE * blocks) * sizeof(double), s));
  return MPC_OK;
}

int mpc_episode_random_progress(long long *d_progress, int n, long long max_len, unsigned long long seed, void *stream) {
  if (!d_progress || n < 1) return fail(MPC_E_ARG, "mpc_episode_random_progress: bad argument");
  if (max_len < 1 || max_len > (1ll << 31)) return fail(MPC_E_ARG, "mpc_episode_random_progress: max_len must lie in [1, 2^31]");
  hipLaunchKernelGGL(random_progress_kernel, dim3((unsigned)((n + kGridThreads - 1) / kGridThreads)), dim3(kGridThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     d_progress, n, max_len, seed);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
