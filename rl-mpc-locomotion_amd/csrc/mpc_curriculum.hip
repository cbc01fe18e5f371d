// mpc_curriculum.hip -- the C ABI of mpc_curriculum.h: the terrain curriculum (terrain_curriculum.h) on the device, in two kernels.
//   curriculum_update_kernel    one lane per environment, one wave per workgroup like task_begin_kernel: the flag, two floats of the root state and
//                               two of the command in; the level, the counter and the two float64 words of the sim's origin out -- only where the
//                               flag is set.
//   curriculum_summary_kernel   ONE workgroup: per type a fixed stride loop per lane feeds a fixed-order LDS tree of integer sums (count, sum of
//                               levels); lane 0 adds the types up for the totals and writes float64 counts and means.  Integer sums are exact, so
//                               the order is not a numerical question; the fixed order keeps the unit free of atomics like the rest of the library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "mpc_curriculum.h"
#include "mpc_host.h"
#include "mpc_sim_internal.h"
#include "terrain_curriculum.h"

using curriculum::Config;
using mpchost::DeviceGuard;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kUpdateThreads = 64;     // one wave per workgroup: 4096 environments are 64 waves
constexpr int kSummaryThreads = 256;

__global__ __launch_bounds__(kUpdateThreads) void curriculum_update_kernel(Config c, int n, const long long *__restrict__ reset,
                                                                           const float *__restrict__ root, const float *__restrict__ commands,
                                                                           const int *__restrict__ type, const double *__restrict__ tiles,
                                                                           int *level, int *count, double *origin) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (reset[r] == 0) return;
  const float xy[2] = {root[(size_t)r * 13], root[(size_t)r * 13 + 1]};
  const float cmd[2] = {commands[(size_t)r * 3], commands[(size_t)r * 3 + 1]};
  int lv = level[r], k = count[r];
  double o[2];
  curriculum::update_env(c, r, xy, cmd, type[r], tiles, lv, k, o);
  level[r] = lv;
  count[r] = k;
  origin[2 * (size_t)r] = o[0];
  origin[2 * (size_t)r + 1] = o[1];
}

__global__ __launch_bounds__(kSummaryThreads) void curriculum_summary_kernel(int n, int num_types, const int *__restrict__ level,
                                                                             const int *__restrict__ type, double *out) {
  __shared__ long long cnt[kSummaryThreads], sum[kSummaryThreads];
  const int tid = threadIdx.x;
  long long total_n = 0, total_sum = 0;                  // (lane 0's)
  for (int t = 0; t < num_types; ++t) {
    long long a = 0, b = 0;
    for (int r = tid; r < n; r += kSummaryThreads)
      if (type[r] == t) { a += 1; b += level[r]; }
    cnt[tid] = a;
    sum[tid] = b;
    __syncthreads();
    for (int w = kSummaryThreads / 2; w > 0; w >>= 1) {
      if (tid < w) { cnt[tid] += cnt[tid + w]; sum[tid] += sum[tid + w]; }
      __syncthreads();
    }
    if (tid == 0) {
      const long long ct = cnt[0], st = sum[0];
      total_n += ct;
      total_sum += st;
      out[2 + t] = (double)ct;
      out[2 + num_types + t] = ct > 0 ? (double)st / (double)ct : 0.0;
    }
    __syncthreads();                                     // lane 0 has read the roots before the next type overwrites them
  }
  if (tid == 0) {
    out[0] = (double)total_n;
    out[1] = total_n > 0 ? (double)total_sum / (double)total_n : 0.0;
  }
}
}  // namespace

struct mpc_curriculum {
  int n = 0, device = 0;
  Config c{};
  mpchost::DeviceArray<int> d_level, d_count, d_type;                  // [n] each
  mpchost::DeviceArray<double> d_tiles;                                // [num_levels][num_types][2]
  double *d_origin = nullptr;                                          // the bound sim's own array [n][2]
};

extern "C" {

const char *mpc_curriculum_last_error(void) { return g_err.c_str(); }

void mpc_curriculum_destroy(mpc_curriculum *c) { mpchost::destroy_handle(c); }

int mpc_curriculum_create(mpc_curriculum **out, int n, int num_levels, int num_types, const double *h_tile_origins, const int *h_levels0,
                          const int *h_types, double env_length, double episode_length_s, unsigned long long seed) {
  // everything is validated before the device is touched
  if (!out || !h_tile_origins || !h_levels0 || !h_types) return fail(MPC_E_ARG, "mpc_curriculum_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_curriculum_create: n must be at least 1");
  if (num_levels < 1 || num_types < 1) return fail(MPC_E_ARG, "mpc_curriculum_create: num_levels and num_types must be at least 1");
  if (!std::isfinite(env_length) || !(env_length > 0.0)) return fail(MPC_E_ARG, "mpc_curriculum_create: env_length must be finite and > 0");
  if (!std::isfinite(episode_length_s) || !(episode_length_s >= 0.0))      // (0 is allowed: then nobody is ever demoted)
    return fail(MPC_E_ARG, "mpc_curriculum_create: episode_length_s must be finite and >= 0");
  const size_t tiles = (size_t)num_levels * (size_t)num_types;
  for (size_t i = 0; i < 2 * tiles; ++i)
    if (!std::isfinite(h_tile_origins[i])) return fail(MPC_E_ARG, "mpc_curriculum_create: origin of tile " + std::to_string(i / 2) + " is not finite");
  for (int r = 0; r < n; ++r) {
    if (h_levels0[r] < 0 || h_levels0[r] >= num_levels)
      return fail(MPC_E_ARG, "mpc_curriculum_create: level of environment " + std::to_string(r) + " outside [0, num_levels)");
    if (h_types[r] < 0 || h_types[r] >= num_types)
      return fail(MPC_E_ARG, "mpc_curriculum_create: type of environment " + std::to_string(r) + " outside [0, num_types)");
  }
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_curriculum_create: no HIP device");
  mpc_curriculum *c = new mpc_curriculum();
  c->n = n;
  c->device = device;
  c->c = Config{num_levels, num_types, (float)(env_length / 2.0), (float)episode_length_s, seed};
  hipError_t e;
  if ((e = c->d_level.alloc_copy(h_levels0, (size_t)n)) != hipSuccess || (e = c->d_count.alloc_zero((size_t)n)) != hipSuccess ||
      (e = c->d_type.alloc_copy(h_types, (size_t)n)) != hipSuccess || (e = c->d_tiles.alloc_copy(h_tile_origins, 2 * tiles)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess) {
    mpc_curriculum_destroy(c);
    return fail(MPC_E_HIP, std::string("mpc_curriculum_create: ") + hipGetErrorString(e));
  }
  *out = c;
  return MPC_OK;
}

int mpc_curriculum_bind(mpc_curriculum *c, mpc_sim *s) {
  if (!c) return fail(MPC_E_ARG, "mpc_curriculum_bind: null curriculum handle");
  if (!s) return fail(MPC_E_ARG, "mpc_curriculum_bind: null sim handle");
  if (!s->d_heights || !s->d_origin) return fail(MPC_E_ARG, "mpc_curriculum_bind: the sim has no terrain attached");
  if (s->n != c->n)
    return fail(MPC_E_ARG, "mpc_curriculum_bind: the sim has " + std::to_string(s->n) + " robots, the curriculum " + std::to_string(c->n) + " environments");
  if (s->device != c->device) return fail(MPC_E_ARG, "mpc_curriculum_bind: the sim lives on another device");
  c->d_origin = s->d_origin;
  return MPC_OK;
}

int mpc_curriculum_update(mpc_curriculum *c, const long long *d_reset, const float *d_root, const float *d_commands, void *stream) {
  if (!c || !d_reset || !d_root || !d_commands) return fail(MPC_E_ARG, "mpc_curriculum_update: bad argument");
  if (!c->d_origin) return fail(MPC_E_ARG, "mpc_curriculum_update: no sim bound (mpc_curriculum_bind)");
  DeviceGuard guard_(c->device);
  hipLaunchKernelGGL(curriculum_update_kernel, dim3((unsigned)((c->n + kUpdateThreads - 1) / kUpdateThreads)), dim3(kUpdateThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), c->c, c->n, d_reset, d_root, d_commands, c->d_type, c->d_tiles, c->d_level, c->d_count,
                     c->d_origin);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_curriculum_summary(mpc_curriculum *c, double *d_out, void *stream) {
  if (!c || !d_out) return fail(MPC_E_ARG, "mpc_curriculum_summary: bad argument");
  DeviceGuard guard_(c->device);
  hipLaunchKernelGGL(curriculum_summary_kernel, dim3(1), dim3(kSummaryThreads), 0, reinterpret_cast<hipStream_t>(stream), c->n, c->c.num_types,
                     c->d_level, c->d_type, d_out);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_curriculum_levels(mpc_curriculum *c, int **d_levels) {
  if (!c || !d_levels) return fail(MPC_E_ARG, "mpc_curriculum_levels: bad argument");
  *d_levels = c->d_level;
  return MPC_OK;
}

int mpc_curriculum_counts(mpc_curriculum *c, int **d_counts) {
  if (!c || !d_counts) return fail(MPC_E_ARG, "mpc_curriculum_counts: bad argument");
  *d_counts = c->d_count;
  return MPC_OK;
}

}  // extern "C"
