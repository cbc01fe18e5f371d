// mpc_obs_norm.hip -- the C ABI of include/mpc_obs_norm.h: rsl_rl 2.x's EmpiricalNormalization (obs_norm.h) on the device.  An updating call is
// three phases with a dependency between workgroups at each boundary, and the boundaries are launch boundaries (no atomics, no workgroup waits
// on another, nobody reads a state that another workgroup is writing):
//   partial_kernel     a grid over blocks of kBlockRows rows.  A block's rows are one contiguous run of rows * D floats: the workgroup loads it with
//                      consecutive lanes on consecutive words into an LDS tile whose row stride is padded to an odd number of words; lane r of the
//                      first wave walks row r for a non-finite entry and a ballot makes the mask of the rows in use; then lane c walks column c
//                      twice (the mean, the squared deviations) and writes (mean, M2) to the workspace, column-major within the block so that
//                      the stores and the next phase's loads are coalesced too.  The rows in use are one count per block.
//   merge_kernel       ONE workgroup, lane c owns column c: it joins the blocks' partials in index order (loaded sixteen at a time, so that the
//                      chain of joins does not wait for one load per link), merges the result into the running state and publishes the float32
//                      buffers -- unless the count had reached `until`, or no row was in use.
//   normalize_kernel   a grid over the same blocks of rows: y = (x - mean) / (std + eps) with the published buffers, element by element (the
//                      thread that reads an element writes it: in place is safe).
// update = 0 is normalize_kernel alone.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mpc_obs_norm.h"
#include "mpc_host.h"
#include "obs_norm.h"

static_assert(MPC_OBSNORM_MAX_OBS == obs_norm::kMaxObs && MPC_OBSNORM_BLOCK_ROWS == obs_norm::kBlockRows, "include/mpc_obs_norm.h and obs_norm.h disagree");

using mpchost::DeviceGuard;
using mpchost::round16;

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

using obs_norm::kBlockRows;
using obs_norm::kMaxObs;
using obs_norm::Moments;

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kTileWords = kBlockRows * (kMaxObs | 1);          // 32 rows of at most 257 words: 32.1 KiB
constexpr int kLoadBatch = 16;

struct Call {
  int D;
  long long n;
  const float *x;
  float *y;
  float eps;
  long long until;
  mpc_obsnorm_buffers_t buf;
  long long *part_n;          // workspace [blocks]: rows in use
  double *part_mean;          // workspace [blocks][D]
  double *part_m2;            // workspace [blocks][D]
};

__device__ __forceinline__ int rows_of(const Call &a, long long block) {
  const long long left = a.n - block * kBlockRows;
  return (int)(left < kBlockRows ? left : kBlockRows);
}

__global__ __launch_bounds__(kThreads) void partial_kernel(Call a) {
  __shared__ float tile[kTileWords];
  __shared__ uint32_t used_mask;
  const int tid = threadIdx.x, D = a.D, stride = obs_norm::padded_stride(D);
  const long long block = blockIdx.x;
  const int rows = rows_of(a, block), words = rows * D;
  const float *src = a.x + block * kBlockRows * (long long)D;
  for (int e = tid; e < words; e += kThreads) {
    const int r = e / D, c = e - r * D;
    tile[r * stride + c] = src[e];
  }
  __syncthreads();
  if (tid < kWave) {                   // kBlockRows <= kWave: the rows are lanes of the first wave
    const bool ok = tid < rows && obs_norm::row_is_finite(tile + tid * stride, D);
    const unsigned long long m = __ballot(ok);
    if (tid == 0) used_mask = (uint32_t)m;
  }
  __syncthreads();
  const uint32_t used = used_mask;
  if (tid == 0) a.part_n[block] = __popc(used);
  for (int c = tid; c < D; c += kThreads) {
    const Moments m = obs_norm::block_moments(tile + c, stride, rows, used);
    a.part_mean[block * D + c] = m.mean;
    a.part_m2[block * D + c] = m.m2;
  }
}

__global__ __launch_bounds__(kThreads) void merge_kernel(Call a, long long blocks) {
  const int tid = threadIdx.x, D = a.D;
  const long long count0 = a.buf.d_count[0];
  __syncthreads();                     // every lane has read the count before lane 0 rewrites it
  const bool skip = obs_norm::frozen(count0, a.until);
  long long used_rows = 0;
  for (int c = tid; c < D && !skip; c += kThreads) {
    Moments acc{0, 0.0, 0.0};
    for (long long b0 = 0; b0 < blocks; b0 += kLoadBatch) {
      long long pn[kLoadBatch];
      double pm[kLoadBatch], p2[kLoadBatch];
#pragma unroll
      for (int k = 0; k < kLoadBatch; ++k) {
        const long long b = b0 + k < blocks ? b0 + k : blocks - 1;       // (a repeated load, not a branch; the join below skips it)
        pn[k] = a.part_n[b];
        pm[k] = a.part_mean[b * D + c];
        p2[k] = a.part_m2[b * D + c];
      }
#pragma unroll
      for (int k = 0; k < kLoadBatch; ++k)
        if (b0 + k < blocks) acc = obs_norm::join(acc, Moments{pn[k], pm[k], p2[k]});
    }
    used_rows = acc.n;
    if (acc.n > 0) {
      double mean = a.buf.d_state[c], var = a.buf.d_state[D + c];
      obs_norm::merge(mean, var, count0, acc);
      a.buf.d_state[c] = mean;
      a.buf.d_state[D + c] = var;
      a.buf.d_mean[c] = (float)mean;
      a.buf.d_var[c] = (float)var;
      a.buf.d_std[c] = (float)__builtin_sqrt(var);
    }
  }
  if (tid == 0 && used_rows > 0) a.buf.d_count[0] = count0 + used_rows;
}

__global__ __launch_bounds__(kThreads) void normalize_kernel(Call a) {
  const int D = a.D;
  const long long block = blockIdx.x, base = block * kBlockRows * (long long)D;
  const int words = rows_of(a, block) * D;
  for (int e = threadIdx.x; e < words; e += kThreads) {
    const int c = e % D;
    a.y[base + e] = obs_norm::normalize(a.x[base + e], a.buf.d_mean[c], a.buf.d_std[c], a.eps);
  }
}

__global__ __launch_bounds__(kThreads) void clear_kernel(int D, mpc_obsnorm_buffers_t buf) {
  for (int c = threadIdx.x; c < D; c += kThreads) {
    buf.d_state[c] = 0.0;
    buf.d_state[D + c] = 1.0;
    buf.d_mean[c] = 0.0f;
    buf.d_var[c] = 1.0f;
    buf.d_std[c] = 1.0f;
  }
  if (threadIdx.x == 0) buf.d_count[0] = 0;
}

}  // namespace

struct mpc_obsnorm {
  int D = 0;
  float eps = 0.0f;
  long long until = -1;
  mpc_obsnorm_buffers_t buf{};
  mpchost::DeviceArray<char> workspace;        // on `device`
  long long capacity = 0;              // blocks the workspace holds
  int device = -1;
  bool bound = false;
};

extern "C" {

const char *mpc_obsnorm_last_error(void) { return g_err.c_str(); }

int mpc_obsnorm_create(mpc_obsnorm **out, int num_obs, float eps, long long until) {
  if (!out) return fail(MPC_E_ARG, "mpc_obsnorm_create: bad argument");
  if (num_obs < 1 || num_obs > MPC_OBSNORM_MAX_OBS) return fail(MPC_E_ARG, "mpc_obsnorm_create: num_obs must lie in [1, 256]");
  if (!std::isfinite(eps) || eps < 0.0f) return fail(MPC_E_ARG, "mpc_obsnorm_create: eps must be finite and not negative");
  mpc_obsnorm *h = new mpc_obsnorm();
  h->D = num_obs; h->eps = eps; h->until = until < 0 ? -1 : until;
  *out = h;
  return MPC_OK;
}

void mpc_obsnorm_destroy(mpc_obsnorm *h) { mpchost::destroy_handle(h); }

int mpc_obsnorm_bind(mpc_obsnorm *h, const mpc_obsnorm_buffers_t *b) {
  if (!h || !b) return fail(MPC_E_ARG, "mpc_obsnorm_bind: bad argument");
  if (!b->d_state || !b->d_count || !b->d_mean || !b->d_var || !b->d_std) return fail(MPC_E_ARG, "mpc_obsnorm_bind: every buffer must be non-null");
  const int dev = mpchost::current_device();
  if (dev < 0) return fail(MPC_E_NODEVICE, "mpc_obsnorm_bind: no HIP device");
  if (h->workspace && h->device != dev) {
    DeviceGuard guard_(h->device);
    h->workspace.reset();
    h->capacity = 0;
  }
  h->buf = *b;
  h->device = dev;
  h->bound = true;
  return MPC_OK;
}

int mpc_obsnorm_apply(mpc_obsnorm *h, const float *d_x, float *d_y, long long n, int update, void *stream) {
  if (!h || !d_x || !d_y) return fail(MPC_E_ARG, "mpc_obsnorm_apply: bad argument");
  if (n < 1 || n > (long long)INT_MAX) return fail(MPC_E_ARG, "mpc_obsnorm_apply: n must lie in [1, 2^31 - 1]");
  if (!h->bound) return fail(MPC_E_ARG, "mpc_obsnorm_apply: no buffers bound (mpc_obsnorm_bind)");
  DeviceGuard guard_(h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long blocks = (n + kBlockRows - 1) / kBlockRows;
  Call a{h->D, n, d_x, d_y, h->eps, h->until, h->buf, nullptr, nullptr, nullptr};
  if (update) {
    if (blocks > h->capacity) {        // (hipFree waits for the launches that still read the old one)
      h->capacity = 0;
      const size_t counts = round16((size_t)blocks * sizeof(long long)), cols = round16((size_t)blocks * (size_t)h->D * sizeof(double));
      HIP_TRY(h->workspace.alloc(counts + 2 * cols));
      h->capacity = blocks;
    }
    char *w = h->workspace;
    const size_t counts = round16((size_t)h->capacity * sizeof(long long)), cols = round16((size_t)h->capacity * (size_t)h->D * sizeof(double));
    a.part_n = reinterpret_cast<long long *>(w);
    a.part_mean = reinterpret_cast<double *>(w + counts);
    a.part_m2 = reinterpret_cast<double *>(w + counts + cols);
    hipLaunchKernelGGL(partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kThreads), 0, s, a, blocks);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_obsnorm_clear(mpc_obsnorm *h, void *stream) {
  if (!h) return fail(MPC_E_ARG, "mpc_obsnorm_clear: bad argument");
  if (!h->bound) return fail(MPC_E_ARG, "mpc_obsnorm_clear: no buffers bound (mpc_obsnorm_bind)");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), h->D, h->buf);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
