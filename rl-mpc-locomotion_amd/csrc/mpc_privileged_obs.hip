// mpc_privileged_obs.hip -- the C ABI of mpc_privileged_obs.h: the critic's privileged observation row (privileged_obs.h) on the device, in one kernel.
//   privileged_obs_kernel   one lane per float4 of the output matrix [n][Wp]: consecutive lanes sit on consecutive 16-byte words of a row (Wp is a
//                           multiple of 16, so every row starts on a 64-byte boundary and a wave's store covers 1024 consecutive bytes).  A quad that
//                           lies inside the 48 + P live columns is one 16-byte load of the wide observation row; the quad that straddles their end and
//                           the ones behind it are put together element by element: the rest of the live columns, the four contact flags from the
//                           sim's int32 record, the phase, the zero pad.  No LDS, no atomics, no scratch.
//   privileged_obs_plant_kernel   the same lanes on the wider row of mpc_privobs_run_plant: the three plant columns from the sim's float64 plant record
//                           follow the phase.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mpc_host.h"
#include "mpc_privileged_obs.h"
#include "mpc_sim_internal.h"
#include "privileged_obs.h"

using mpchost::DeviceGuard;

static_assert(MPC_PRIVOBS_TASK_OBS == privobs::kTaskObs && MPC_PRIVOBS_CONTACTS == privobs::kContacts && MPC_PRIVOBS_MAX_SCAN == privobs::kMaxScan,
              "mpc_privileged_obs.h and privileged_obs.h disagree");
static_assert(toysim::kI32 >= privobs::kContacts, "the sim's int32 record starts with the four contact flags");
static_assert(toysim::kPlant == privobs::kPlantCols && toysim::kGravZ == privobs::kGravZ, "toy_sim.h and privileged_obs.h disagree");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kThreads = 256;
constexpr int kMaxObsWidth = 65536;

// total = n * quads_per_row; live = 48 + P <= obs_width; quads_per_row = Wp / 4.  kPlant: the row of mpc_privobs_run_plant (plant non-null)
template <bool kPlant>
__device__ __forceinline__ void assemble_quad(int n, unsigned total, unsigned quads_per_row, int live, int obs_width, float inv_len,
                                              const float *__restrict__ obs, const int *__restrict__ i32, const double *__restrict__ plant,
                                              const long long *__restrict__ progress, float *__restrict__ out) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const unsigned r = i / quads_per_row, q = i - r * quads_per_row;
  const int col0 = 4 * (int)q;
  const float *in = obs + (size_t)r * (size_t)obs_width;
  float4 v;
  if (col0 + 4 <= live) {
    v = *reinterpret_cast<const float4 *>(in + col0);
  } else {
    const long long prog = progress[r];
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + j;
      if constexpr (kPlant) e[j] = col < live ? in[col] : privobs::tail_column_plant(col, live, i32, plant, n, (int)r, prog, inv_len);
      else e[j] = col < live ? in[col] : privobs::tail_column(col, live, i32, n, (int)r, prog, inv_len);
    }
    v = make_float4(e[0], e[1], e[2], e[3]);
  }
  reinterpret_cast<float4 *>(out)[i] = v;
}

__global__ __launch_bounds__(kThreads) void privileged_obs_kernel(int n, unsigned total, unsigned quads_per_row, int live, int obs_width, float inv_len,
                                                                  const float *__restrict__ obs, const int *__restrict__ i32,
                                                                  const long long *__restrict__ progress, float *__restrict__ out) {
  assemble_quad<false>(n, total, quads_per_row, live, obs_width, inv_len, obs, i32, nullptr, progress, out);
}

__global__ __launch_bounds__(kThreads) void privileged_obs_plant_kernel(int n, unsigned total, unsigned quads_per_row, int live, int obs_width, float inv_len,
                                                                        const float *__restrict__ obs, const int *__restrict__ i32,
                                                                        const double *__restrict__ plant, const long long *__restrict__ progress,
                                                                        float *__restrict__ out) {
  assemble_quad<true>(n, total, quads_per_row, live, obs_width, inv_len, obs, i32, plant, progress, out);
}
}  // namespace

struct mpc_privobs {
  int n = 0, device = -1;
  const int *d_i32 = nullptr;          // the bound sim's int32 state record (null until mpc_privobs_bind)
  const double *d_plant = nullptr;     // the bound sim's plant record (null until mpc_privobs_bind_plant)
};

extern "C" {

const char *mpc_privobs_last_error(void) { return g_err.c_str(); }

int mpc_privobs_width(int P) {
  if (P < 0 || P > MPC_PRIVOBS_MAX_SCAN) return fail(MPC_E_ARG, "mpc_privobs_width: P must lie in [0, 208]");
  return privobs::width(P);
}

void mpc_privobs_destroy(mpc_privobs *h) { delete h; }      // owns no device memory

int mpc_privobs_create(mpc_privobs **out, int n) {
  if (!out) return fail(MPC_E_ARG, "mpc_privobs_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_privobs_create: n must be at least 1");
  mpc_privobs *h = new mpc_privobs();
  h->n = n;
  *out = h;
  return MPC_OK;
}

int mpc_privobs_bind(mpc_privobs *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_privobs_bind: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_privobs_bind: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_privobs_bind: the sim has " + std::to_string(s->n) + " robots, the privileged row " + std::to_string(h->n) + " environments");
  if (!s->d_i32) return fail(MPC_E_ARG, "mpc_privobs_bind: the sim has no state record");
  h->d_i32 = s->d_i32;
  h->device = s->device;
  return MPC_OK;
}

// mpc_privobs_run (plant false) and mpc_privobs_run_plant: the same checks in the same order under the entry point's own name
static int run(const char *name, bool plant, mpc_privobs *h, const float *d_obs, int obs_width, int P, const long long *d_progress, double inv_len, float *d_out,
               void *stream) {
  const std::string who = std::string(name) + ": ";
  if (!h || !d_obs || !d_progress || !d_out) return fail(MPC_E_ARG, who + "null argument");
  if (P < 0 || P > MPC_PRIVOBS_MAX_SCAN) return fail(MPC_E_ARG, who + "P must lie in [0, 208]");
  const int live = privobs::kTaskObs + P;
  if (obs_width < live || obs_width > kMaxObsWidth || (obs_width & 3)) return fail(MPC_E_ARG, who + "obs_width must be a multiple of 4 in [48 + P, 65536]");
  if (((uintptr_t)d_obs | (uintptr_t)d_out) & 15u) return fail(MPC_E_ARG, who + "d_obs and d_out must be 16-byte aligned");
  if ((uintptr_t)d_progress & 7u) return fail(MPC_E_ARG, who + "d_progress must be 8-byte aligned");
  if (d_obs == d_out) return fail(MPC_E_ARG, who + "d_out must not be d_obs (the rows have different widths)");
  if (!std::isfinite((float)inv_len)) return fail(MPC_E_ARG, who + "inv_len must be finite as a float32");
  const unsigned quads = (unsigned)((plant ? privobs::width_plant(P) : privobs::width(P)) / 4);
  if ((long long)h->n * quads > 0x7FFFFFFFll) return fail(MPC_E_ARG, who + "n * width / 4 must stay below 2^31");
  if (!h->d_i32) return fail(MPC_E_ARG, who + "no sim bound (mpc_privobs_bind)");
  if (plant && !h->d_plant) return fail(MPC_E_ARG, who + "no plant record bound (mpc_privobs_bind_plant)");
  const unsigned total = (unsigned)h->n * quads;
  const dim3 grid((total + kThreads - 1) / kThreads);
  DeviceGuard guard_(h->device);
  if (plant)
    hipLaunchKernelGGL(privileged_obs_plant_kernel, grid, dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), h->n, total, quads, live, obs_width,
                       (float)inv_len, d_obs, h->d_i32, h->d_plant, d_progress, d_out);
  else
    hipLaunchKernelGGL(privileged_obs_kernel, grid, dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), h->n, total, quads, live, obs_width,
                       (float)inv_len, d_obs, h->d_i32, d_progress, d_out);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_privobs_run(mpc_privobs *h, const float *d_obs, int obs_width, int P, const long long *d_progress, double inv_len, float *d_out,
                    void *stream) {
  return run("mpc_privobs_run", false, h, d_obs, obs_width, P, d_progress, inv_len, d_out, stream);
}

int mpc_privobs_width_plant(int P) {
  if (P < 0 || P > MPC_PRIVOBS_MAX_SCAN) return fail(MPC_E_ARG, "mpc_privobs_width_plant: P must lie in [0, 208]");
  return privobs::width_plant(P);
}

int mpc_privobs_bind_plant(mpc_privobs *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_privobs_bind_plant: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_privobs_bind_plant: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_privobs_bind_plant: the sim has " + std::to_string(s->n) + " robots, the privileged row " + std::to_string(h->n) + " environments");
  if (h->d_i32 != s->d_i32) return fail(MPC_E_ARG, "mpc_privobs_bind_plant: bind the same sim with mpc_privobs_bind first");
  if (!s->d_plant) return fail(MPC_E_ARG, "mpc_privobs_bind_plant: the sim has no plant record (mpc_plant_rand_attach)");
  h->d_plant = s->d_plant;
  return MPC_OK;
}

int mpc_privobs_run_plant(mpc_privobs *h, const float *d_obs, int obs_width, int P, const long long *d_progress, double inv_len, float *d_out,
                          void *stream) {
  return run("mpc_privobs_run_plant", true, h, d_obs, obs_width, P, d_progress, inv_len, d_out, stream);
}

}  // extern "C"
