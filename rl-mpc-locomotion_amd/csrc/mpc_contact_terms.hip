// mpc_contact_terms.hip -- the C ABI of mpc_contact_terms.h: the opt-in contact reward terms, the reward they rewrite, their per-term episode sums
// and the critic's friction columns (contact_terms.h) on the device, in four kernels and at most four launches per tick.
//   contact_close_kernel   one lane per environment, one wave per workgroup like shaping_close_kernel.  A marked lane (id >= 0) puts its float32 sums
//                          and its closed flag into LDS and zeroes its sums and ticks; lanes 0 .. 3 then each add one word of the block's partial
//                          over the wave's 64 environments in environment order, in float64, and lanes 0 .. 7 write the row.
//   contact_join_kernel    ONE workgroup of 256: the block partials are staged 256 rows at a time into LDS, lanes 0 .. 3 each add one word over
//                          the staged rows in block order and then add it to the window.
//   contact_run_kernel     one lane per environment, one wave per workgroup (4096 environments are 64 waves on 64 CUs): the task's six terms from
//                          what `finish` read, the shaping unit's eight from the tensor it has just written, the three contact terms from the
//                          plant's force and slip rows, the reward, sums += terms, ticks += 1.
//   contact_extend_kernel  one wavefront per environment, four to a workgroup, like height_scan_kernel's row copy but in 16-byte words: lane l
//                          handles words l, l + 64, ... of the wide row; a word below Wp / 4 is copied from the assembled row, the four behind it
//                          hold the sixteen columns.  The coefficient and the force row are addressed by a wave-uniform index.
// No atomics, static LDS only; the order of every sum is fixed, so a rerun from the same state is bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "contact_terms.h"
#include "mpc_contact_terms.h"
#include "mpc_host.h"
#include "mpc_sim_internal.h"
#include "mpc_task_config.h"

using cterms::kBlock;
using cterms::kColumns;
using cterms::kLegs;
using cterms::kPartial;
using cterms::kShapingTerms;
using cterms::kTerms;
using cterms::kWords;
using mpchost::DeviceArray;
using mpchost::DeviceGuard;

static_assert(MPC_CONTACT_TERMS == kTerms && MPC_CONTACT_SUMMARY == cterms::kSummaryLen && MPC_CONTACT_COLUMNS == kColumns &&
                  MPC_CONTACT_SHAPING_TERMS == kShapingTerms,
              "mpc_contact_terms.h and contact_terms.h disagree");
static_assert(kColumns % 4 == 0 && kPartial >= kWords, "the columns are whole 16-byte words, a partial row holds every live word");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kEnvThreads = kBlock;    // one wave per workgroup of the close and the run, and one workgroup per block of the reduction
constexpr int kJoinThreads = 256;      // block partials staged per pass of the join
constexpr int kRow = kTerms;           // LDS row stride of the close kernel: 3 words, odd, so the 64 lanes' stores spread over the banks
constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;      // of the row widening: 4096 environments are 1024 workgroups of four waves
constexpr int kExtendThreads = kWave * kWavesPerBlock;
constexpr int kMaxWidth = 65536;

__global__ __launch_bounds__(kEnvThreads) void contact_close_kernel(int n, const int *__restrict__ ids, float *sums, int *ticks,
                                                                    double *__restrict__ partials) {
  __shared__ float rows[kEnvThreads * kRow];
  __shared__ int closed[kEnvThreads];
  const int lane = threadIdx.x;
  const int first = blockIdx.x * kEnvThreads;
  const int r = first + lane;
  int cl = 0;
  if (r < n && ids[r] >= 0) {
    float s[kTerms];
#pragma unroll
    for (int i = 0; i < kTerms; ++i) {
      s[i] = sums[(size_t)r * kTerms + i];
      rows[lane * kRow + i] = s[i];
      sums[(size_t)r * kTerms + i] = 0.0f;
    }
    cl = cterms::closes(ids[r], ticks[r], s) ? 1 : 0;
    ticks[r] = 0;
  }
  closed[lane] = cl;
  __syncthreads();
  if (lane < kPartial)
    partials[(size_t)blockIdx.x * kPartial + lane] = cterms::block_partial_word(min(kEnvThreads, n - first), closed, rows, kRow, lane);
}

__global__ __launch_bounds__(kJoinThreads) void contact_join_kernel(int blocks, const double *__restrict__ partials, double *window) {
  __shared__ double stage[kJoinThreads * kPartial];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int base = 0; base < blocks; base += kJoinThreads) {
    const int here = min(kJoinThreads, blocks - base);
    for (int i = tid; i < here * kPartial; i += kJoinThreads) stage[i] = partials[(size_t)base * kPartial + i];
    __syncthreads();
    if (tid < kWords) acc = cterms::join_word(acc, here, stage, tid);
    __syncthreads();                   // the words are read before the next pass overwrites them
  }
  if (tid < kWords) window[tid] = window[tid] + acc;
}

__global__ __launch_bounds__(kEnvThreads) void contact_run_kernel(rltask::Config c, cterms::Spec k, cterms::Shaping g, int n, const float *__restrict__ root,
                                                                  const float *__restrict__ commands, const float *__restrict__ torques,
                                                                  const unsigned char *__restrict__ fell, const int *__restrict__ ids,
                                                                  const float *__restrict__ shaping_terms, const float *__restrict__ force,
                                                                  const float *__restrict__ slip, float *sums, int *ticks, float *rew,
                                                                  float *terms_out) {
  const int r = blockIdx.x * kEnvThreads + threadIdx.x;
  if (r >= n) return;
  float rt[13], cmd[3], tq[12], t[cterms::kTaskTerms], se[kShapingTerms], F[3 * kLegs], S[kLegs], e[kTerms], sm[kTerms];
#pragma unroll
  for (int i = 0; i < 13; ++i) rt[i] = root[(size_t)r * 13 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) cmd[i] = commands[(size_t)r * 3 + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) tq[i] = torques[(size_t)r * 12 + i];
#pragma unroll
  for (int i = 0; i < 3 * kLegs; ++i) F[i] = force[(size_t)r * 3 * kLegs + i];
#pragma unroll
  for (int l = 0; l < kLegs; ++l) S[l] = slip[(size_t)r * kLegs + l];
#pragma unroll
  for (int i = 0; i < kShapingTerms; ++i) se[i] = g.live ? shaping_terms[(size_t)r * kShapingTerms + i] : 0.0f;
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sm[i] = sums[(size_t)r * kTerms + i];
  int tk = ticks[r];
  rltask::reward_terms(c, rt, cmd, tq, rltask::contacts_from_fell(fell != nullptr && fell[r] != 0), t);
  cterms::tick_terms(k, F, S, ids[r], e);
  rew[r] = cterms::reward_from(k, g, cterms::chain_from(g, t, se), e, se);
  cterms::accumulate_env(e, sm, tk);
#pragma unroll
  for (int i = 0; i < kTerms; ++i) sums[(size_t)r * kTerms + i] = sm[i];
  ticks[r] = tk;
  if (terms_out) {
#pragma unroll
    for (int i = 0; i < kTerms; ++i) terms_out[(size_t)r * kTerms + i] = e[i];
  }
}

__global__ __launch_bounds__(kExtendThreads) void contact_extend_kernel(cterms::Spec k, int n, int words_in, const double *__restrict__ mu,
                                                                        const float *__restrict__ force, const float4 *__restrict__ priv,
                                                                        float4 *__restrict__ out) {
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));      // wave-uniform
  if (r >= n) return;
  const int words_out = words_in + kColumns / 4;
  const float4 *in = priv + (size_t)r * (size_t)words_in;
  float4 *row = out + (size_t)r * (size_t)words_out;
  const float *F = force + (size_t)r * 3 * kLegs;
  const double m = mu[r];
  for (int w = lane; w < words_out; w += kWave) {
    float4 v;
    if (w < words_in) {
      v = in[w];
    } else {
      const int j = 4 * (w - words_in);
      v = make_float4(cterms::column(k, m, F, j), cterms::column(k, m, F, j + 1), cterms::column(k, m, F, j + 2), cterms::column(k, m, F, j + 3));
    }
    row[w] = v;
  }
}

__global__ __launch_bounds__(64) void contact_summary_kernel(const double *__restrict__ window, double episode_length_s, double *out) {
  const int j = threadIdx.x;
  if (j < kWords) out[cterms::kSumClosed + j] = window[j];
  if (j == 0) out[cterms::kSumEpisodeS] = episode_length_s;
}
}  // namespace

struct mpc_contact {
  int n = 0, blocks = 0, device = -1;  // (the device is the bound sim's)
  rltask::Config c{};
  cterms::Spec k{};
  double episode_length_s = 0.0;
  // the bound sim's (null until mpc_contact_bind): its friction coefficients, and its caller's force and slip rows
  const double *d_mu = nullptr;        // [n]
  const float *d_force = nullptr;      // [n][4][3]
  const float *d_slip = nullptr;       // [n][4]
  DeviceArray<float> d_sums;           // [n][3]
  DeviceArray<int> d_ticks;            // [n]
  DeviceArray<double> d_partials;      // [blocks][kPartial]
  DeviceArray<double> d_window;        // [kWords]
};

extern "C" {

const char *mpc_contact_last_error(void) { return g_err.c_str(); }

void mpc_contact_destroy(mpc_contact *h) { mpchost::destroy_handle(h); }

int mpc_contact_create(mpc_contact **out, int n, const mpc_task_config *cfg, const double *scales, double max_contact_force, double force_scale,
                       double mu_clip, double dt, double episode_length_s) {
  if (!out || !cfg || !scales) return fail(MPC_E_ARG, "mpc_contact_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_contact_create: n must be at least 1");
  const taskcfg::Fault bad = taskcfg::check(*cfg);
  if (bad == taskcfg::kNotFinite) return fail(MPC_E_ARG, "mpc_contact_create: a scale or a command range is not finite");
  if (bad == taskcfg::kRangeOrder) return fail(MPC_E_ARG, "mpc_contact_create: command range with min > max");
  if (bad == taskcfg::kEpisodeLength) return fail(MPC_E_ARG, "mpc_contact_create: max_episode_length must be at least 1");
  if (!std::isfinite(cfg->clip_observations) || !(cfg->clip_observations >= 0.0))
    return fail(MPC_E_ARG, "mpc_contact_create: clip_observations must be finite and >= 0");
  if (!taskcfg::finite_all(scales, kTerms)) return fail(MPC_E_ARG, "mpc_contact_create: a contact scale is not finite");
  if (!std::isfinite(max_contact_force) || !(max_contact_force >= 0.0))
    return fail(MPC_E_ARG, "mpc_contact_create: max_contact_force must be finite and >= 0");
  if (!std::isfinite(force_scale) || !(force_scale > 0.0)) return fail(MPC_E_ARG, "mpc_contact_create: force_scale must be finite and > 0");
  if (!std::isfinite(mu_clip) || !(mu_clip > 0.0)) return fail(MPC_E_ARG, "mpc_contact_create: mu_clip must be finite and > 0");
  if (!std::isfinite(dt) || !(dt > 0.0)) return fail(MPC_E_ARG, "mpc_contact_create: dt must be finite and > 0");
  if (!std::isfinite(episode_length_s) || !(episode_length_s > 0.0))
    return fail(MPC_E_ARG, "mpc_contact_create: episode_length_s must be finite and > 0");
  mpc_contact *h = new mpc_contact();
  h->n = n;
  h->blocks = (n + kBlock - 1) / kBlock;
  h->c = taskcfg::to_device_config(*cfg);
  for (int i = 0; i < kTerms; ++i) h->k.scale[i] = (float)scales[i];
  h->k.max_contact_force = (float)max_contact_force;
  h->k.dt = (float)dt;
  h->k.force_scale = (float)force_scale;
  h->k.mu_clip = (float)mu_clip;
  h->k.clip_obs = h->c.clip_obs;
  h->episode_length_s = episode_length_s;
  *out = h;
  return MPC_OK;
}

int mpc_contact_bind(mpc_contact *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_contact_bind: null handle");
  if (!s) return fail(MPC_E_ARG, "mpc_contact_bind: null sim handle");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_contact_bind: the sim has " + std::to_string(s->n) + " robots, the contact terms " + std::to_string(h->n) + " environments");
  if (h->d_mu) return fail(MPC_E_ARG, "mpc_contact_bind: the contact terms are bound to a sim already");
  if (!s->friction || !s->d_mu) return fail(MPC_E_ARG, "mpc_contact_bind: the sim has no friction record (mpc_friction_attach)");
  if (!s->d_force || !s->d_slip) return fail(MPC_E_ARG, "mpc_contact_bind: the sim's friction record has no force or no slip rows");
  DeviceGuard guard_(s->device);
  DeviceArray<float> d_sums;
  DeviceArray<int> d_ticks;
  DeviceArray<double> d_partials, d_window;
  hipError_t e;
  if ((e = d_sums.alloc_zero((size_t)h->n * kTerms)) != hipSuccess || (e = d_ticks.alloc_zero((size_t)h->n)) != hipSuccess ||
      (e = d_partials.alloc_zero((size_t)h->blocks * kPartial)) != hipSuccess || (e = d_window.alloc_zero(kWords)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess)
    return fail(MPC_E_HIP, std::string("mpc_contact_bind: ") + hipGetErrorString(e));
  h->d_sums = std::move(d_sums);
  h->d_ticks = std::move(d_ticks);
  h->d_partials = std::move(d_partials);
  h->d_window = std::move(d_window);
  h->device = s->device;
  h->d_mu = s->d_mu;
  h->d_force = s->d_force;
  h->d_slip = s->d_slip;
  return MPC_OK;
}

int mpc_contact_close(mpc_contact *h, const int *d_reset_ids, void *stream) {
  if (!h || !d_reset_ids) return fail(MPC_E_ARG, "mpc_contact_close: null argument");
  if (!h->d_mu) return fail(MPC_E_ARG, "mpc_contact_close: no sim bound (mpc_contact_bind)");
  DeviceGuard guard_(h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(contact_close_kernel, dim3((unsigned)h->blocks), dim3(kEnvThreads), 0, s, h->n, d_reset_ids, h->d_sums, h->d_ticks, h->d_partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(contact_join_kernel, dim3(1), dim3(kJoinThreads), 0, s, h->blocks, (const double *)h->d_partials, h->d_window);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_contact_run(mpc_contact *h, const float *d_root, const float *d_commands, const float *d_torques, const unsigned char *d_fell,
                    const int *d_reset_ids, const float *d_shaping_terms, const double *shaping_scales, float *d_rew, float *d_terms, void *stream) {
  if (!h || !d_root || !d_commands || !d_torques || !d_reset_ids || !d_rew) return fail(MPC_E_ARG, "mpc_contact_run: null argument");
  if ((d_shaping_terms != nullptr) != (shaping_scales != nullptr))
    return fail(MPC_E_ARG, "mpc_contact_run: d_shaping_terms goes with shaping_scales, NULL with NULL");
  if (shaping_scales && !taskcfg::finite_all(shaping_scales, kShapingTerms)) return fail(MPC_E_ARG, "mpc_contact_run: a shaping scale is not finite");
  if (d_terms && (const void *)d_terms == (const void *)d_shaping_terms)
    return fail(MPC_E_ARG, "mpc_contact_run: d_terms must not be d_shaping_terms (the rows have different widths)");
  if (!h->d_mu) return fail(MPC_E_ARG, "mpc_contact_run: no sim bound (mpc_contact_bind)");
  cterms::Shaping g{};
  if (shaping_scales) {
    g.live = 1;
    for (int i = 0; i < kShapingTerms; ++i) g.scale[i] = (float)shaping_scales[i];
  }
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(contact_run_kernel, dim3((unsigned)h->blocks), dim3(kEnvThreads), 0, reinterpret_cast<hipStream_t>(stream), h->c, h->k, g, h->n, d_root,
                     d_commands, d_torques, d_fell, d_reset_ids, d_shaping_terms, h->d_force, h->d_slip, h->d_sums, h->d_ticks, d_rew, d_terms);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_contact_extend(mpc_contact *h, const float *d_priv, int Wp, float *d_out, void *stream) {
  if (!h || !d_priv || !d_out) return fail(MPC_E_ARG, "mpc_contact_extend: null argument");
  if (Wp < 16 || Wp > kMaxWidth || Wp % 16 != 0) return fail(MPC_E_ARG, "mpc_contact_extend: Wp must be a multiple of 16 in [16, 65536]");
  if (!mpchost::aligned16(d_priv) || !mpchost::aligned16(d_out)) return fail(MPC_E_ARG, "mpc_contact_extend: d_priv and d_out must be 16-byte aligned");
  const mpchost::Range ranges[2] = {{d_priv, sizeof(float) * (size_t)h->n * (size_t)Wp}, {d_out, sizeof(float) * (size_t)h->n * (size_t)(Wp + kColumns)}};
  if (mpchost::any_overlap(ranges, 2)) return fail(MPC_E_ARG, "mpc_contact_extend: d_out must be distinct from d_priv (the rows have different widths)");
  if (!h->d_mu) return fail(MPC_E_ARG, "mpc_contact_extend: no sim bound (mpc_contact_bind)");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(contact_extend_kernel, dim3((unsigned)((h->n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kExtendThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), h->k, h->n, Wp / 4, h->d_mu, h->d_force, reinterpret_cast<const float4 *>(d_priv),
                     reinterpret_cast<float4 *>(d_out));
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_contact_summary(mpc_contact *h, double *d_out, void *stream) {
  if (!h || !d_out) return fail(MPC_E_ARG, "mpc_contact_summary: null argument");
  if (!h->d_mu) return fail(MPC_E_ARG, "mpc_contact_summary: no sim bound (mpc_contact_bind)");
  DeviceGuard guard_(h->device);
  hipLaunchKernelGGL(contact_summary_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (const double *)h->d_window, h->episode_length_s,
                     d_out);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_contact_new_window(mpc_contact *h, void *stream) {
  if (!h) return fail(MPC_E_ARG, "mpc_contact_new_window: null handle");
  if (!h->d_mu) return fail(MPC_E_ARG, "mpc_contact_new_window: no sim bound (mpc_contact_bind)");
  DeviceGuard guard_(h->device);
  HIP_TRY(hipMemsetAsync(h->d_window, 0, sizeof(double) * kWords, reinterpret_cast<hipStream_t>(stream)));
  return MPC_OK;
}

int mpc_contact_arrays(mpc_contact *h, float **d_sums, int **d_ticks, double **d_window) {
  if (!h || !d_sums || !d_ticks || !d_window) return fail(MPC_E_ARG, "mpc_contact_arrays: null argument");
  if (!h->d_mu) return fail(MPC_E_ARG, "mpc_contact_arrays: no sim bound (mpc_contact_bind)");
  *d_sums = h->d_sums;
  *d_ticks = h->d_ticks;
  *d_window = h->d_window;
  return MPC_OK;
}

}  // extern "C"
