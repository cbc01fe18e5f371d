// mpc_ppo_update.hip -- the C ABI of include/mpc_ppo_update.h: the update half of a PPO iteration on the device.
//   pgemm::launch        forward, backward-data and backward-weight GEMMs of both nets (mpc_ppo_gemm.hip), actor and critic in one launch per layer
//   head_kernel          one lane per row: ppo::head_row on the forward pass's mean and value and the indexed storage rows; writes d loss / d mu and
//                        d loss / d V where the backward pass reads them, and one float64 partial per workgroup and quantity (fixed-order LDS sums)
//   head_reduce_kernel   ONE workgroup joins the partials in index order: the four terms, d loss / d std, the learning-rate decision
//   pgemm::reduce        the weight-gradient chunks, and the bias gradients, summed in index order into the .grad tensors
//   norm_partial_kernel  the sum of squares of every gradient element in float64, one partial per 4096 elements of a tensor (fixed-order LDS tree), and
//   norm_kernel          ONE workgroup joins the partials in a fixed order, as normalise_kernel of mpc_ppo.hip does
//   adam_kernel          every parameter tensor in one launch (blockIdx.y picks the tensor): ppo::adam_element
// No atomics anywhere, so a rerun is bit-identical; nothing synchronises.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mpc_ppo_update.h"
#include "mpc_ac_internal.h"
#include "mpc_host.h"
#include "ppo_gemm_plan.h"
#include "ppo_update.h"

using mpchost::DeviceGuard;
using mpchost::present16;

namespace {
int fail(int code, const std::string &msg) { return mpc_ppo_set_error(code, msg.c_str()); }      // (mpc_ppo.hip's slot: one mpc_ppo_last_error for both halves)

constexpr int kActor = 0, kCritic = 1;
constexpr int kHeadThreads = 256;
constexpr int kHeadQ = 3 + ppo::kActions;      // surrogate, value loss, kl, d std[12]
constexpr int kHeadStride = 16;                // doubles per workgroup partial
constexpr int kOutLd = 16;                     // leading dimension of the last layer's output (12 or 1 columns) in the workspace
constexpr int kNormThreads = 1024;
constexpr int kMaxTensors = 4 * MPC_AC_MAX_LAYERS + 1;

struct Storage {
  const float *obs, *actions, *values, *adv, *returns, *log_prob, *mu, *sigma;
  long long total_rows;
};

__global__ __launch_bounds__(kHeadThreads) void head_kernel(int rows, const long long *__restrict__ idx, Storage st, ppo::HeadCfg cfg,
                                                            const float *__restrict__ mu, const float *__restrict__ V, const float *__restrict__ std,
                                                            float *__restrict__ dmu, float *__restrict__ dV, double *__restrict__ partials) {
  __shared__ float vals[kHeadQ][kHeadThreads];
  __shared__ double mid[kHeadQ][16];
  const int t = threadIdx.x, row = blockIdx.x * kHeadThreads + t;
  ppo::HeadRow o;
  o.surrogate = o.value_loss = o.kl = 0.f;
#pragma unroll
  for (int k = 0; k < ppo::kActions; ++k) o.dstd[k] = 0.f;
  if (row < rows) {
    long long r = idx[row];
    r = r < 0 ? 0 : (r >= st.total_rows ? st.total_rows - 1 : r);
    float s[ppo::kActions], m[ppo::kActions], a[ppo::kActions], om[ppo::kActions], os[ppo::kActions];
#pragma unroll
    for (int k = 0; k < ppo::kActions; k += 4) {
      *reinterpret_cast<float4 *>(s + k) = *reinterpret_cast<const float4 *>(std + k);
      *reinterpret_cast<float4 *>(m + k) = *reinterpret_cast<const float4 *>(mu + (size_t)row * kOutLd + k);
      *reinterpret_cast<float4 *>(a + k) = *reinterpret_cast<const float4 *>(st.actions + (size_t)r * ppo::kActions + k);
      *reinterpret_cast<float4 *>(om + k) = *reinterpret_cast<const float4 *>(st.mu + (size_t)r * ppo::kActions + k);
      *reinterpret_cast<float4 *>(os + k) = *reinterpret_cast<const float4 *>(st.sigma + (size_t)r * ppo::kActions + k);
    }
    ppo::head_row(cfg, m, V[(size_t)row * kOutLd], s, a, st.values[r], st.adv[r], st.returns[r], st.log_prob[r], om, os, o);
#pragma unroll
    for (int k = 0; k < ppo::kActions; k += 4)
      *reinterpret_cast<float4 *>(dmu + (size_t)row * kOutLd + k) = *reinterpret_cast<const float4 *>(o.dmu + k);
    dV[(size_t)row * kOutLd] = o.dv;
  }
  vals[0][t] = o.surrogate; vals[1][t] = o.value_loss; vals[2][t] = o.kl;
#pragma unroll
  for (int k = 0; k < ppo::kActions; ++k) vals[3 + k][t] = o.dstd[k];
  __syncthreads();
  if (t < kHeadQ * 16) {                 // 16 consecutive rows each, in row order
    const int q = t >> 4, j = t & 15;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += (double)vals[q][16 * j + i];
    mid[q][j] = sum;
  }
  __syncthreads();
  if (t < kHeadQ) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) sum += mid[t][j];
    partials[(size_t)blockIdx.x * kHeadStride + t] = sum;
  }
}

__global__ __launch_bounds__(kHeadThreads) void head_reduce_kernel(int blocks, int rows, const double *__restrict__ partials, const float *__restrict__ std,
                                                                   float entropy_coef, int adaptive, double desired_kl, double *__restrict__ lr,
                                                                   float *__restrict__ terms, float *__restrict__ gstd) {
  __shared__ double mid[kHeadQ][16];
  const int t = threadIdx.x;
  if (t < kHeadQ * 16) {                 // sixteen runs of consecutive workgroups per quantity, each in index order ...
    const int q = t >> 4, j = t & 15, per = (blocks + 15) / 16;
    const int b1 = (j + 1) * per < blocks ? (j + 1) * per : blocks;
    double sum = 0.0;
    for (int b = j * per; b < b1; ++b) sum += partials[(size_t)b * kHeadStride + q];
    mid[q][j] = sum;
  }
  __syncthreads();
  if (t >= kHeadQ) return;
  const int q = t;
  double s = 0.0;                        // ... and the runs in index order
#pragma unroll
  for (int j = 0; j < 16; ++j) s += mid[q][j];
  if (q < 3) {
    const float mean = (float)(s / (double)rows);
    terms[q == 2 ? 3 : q] = mean;
    if (q == 2) {
      terms[2] = ppo::entropy_row(std);
      if (adaptive) *lr = ppo::adapt_lr(*lr, (double)mean, desired_kl);
    }
  } else {
    gstd[q - 3] = (float)s + ppo::entropy_dstd(entropy_coef, std[q - 3]);
  }
}

struct NormTable {
  const float *g[kMaxTensors];
  int numel[kMaxTensors];
};
constexpr int kNormPerBlock = 4096;            // elements per workgroup of the first stage

// grid (ceil(max numel / 4096), tensors): partial[tensor * gridDim.x + block] = that slice's sum of squares in float64 (lane i takes elements i, i + 256,
// ..., then a fixed-order LDS tree); a workgroup past its tensor's end writes zero
__global__ __launch_bounds__(256) void norm_partial_kernel(NormTable t, double *__restrict__ partial) {
  __shared__ double tree[256];
  const int k = blockIdx.y, m = t.numel[k];
  const float *__restrict__ g = t.g[k];
  const int i0 = blockIdx.x * kNormPerBlock;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kNormPerBlock / 256; ++j) {
    const int i = i0 + j * 256 + (int)threadIdx.x;
    const double x = i < m ? (double)g[i] : 0.0;
    s += x * x;
  }
  tree[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)k * gridDim.x + blockIdx.x] = tree[0];
}

// ONE workgroup: the partials in a fixed order (lane i takes i, i + 1024, ..., then the tree)
__global__ __launch_bounds__(kNormThreads) void norm_kernel(int n, const double *__restrict__ partial, float *__restrict__ norm) {
  __shared__ double tree[kNormThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kNormThreads) s += partial[i];
  tree[threadIdx.x] = s;
  __syncthreads();
  for (int w = kNormThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *norm = (float)sqrt(tree[0]);
}

struct AdamTable {
  float *p[kMaxTensors], *g[kMaxTensors], *m[kMaxTensors], *v[kMaxTensors];
  int numel[kMaxTensors];
};

// grid (ceil(max numel / 256), tensors)
__global__ __launch_bounds__(256) void adam_kernel(AdamTable t, ppo::AdamCfg cfg, float max_norm, const float *__restrict__ norm,
                                                   const double *__restrict__ lr) {
  const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= t.numel[k]) return;
  const float coef = ppo::clip_coef(*norm, max_norm);
  float p = t.p[k][i], g = t.g[k][i], m = t.m[k][i], v = t.v[k][i];
  ppo::adam_element(cfg, *lr, coef, p, g, m, v);
  t.p[k][i] = p; t.g[k][i] = g; t.m[k][i] = m; t.v[k][i] = v;
}

int round16(int x) { return (x + 15) / 16 * 16; }

// one GEMM launch of both nets through mpc_ppo_gemm.hip, which fills the plan's tiles and chunks into L
int launch_gemm(pgemm::Kind kind, pgemm::Launch &L, hipStream_t s) {
  pgemm::launch(kind, L, s);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}
}  // namespace

struct mpc_ppo_update {
  mpc_ac *ac = nullptr;
  int device = -1, max_rows = 0, max_chunks = 0, head_blocks_max = 0;
  int nl[2] = {0, 0};
  int dims[2][MPC_AC_MAX_LAYERS + 1] = {};
  int n_tensors = 0;
  mpchost::DeviceArray<float> ws;               // one allocation; the pointers below, down to `norm`, point into it
  float *Y[2][MPC_AC_MAX_LAYERS] = {};          // [rows][ld(k, l)] activations after layer l
  float *dY[2][MPC_AC_MAX_LAYERS] = {};         // their gradients
  float *dWp[2][MPC_AC_MAX_LAYERS] = {};        // [chunks][out][in]
  float *dbp[2][MPC_AC_MAX_LAYERS] = {};        // [chunks][out]
  double *partials = nullptr;                   // [head blocks][16]
  double *norm_partials = nullptr;              // [tensors][norm blocks]
  int norm_blocks = 0;
  float *norm = nullptr;
  float *grad[kMaxTensors] = {}, *exp_avg[kMaxTensors] = {}, *exp_avg_sq[kMaxTensors] = {};
  bool grads_bound = false, moments_bound = false, storage_set = false;
  Storage st{};
  const float *critic_obs = nullptr;            // [total_rows][dims[kCritic][0]] (mpc_ppo_update_set_critic_storage), or null: the critic reads st.obs

  // the rows layer 0 of net k reads through the index
  const float *rows0(int k) const { return k == kCritic && critic_obs ? critic_obs : st.obs; }
  int ld(int k, int l) const { return l + 1 == nl[k] ? kOutLd : dims[k][l + 1]; }
  // mpc_ac_bind's order: actor weights, actor biases, critic weights, critic biases, std
  int w_index(int k, int l) const { return (k == kActor ? 0 : 2 * nl[0]) + l; }
  int b_index(int k, int l) const { return (k == kActor ? nl[0] : 2 * nl[0] + nl[1]) + l; }
  int numel(int t) const {
    if (t == n_tensors - 1) return ppo::kActions;
    for (int k = 0; k < 2; ++k)
      for (int l = 0; l < nl[k]; ++l) {
        if (t == w_index(k, l)) return dims[k][l + 1] * dims[k][l];
        if (t == b_index(k, l)) return dims[k][l + 1];
      }
    return 0;
  }
};

extern "C" {

void mpc_ppo_update_destroy(mpc_ppo_update *u) { mpchost::destroy_handle(u); }

int mpc_ppo_update_tensors(const mpc_ppo_update *u) { return u ? u->n_tensors : -1; }

int mpc_ppo_update_create(mpc_ppo_update **out, mpc_ac *ac, int max_rows) {
  mpc_ac_view v;
  if (!out || !mpc_ac_get_view(ac, &v)) return fail(MPC_E_ARG, "mpc_ppo_update_create: bad argument");
  if (max_rows <= 0) return fail(MPC_E_ARG, "mpc_ppo_update_create: max_rows must be positive");
  if (!v.bound) return fail(MPC_E_ARG, "mpc_ppo_update_create: the mpc_ac has no parameters bound (mpc_ac_bind)");
  mpc_ppo_update *u = new mpc_ppo_update();
  u->ac = ac;
  u->device = v.device;
  u->max_rows = max_rows;
  u->max_chunks = (max_rows + pgemm::kMinChunk - 1) / pgemm::kMinChunk;
  u->head_blocks_max = (max_rows + kHeadThreads - 1) / kHeadThreads;
  size_t words = 0;
  for (int k = 0; k < 2; ++k) {
    u->nl[k] = v.n_layers[k];
    for (int l = 0; l <= v.n_layers[k]; ++l) u->dims[k][l] = v.dims[k][l];
    for (int l = 0; l < u->nl[k]; ++l)
      words += 2 * (size_t)max_rows * u->ld(k, l) + (size_t)u->max_chunks * ((size_t)round16(u->dims[k][l + 1]) * u->dims[k][l] + round16(u->dims[k][l + 1]));
  }
  u->n_tensors = 2 * (u->nl[0] + u->nl[1]) + 1;
  int maxn = 0;
  for (int t = 0; t < u->n_tensors; ++t) maxn = u->numel(t) > maxn ? u->numel(t) : maxn;
  u->norm_blocks = (maxn + kNormPerBlock - 1) / kNormPerBlock;
  words += 2 * (size_t)u->head_blocks_max * kHeadStride + 2 * (size_t)round16(u->n_tensors * u->norm_blocks) + 16;
  DeviceGuard guard_(u->device);
  if (u->ws.alloc(words) != hipSuccess) {
    delete u;
    return fail(MPC_E_HIP, "mpc_ppo_update_create: the workspace could not be allocated");
  }
  float *w = u->ws;
  u->partials = reinterpret_cast<double *>(w); w += 2 * (size_t)u->head_blocks_max * kHeadStride;
  u->norm_partials = reinterpret_cast<double *>(w); w += 2 * (size_t)round16(u->n_tensors * u->norm_blocks);
  u->norm = w; w += 16;
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < u->nl[k]; ++l) {
      u->Y[k][l] = w; w += (size_t)max_rows * u->ld(k, l);
      u->dY[k][l] = w; w += (size_t)max_rows * u->ld(k, l);
      u->dWp[k][l] = w; w += (size_t)u->max_chunks * round16(u->dims[k][l + 1]) * u->dims[k][l];
      u->dbp[k][l] = w; w += (size_t)u->max_chunks * round16(u->dims[k][l + 1]);
    }
  *out = u;
  return MPC_OK;
}

int mpc_ppo_update_bind(mpc_ppo_update *u, float *const *d_grads, float *const *d_exp_avg, float *const *d_exp_avg_sq) {
  if (!u || !d_grads) return fail(MPC_E_ARG, "mpc_ppo_update_bind: bad argument");
  if ((d_exp_avg == nullptr) != (d_exp_avg_sq == nullptr)) return fail(MPC_E_ARG, "mpc_ppo_update_bind: both moments or neither");
  for (int t = 0; t < u->n_tensors; ++t)
    if (!present16(d_grads[t]) || (d_exp_avg && (!present16(d_exp_avg[t]) || !present16(d_exp_avg_sq[t]))))
      return fail(MPC_E_ARG, "mpc_ppo_update_bind: every gradient and moment pointer must be non-null and 16-byte aligned");
  for (int t = 0; t < u->n_tensors; ++t) {
    u->grad[t] = d_grads[t];
    u->exp_avg[t] = d_exp_avg ? d_exp_avg[t] : nullptr;
    u->exp_avg_sq[t] = d_exp_avg ? d_exp_avg_sq[t] : nullptr;
  }
  u->grads_bound = true;
  u->moments_bound = d_exp_avg != nullptr;
  return MPC_OK;
}

int mpc_ppo_update_set_storage(mpc_ppo_update *u, long long total_rows, const float *d_obs, const float *d_actions, const float *d_values,
                               const float *d_advantages, const float *d_returns, const float *d_log_prob, const float *d_mu, const float *d_sigma) {
  if (!u || total_rows <= 0 || !d_values || !d_advantages || !d_returns || !d_log_prob) return fail(MPC_E_ARG, "mpc_ppo_update_set_storage: bad argument");
  if (!present16(d_obs) || !present16(d_actions) || !present16(d_mu) || !present16(d_sigma))
    return fail(MPC_E_ARG, "mpc_ppo_update_set_storage: d_obs, d_actions, d_mu and d_sigma must be non-null and 16-byte aligned");
  u->st = Storage{d_obs, d_actions, d_values, d_advantages, d_returns, d_log_prob, d_mu, d_sigma, total_rows};
  u->storage_set = true;
  return MPC_OK;
}

int mpc_ppo_update_set_critic_storage(mpc_ppo_update *u, const float *d_critic_obs) {
  if (!mpchost::aligned16(d_critic_obs))
    return fail(MPC_E_ARG, "mpc_ppo_update_set_critic_storage: d_critic_obs must be 16-byte aligned");
  if (!u) return fail(MPC_E_ARG, "mpc_ppo_update_set_critic_storage: bad argument");
  u->critic_obs = d_critic_obs;                 // (null: back to the actor's rows)
  return MPC_OK;
}

int mpc_ppo_update_grads(mpc_ppo_update *u, int rows, const long long *d_idx, double clip_param, double value_loss_coef, double entropy_coef,
                         int use_clipped_value_loss, int adaptive, double desired_kl, double *d_lr, float *d_terms, void *stream) {
  if (!u || !d_idx || !d_terms) return fail(MPC_E_ARG, "mpc_ppo_update_grads: bad argument");
  if (rows <= 0 || rows > u->max_rows) return fail(MPC_E_ARG, "mpc_ppo_update_grads: rows must lie in 1 .. max_rows");
  if (!std::isfinite(clip_param) || clip_param <= 0.0 || !std::isfinite(value_loss_coef) || !std::isfinite(entropy_coef))
    return fail(MPC_E_ARG, "mpc_ppo_update_grads: clip_param must be positive and the coefficients finite");
  if (adaptive && (!d_lr || !(desired_kl > 0.0) || !std::isfinite(desired_kl)))
    return fail(MPC_E_ARG, "mpc_ppo_update_grads: the adaptive schedule needs d_lr and a positive desired_kl");
  if (!u->grads_bound) return fail(MPC_E_ARG, "mpc_ppo_update_grads: no gradients bound (mpc_ppo_update_bind)");
  if (!u->storage_set) return fail(MPC_E_ARG, "mpc_ppo_update_grads: no storage set (mpc_ppo_update_set_storage)");
  mpc_ac_view v;
  if (!mpc_ac_get_view(u->ac, &v) || !v.bound) return fail(MPC_E_ARG, "mpc_ppo_update_grads: the mpc_ac has no parameters bound");
  if (v.asymmetric && !u->critic_obs)
    return fail(MPC_E_ARG, "mpc_ppo_update_grads: an asymmetric mpc_ac needs the critic's rows (mpc_ppo_update_set_critic_storage)");
  DeviceGuard guard_(u->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int maxl = u->nl[0] > u->nl[1] ? u->nl[0] : u->nl[1];

  // forward: layer l of both nets side by side.  (tests/test_ppo_gemm_plan.py restates this sequence of launches and their (M, N, K), here and in the
  // backward loop below, to pin which kernels the tests reach: a launch added, dropped or reshaped here has to be restated there)
  for (int l = 0; l < maxl; ++l) {
    pgemm::Launch L{};
    for (int k = 0; k < 2; ++k) {
      if (l >= u->nl[k]) continue;
      pgemm::Problem &p = L.p[k];
      p.A = l == 0 ? u->rows0(k) : u->Y[k][l - 1];
      p.idx = l == 0 ? d_idx : nullptr;
      p.idx_limit = u->st.total_rows;
      p.B = v.w[k][l];
      p.C = u->Y[k][l];
      p.aux = v.b[k][l];
      p.M = rows; p.N = u->dims[k][l + 1]; p.K = u->dims[k][l];
      p.lda = l == 0 ? u->dims[k][0] : u->ld(k, l - 1); p.ldb = p.K; p.ldc = u->ld(k, l);
      p.elu = l + 1 < u->nl[k];
      p.chunks = 1;
    }
    if (int rc = launch_gemm(pgemm::kForward, L, s)) return rc;
  }

  // the loss head
  ppo::HeadCfg cfg{(float)clip_param, (float)value_loss_coef, (float)entropy_coef, use_clipped_value_loss ? 1 : 0, 1.0f / (float)rows};
  const int hb = (rows + kHeadThreads - 1) / kHeadThreads;
  const int la = u->nl[kActor] - 1, lc = u->nl[kCritic] - 1;
  hipLaunchKernelGGL(head_kernel, dim3((unsigned)hb), dim3(kHeadThreads), 0, s, rows, d_idx, u->st, cfg, u->Y[kActor][la], u->Y[kCritic][lc], v.std,
                     u->dY[kActor][la], u->dY[kCritic][lc], u->partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(head_reduce_kernel, dim3(1), dim3(kHeadThreads), 0, s, hb, rows, u->partials, v.std, (float)entropy_coef, adaptive ? 1 : 0, desired_kl, d_lr,
                     d_terms, u->grad[u->n_tensors - 1]);
  HIP_TRY(hipGetLastError());

  // backward: from the last layer of each net towards the first; dW partials, then dX into the layer below
  int dw_chunks[2][MPC_AC_MAX_LAYERS] = {};
  for (int sidx = 0; sidx < maxl; ++sidx) {
    pgemm::Launch W{}, D{};
    for (int k = 0; k < 2; ++k) {
      const int l = u->nl[k] - 1 - sidx;
      if (l < 0) continue;
      const int nout = u->dims[k][l + 1], nin = u->dims[k][l];
      pgemm::Problem &p = W.p[k];
      p.A = u->dY[k][l]; p.lda = u->ld(k, l);
      p.B = l == 0 ? u->rows0(k) : u->Y[k][l - 1];
      p.ldb = l == 0 ? nin : u->ld(k, l - 1);
      p.idx = l == 0 ? d_idx : nullptr;
      p.idx_limit = u->st.total_rows;
      p.C = u->dWp[k][l]; p.ldc = nin;
      p.dbias = u->dbp[k][l];
      p.M = nout; p.N = nin; p.K = rows;
      p.chunks = 1;                      // (launch_gemm sets the chunking)
      if (l == 0) continue;
      pgemm::Problem &q = D.p[k];
      q.A = u->dY[k][l]; q.lda = u->ld(k, l);
      q.B = v.w[k][l]; q.ldb = nin;
      q.C = u->dY[k][l - 1]; q.ldc = u->ld(k, l - 1);
      q.aux = u->Y[k][l - 1]; q.ldaux = u->ld(k, l - 1);
      q.M = rows; q.N = nin; q.K = nout;
      q.chunks = 1;
    }
    if (int rc = launch_gemm(pgemm::kBackwardWeight, W, s)) return rc;
    for (int k = 0; k < 2; ++k)
      if (u->nl[k] - 1 - sidx >= 0) dw_chunks[k][u->nl[k] - 1 - sidx] = W.p[k].chunks;
    if (int rc = launch_gemm(pgemm::kBackwardData, D, s)) return rc;
  }

  // the chunks in index order into .grad
  pgemm::ReduceTable rt{};
  int ne = 0, maxn = 0;
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < u->nl[k]; ++l) {
      const int nout = u->dims[k][l + 1], nin = u->dims[k][l];
      rt.e[ne++] = pgemm::ReduceEntry{u->dWp[k][l], u->grad[u->w_index(k, l)], nout * nin, dw_chunks[k][l]};
      rt.e[ne++] = pgemm::ReduceEntry{u->dbp[k][l], u->grad[u->b_index(k, l)], nout, dw_chunks[k][l]};
      maxn = nout * nin > maxn ? nout * nin : maxn;
    }
  pgemm::reduce(rt, ne, maxn, s);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_ppo_update_apply(mpc_ppo_update *u, double max_norm, double beta1, double beta2, double eps, int step, const double *d_lr, void *stream) {
  if (!u || !d_lr) return fail(MPC_E_ARG, "mpc_ppo_update_apply: bad argument");
  if (!(max_norm > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(eps))
    return fail(MPC_E_ARG, "mpc_ppo_update_apply: max_norm must be positive, the betas in [0, 1), eps not negative");
  if (step < 1) return fail(MPC_E_ARG, "mpc_ppo_update_apply: step counts from 1");
  if (!u->grads_bound || !u->moments_bound) return fail(MPC_E_ARG, "mpc_ppo_update_apply: no gradients and moments bound (mpc_ppo_update_bind)");
  mpc_ac_view v;
  if (!mpc_ac_get_view(u->ac, &v) || !v.bound) return fail(MPC_E_ARG, "mpc_ppo_update_apply: the mpc_ac has no parameters bound");
  DeviceGuard guard_(u->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  NormTable nt{};
  AdamTable at{};
  int maxn = 0;
  for (int t = 0; t < u->n_tensors; ++t) {
    nt.g[t] = u->grad[t];
    at.g[t] = u->grad[t]; at.m[t] = u->exp_avg[t]; at.v[t] = u->exp_avg_sq[t];
    nt.numel[t] = at.numel[t] = u->numel(t);
    maxn = at.numel[t] > maxn ? at.numel[t] : maxn;
  }
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < u->nl[k]; ++l) {
      at.p[u->w_index(k, l)] = const_cast<float *>(v.w[k][l]);
      at.p[u->b_index(k, l)] = const_cast<float *>(v.b[k][l]);
    }
  at.p[u->n_tensors - 1] = const_cast<float *>(v.std);
  hipLaunchKernelGGL(norm_partial_kernel, dim3((unsigned)u->norm_blocks, (unsigned)u->n_tensors), dim3(256), 0, s, nt, u->norm_partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(norm_kernel, dim3(1), dim3(kNormThreads), 0, s, u->n_tensors * u->norm_blocks, u->norm_partials, u->norm);
  HIP_TRY(hipGetLastError());
  ppo::AdamCfg cfg{beta1, beta2, eps, 1.0 - std::pow(beta1, (double)step), std::pow(1.0 - std::pow(beta2, (double)step), 0.5)};
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((maxn + 255) / 256), (unsigned)u->n_tensors), dim3(256), 0, s, at, cfg, (float)max_norm, u->norm, d_lr);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
