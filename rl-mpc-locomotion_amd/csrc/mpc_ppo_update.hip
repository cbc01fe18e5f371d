// mpc_ppo_update.hip -- the C ABI of include/mpc_ppo_update.h: the update half of a PPO iteration on the device.
//   pgemm::launch        forward, backward-data and backward-weight GEMMs of both nets (mpc_ppo_gemm.hip), actor and critic in one launch per layer
//   head_kernel          one lane per row: ppo::head_row on the forward pass's mean and value and the indexed storage rows; writes d loss / d mu and
//                        d loss / d V where the backward pass reads them, and one float64 partial per workgroup and quantity (fixed-order LDS sums)
//   head_reduce_kernel   ONE workgroup joins the partials in index order: the four terms, d loss / d std, the learning-rate decision
//   pgemm::reduce        the weight-gradient chunks, and the bias gradients, summed in index order into the .grad tensors
//   norm_partial_kernel  the sum of squares of every gradient element in float64, one partial per 4096 elements of a tensor (fixed-order LDS tree), and
//   norm_kernel          ONE workgroup joins the partials in a fixed order, as normalise_kernel of mpc_ppo.hip does
//   adam_kernel          every parameter tensor in one launch (blockIdx.y picks the tensor): ppo::adam_element
// mpc_ppo_update_grads_sequence is the same sequence on dense first-layer rows (the outputs of a recurrent actor-critic's memories) plus one
// pgemm::kBackwardDataLinear launch through layer 0 into the rows' gradients; mpc_ppo_update_bind_extra puts up to eight more tensors (the memories'
// parameters) behind the mpc_ac's in the norm, the clip and Adam.
// mpc_ppo_update_grads_distill (policy distillation) is the sequence over the ACTOR alone, the critic's slot of every GEMM launch empty, with
// bc_head_kernel / bc_reduce_kernel (ppo::bc_element against the teacher's actions) for the loss head; mpc_ppo_update_apply_actor is the norm, the
// clip and Adam over the actor's weights and biases alone.  Neither reads or writes anything of the critic's or std's.
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
constexpr int kMaxExtra = MPC_PPO_UPDATE_MAX_EXTRA;      // tensors of mpc_ppo_update_bind_extra
constexpr int kMaxTensors = 4 * MPC_AC_MAX_LAYERS + 1 + kMaxExtra;

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

// The head of policy distillation (mpc_ppo_update_grads_distill): one lane per row, ppo::bc_element on the actor's mean and the teacher's action of
// storage row idx[row]; writes d loss / d mu where the backward pass reads it, and per workgroup the float64 sums of the loss terms and of |d| --
// a row's twelve elements in action order, then head_kernel's fixed-order LDS sums over the rows
constexpr int kBcQ = 2;                        // loss, |mu - target|
__global__ __launch_bounds__(kHeadThreads) void bc_head_kernel(int rows, const long long *__restrict__ idx, long long total_rows, int loss_type, float norm,
                                                               const float *__restrict__ targets, const float *__restrict__ mu, float *__restrict__ dmu,
                                                               double *__restrict__ partials) {
  __shared__ double vals[kBcQ][kHeadThreads];
  __shared__ double mid[kBcQ][16];
  const int t = threadIdx.x, row = blockIdx.x * kHeadThreads + t;
  double loss = 0.0, gap = 0.0;
  if (row < rows) {
    long long r = idx[row];
    r = r < 0 ? 0 : (r >= total_rows ? total_rows - 1 : r);
    float m[ppo::kActions], a[ppo::kActions], g[ppo::kActions];
#pragma unroll
    for (int k = 0; k < ppo::kActions; k += 4) {
      *reinterpret_cast<float4 *>(m + k) = *reinterpret_cast<const float4 *>(mu + (size_t)row * kOutLd + k);
      *reinterpret_cast<float4 *>(a + k) = *reinterpret_cast<const float4 *>(targets + (size_t)r * ppo::kActions + k);
    }
#pragma unroll
    for (int k = 0; k < ppo::kActions; ++k) {
      float value, d;
      ppo::bc_element(loss_type, norm, m[k], a[k], value, g[k], d);
      loss += (double)value;
      gap += (double)d;
    }
#pragma unroll
    for (int k = 0; k < ppo::kActions; k += 4)
      *reinterpret_cast<float4 *>(dmu + (size_t)row * kOutLd + k) = *reinterpret_cast<const float4 *>(g + k);
  }
  vals[0][t] = loss; vals[1][t] = gap;
  __syncthreads();
  if (t < kBcQ * 16) {                   // 16 consecutive rows each, in row order
    const int q = t >> 4, j = t & 15;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += vals[q][16 * j + i];
    mid[q][j] = sum;
  }
  __syncthreads();
  if (t < kBcQ) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) sum += mid[t][j];
    partials[(size_t)blockIdx.x * kHeadStride + t] = sum;
  }
}

// ONE workgroup joins bc_head_kernel's partials as head_reduce_kernel does: terms = (mean loss, mean |d|) over the 12 rows elements
__global__ __launch_bounds__(64) void bc_reduce_kernel(int blocks, int rows, const double *__restrict__ partials, float *__restrict__ terms) {
  __shared__ double mid[kBcQ][16];
  const int t = threadIdx.x;
  if (t < kBcQ * 16) {
    const int q = t >> 4, j = t & 15, per = (blocks + 15) / 16;
    const int b1 = (j + 1) * per < blocks ? (j + 1) * per : blocks;
    double sum = 0.0;
    for (int b = j * per; b < b1; ++b) sum += partials[(size_t)b * kHeadStride + q];
    mid[q][j] = sum;
  }
  __syncthreads();
  if (t >= kBcQ) return;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += mid[t][j];
  terms[t] = (float)(s / ((double)ppo::kActions * (double)rows));
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
  size_t ws_words = 0;
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
  const float *distill_targets = nullptr;       // [total_rows][12] (mpc_ppo_update_set_distill_targets): the teacher's actions, indexed like st.obs
  const float *seq_rows[2] = {};                // mpc_ppo_update_set_sequence_rows: dense [max_rows][dims[k][0]] inputs of the two first layers ...
  float *seq_drows[2] = {};                     // ... and what receives d loss / d rows
  bool sequence_set = false;
  int n_extra = 0;                              // mpc_ppo_update_bind_extra: tensors n_tensors .. n_tensors + n_extra of the norm, the clip and Adam
  float *extra_param[kMaxExtra] = {};
  int extra_numel[kMaxExtra] = {};
  bool extra_moments = false;
  mpchost::DeviceArray<double> extra_partials;  // [n_tensors + n_extra][blocks over all of them]: the norm's partials while extras are bound
  size_t extra_capacity = 0;
  int extra_blocks = 0;

  // the rows layer 0 of net k reads through the index
  const float *rows0(int k) const { return k == kCritic && critic_obs ? critic_obs : st.obs; }
  int ld(int k, int l) const { return l + 1 == nl[k] ? kOutLd : dims[k][l + 1]; }
  // mpc_ac_bind's order: actor weights, actor biases, critic weights, critic biases, std
  int w_index(int k, int l) const { return (k == kActor ? 0 : 2 * nl[0]) + l; }
  int b_index(int k, int l) const { return (k == kActor ? nl[0] : 2 * nl[0] + nl[1]) + l; }
  int numel(int t) const {
    if (t >= n_tensors) return t < n_tensors + n_extra ? extra_numel[t - n_tensors] : 0;
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

int mpc_ppo_update_layer_gradient(const mpc_ppo_update *u, int net, int layer, float **d_out, int *ld) {
  if (!u || !d_out || !ld) return fail(MPC_E_ARG, "mpc_ppo_update_layer_gradient: bad argument");
  if (net < 0 || net > 1 || layer < 0 || layer >= u->nl[net]) return fail(MPC_E_ARG, "mpc_ppo_update_layer_gradient: no such net or layer");
  *d_out = u->dY[net][layer];
  *ld = u->ld(net, layer);
  return MPC_OK;
}

long long mpc_ppo_update_workspace_bytes(const mpc_ppo_update *u) { return u ? (long long)(4 * u->ws_words + 8 * u->extra_capacity) : -1; }

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
  u->ws_words = words;
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

}  // extern "C"

namespace {
int forward_pass(mpc_ppo_update *u, const mpc_ac_view &v, int nets, bool sequence, int rows, const long long *d_idx, hipStream_t s);
int backward_pass(mpc_ppo_update *u, const mpc_ac_view &v, int nets, bool sequence, int rows, const long long *d_idx, hipStream_t s);

// mpc_ppo_update_grads (sequence = false: layer 0 reads the storage's rows through d_idx) and mpc_ppo_update_grads_sequence (true: layer 0 reads the
// dense rows of mpc_ppo_update_set_sequence_rows, and one more launch takes dY_0 W_0 into their gradients); `name` heads the refusals
int grads(const char *name, bool sequence, mpc_ppo_update *u, int rows, const long long *d_idx, double clip_param, double value_loss_coef,
          double entropy_coef, int use_clipped_value_loss, int adaptive, double desired_kl, double *d_lr, float *d_terms, void *stream) {
  if (!u || !d_idx || !d_terms) return fail(MPC_E_ARG, std::string(name) + ": bad argument");
  if (rows <= 0 || rows > u->max_rows) return fail(MPC_E_ARG, std::string(name) + ": rows must lie in 1 .. max_rows");
  if (!std::isfinite(clip_param) || clip_param <= 0.0 || !std::isfinite(value_loss_coef) || !std::isfinite(entropy_coef))
    return fail(MPC_E_ARG, std::string(name) + ": clip_param must be positive and the coefficients finite");
  if (adaptive && (!d_lr || !(desired_kl > 0.0) || !std::isfinite(desired_kl)))
    return fail(MPC_E_ARG, std::string(name) + ": the adaptive schedule needs d_lr and a positive desired_kl");
  if (!u->grads_bound) return fail(MPC_E_ARG, std::string(name) + ": no gradients bound (mpc_ppo_update_bind)");
  if (!u->storage_set) return fail(MPC_E_ARG, std::string(name) + ": no storage set (mpc_ppo_update_set_storage)");
  if (sequence && !u->sequence_set) return fail(MPC_E_ARG, std::string(name) + ": no dense rows set (mpc_ppo_update_set_sequence_rows)");
  mpc_ac_view v;
  if (!mpc_ac_get_view(u->ac, &v) || !v.bound) return fail(MPC_E_ARG, std::string(name) + ": the mpc_ac has no parameters bound");
  if (!sequence && v.asymmetric && !u->critic_obs)
    return fail(MPC_E_ARG, std::string(name) + ": an asymmetric mpc_ac needs the critic's rows (mpc_ppo_update_set_critic_storage)");
  DeviceGuard guard_(u->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = forward_pass(u, v, 2, sequence, rows, d_idx, s)) return rc;

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
  return backward_pass(u, v, 2, sequence, rows, d_idx, s);
}

// The passes of `grads` over the first `nets` nets: 2 is actor and critic side by side; 1 is the actor alone (mpc_ppo_update_grads_distill), the
// critic's slot of every launch empty and nothing of the critic's read or written.
int forward_pass(mpc_ppo_update *u, const mpc_ac_view &v, int nets, bool sequence, int rows, const long long *d_idx, hipStream_t s) {
  int maxl = 0;
  for (int k = 0; k < nets; ++k) maxl = u->nl[k] > maxl ? u->nl[k] : maxl;

  // forward: layer l of both nets side by side.  (tests/test_ppo_gemm_plan.py restates this sequence of launches and their (M, N, K), here and in the
  // backward loop below, to pin which kernels the tests reach: a launch added, dropped or reshaped here has to be restated there)
  for (int l = 0; l < maxl; ++l) {
    pgemm::Launch L{};
    for (int k = 0; k < nets; ++k) {
      if (l >= u->nl[k]) continue;
      pgemm::Problem &p = L.p[k];
      p.A = l == 0 ? (sequence ? u->seq_rows[k] : u->rows0(k)) : u->Y[k][l - 1];
      p.idx = l == 0 && !sequence ? d_idx : nullptr;
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
  return MPC_OK;
}

int backward_pass(mpc_ppo_update *u, const mpc_ac_view &v, int nets, bool sequence, int rows, const long long *d_idx, hipStream_t s) {
  int maxl = 0;
  for (int k = 0; k < nets; ++k) maxl = u->nl[k] > maxl ? u->nl[k] : maxl;

  // backward: from the last layer of each net towards the first; dW partials, then dX into the layer below
  int dw_chunks[2][MPC_AC_MAX_LAYERS] = {};
  for (int sidx = 0; sidx < maxl; ++sidx) {
    pgemm::Launch W{}, D{};
    for (int k = 0; k < nets; ++k) {
      const int l = u->nl[k] - 1 - sidx;
      if (l < 0) continue;
      const int nout = u->dims[k][l + 1], nin = u->dims[k][l];
      pgemm::Problem &p = W.p[k];
      p.A = u->dY[k][l]; p.lda = u->ld(k, l);
      p.B = l == 0 ? (sequence ? u->seq_rows[k] : u->rows0(k)) : u->Y[k][l - 1];
      p.ldb = l == 0 ? nin : u->ld(k, l - 1);
      p.idx = l == 0 && !sequence ? d_idx : nullptr;
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
    for (int k = 0; k < nets; ++k)
      if (u->nl[k] - 1 - sidx >= 0) dw_chunks[k][u->nl[k] - 1 - sidx] = W.p[k].chunks;
    if (int rc = launch_gemm(pgemm::kBackwardData, D, s)) return rc;
  }
  if (sequence) {                        // through layer 0 into the rows' gradients: d rows = dY_0 W_0, no activation in front of these rows
    pgemm::Launch D{};
    for (int k = 0; k < nets; ++k) {
      pgemm::Problem &q = D.p[k];
      q.A = u->dY[k][0]; q.lda = u->ld(k, 0);
      q.B = v.w[k][0]; q.ldb = u->dims[k][0];
      q.C = u->seq_drows[k]; q.ldc = u->dims[k][0];
      q.M = rows; q.N = u->dims[k][0]; q.K = u->dims[k][1];
      q.chunks = 1;
    }
    if (int rc = launch_gemm(pgemm::kBackwardDataLinear, D, s)) return rc;
  }

  // the chunks in index order into .grad
  pgemm::ReduceTable rt{};
  int ne = 0, maxn = 0;
  for (int k = 0; k < nets; ++k)
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

// [a, a + n) and [b, b + m) floats share an address
bool overlap(const float *a, size_t n, const float *b, size_t m) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + 4 * m && b0 < a0 + 4 * n;
}
}  // namespace

extern "C" {

int mpc_ppo_update_grads(mpc_ppo_update *u, int rows, const long long *d_idx, double clip_param, double value_loss_coef, double entropy_coef,
                         int use_clipped_value_loss, int adaptive, double desired_kl, double *d_lr, float *d_terms, void *stream) {
  return grads("mpc_ppo_update_grads", false, u, rows, d_idx, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, adaptive, desired_kl, d_lr,
               d_terms, stream);
}

int mpc_ppo_update_grads_sequence(mpc_ppo_update *u, int rows, const long long *d_idx, double clip_param, double value_loss_coef, double entropy_coef,
                                  int use_clipped_value_loss, int adaptive, double desired_kl, double *d_lr, float *d_terms, void *stream) {
  return grads("mpc_ppo_update_grads_sequence", true, u, rows, d_idx, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, adaptive,
               desired_kl, d_lr, d_terms, stream);
}

int mpc_ppo_update_set_sequence_rows(mpc_ppo_update *u, const float *d_rows_actor, const float *d_rows_critic, float *d_drows_actor,
                                     float *d_drows_critic) {
  const void *all[4] = {d_rows_actor, d_rows_critic, d_drows_actor, d_drows_critic};
  int given = 0;
  for (const void *p : all) given += p != nullptr;
  if (given != 0 && given != 4) return fail(MPC_E_ARG, "mpc_ppo_update_set_sequence_rows: all four buffers, or four NULLs to clear them");
  for (const void *p : all)
    if (!mpchost::aligned16(p)) return fail(MPC_E_ARG, "mpc_ppo_update_set_sequence_rows: every buffer must be 16-byte aligned");
  if (given && (d_drows_actor == d_drows_critic || d_drows_actor == d_rows_actor || d_drows_actor == d_rows_critic || d_drows_critic == d_rows_actor ||
                d_drows_critic == d_rows_critic))
    return fail(MPC_E_ARG, "mpc_ppo_update_set_sequence_rows: the gradient buffers must not overlap each other or the rows");
  if (!u) return fail(MPC_E_ARG, "mpc_ppo_update_set_sequence_rows: bad argument");
  if (given) {
    const size_t na = (size_t)u->max_rows * u->dims[kActor][0], nc = (size_t)u->max_rows * u->dims[kCritic][0];
    if (overlap(d_drows_actor, na, d_drows_critic, nc) || overlap(d_drows_actor, na, d_rows_actor, na) || overlap(d_drows_actor, na, d_rows_critic, nc) ||
        overlap(d_drows_critic, nc, d_rows_actor, na) || overlap(d_drows_critic, nc, d_rows_critic, nc))
      return fail(MPC_E_ARG, "mpc_ppo_update_set_sequence_rows: the gradient buffers must not overlap each other or the rows");
  }
  u->seq_rows[kActor] = d_rows_actor; u->seq_rows[kCritic] = d_rows_critic;
  u->seq_drows[kActor] = d_drows_actor; u->seq_drows[kCritic] = d_drows_critic;
  u->sequence_set = given == 4;
  return MPC_OK;
}

int mpc_ppo_update_bind_extra(mpc_ppo_update *u, int count, float *const *d_params, float *const *d_grads, float *const *d_exp_avg,
                              float *const *d_exp_avg_sq, const int *numel) {
  if (count < 0 || count > kMaxExtra) return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: count must lie in 0 .. 8");
  if (count > 0 && (!d_params || !d_grads || !numel)) return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: bad argument");
  if ((d_exp_avg == nullptr) != (d_exp_avg_sq == nullptr)) return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: both moments or neither");
  for (int t = 0; t < count; ++t) {
    if (numel[t] <= 0) return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: every tensor has at least one element");
    if (!present16(d_params[t]) || !present16(d_grads[t]) || (d_exp_avg && (!present16(d_exp_avg[t]) || !present16(d_exp_avg_sq[t]))))
      return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: every parameter, gradient and moment pointer must be non-null and 16-byte aligned");
  }
  if (!u) return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: bad argument");
  if (count > 0 && !u->grads_bound) return fail(MPC_E_ARG, "mpc_ppo_update_bind_extra: bind the mpc_ac's tensors first (mpc_ppo_update_bind)");
  if (count > 0) {                       // the norm's partials over all tensors: the one allocation, after every refusal
    int maxn = 0;
    for (int t = 0; t < u->n_tensors; ++t) maxn = u->numel(t) > maxn ? u->numel(t) : maxn;
    for (int t = 0; t < count; ++t) maxn = numel[t] > maxn ? numel[t] : maxn;
    const int blocks = (maxn + kNormPerBlock - 1) / kNormPerBlock;
    const size_t need = (size_t)(u->n_tensors + count) * blocks;
    if (u->extra_capacity < need) {
      DeviceGuard guard_(u->device);
      u->extra_capacity = 0;
      u->n_extra = 0;                    // (alloc frees what was there: nothing stays bound to it if it fails)
      if (u->extra_partials.alloc(need) != hipSuccess) return fail(MPC_E_HIP, "mpc_ppo_update_bind_extra: the norm's partials could not be allocated");
      u->extra_capacity = need;
    }
    u->extra_blocks = blocks;
  }
  u->n_extra = count;
  for (int t = 0; t < count; ++t) {
    const int k = u->n_tensors + t;
    u->extra_param[t] = d_params[t];
    u->extra_numel[t] = numel[t];
    u->grad[k] = d_grads[t];
    u->exp_avg[k] = d_exp_avg ? d_exp_avg[t] : nullptr;
    u->exp_avg_sq[k] = d_exp_avg ? d_exp_avg_sq[t] : nullptr;
  }
  u->extra_moments = count > 0 && d_exp_avg != nullptr;
  return MPC_OK;
}

}  // extern "C"

namespace {
// mpc_ppo_update_apply (actor_only = false: every tensor of the mpc_ac and the extras behind them) and mpc_ppo_update_apply_actor (true: the actor's
// weights and biases, which head mpc_ac_bind's order; no other tensor, gradient or moment enters a table)
int apply(const char *name, bool actor_only, mpc_ppo_update *u, double max_norm, double beta1, double beta2, double eps, int step, const double *d_lr,
          void *stream) {
  const std::string who(name);
  if (!u || !d_lr) return fail(MPC_E_ARG, who + ": bad argument");
  if (!(max_norm > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(eps))
    return fail(MPC_E_ARG, who + ": max_norm must be positive, the betas in [0, 1), eps not negative");
  if (step < 1) return fail(MPC_E_ARG, who + ": step counts from 1");
  if (!u->grads_bound || !u->moments_bound) return fail(MPC_E_ARG, who + ": no gradients and moments bound (mpc_ppo_update_bind)");
  const int n_extra = actor_only ? 0 : u->n_extra;
  if (n_extra > 0 && !u->extra_moments) return fail(MPC_E_ARG, who + ": the extra tensors have no moments bound (mpc_ppo_update_bind_extra)");
  mpc_ac_view v;
  if (!mpc_ac_get_view(u->ac, &v) || !v.bound) return fail(MPC_E_ARG, who + ": the mpc_ac has no parameters bound");
  DeviceGuard guard_(u->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  NormTable nt{};
  AdamTable at{};
  int maxn = 0;
  const int total = actor_only ? 2 * u->nl[kActor] : u->n_tensors + n_extra;      // (no extras: today's tables, partials and grids)
  const int blocks = n_extra > 0 ? u->extra_blocks : u->norm_blocks;
  double *partials = n_extra > 0 ? static_cast<double *>(u->extra_partials) : u->norm_partials;
  for (int t = 0; t < total; ++t) {
    nt.g[t] = u->grad[t];
    at.g[t] = u->grad[t]; at.m[t] = u->exp_avg[t]; at.v[t] = u->exp_avg_sq[t];
    nt.numel[t] = at.numel[t] = u->numel(t);
    maxn = at.numel[t] > maxn ? at.numel[t] : maxn;
  }
  for (int k = 0; k < (actor_only ? 1 : 2); ++k)
    for (int l = 0; l < u->nl[k]; ++l) {
      at.p[u->w_index(k, l)] = const_cast<float *>(v.w[k][l]);
      at.p[u->b_index(k, l)] = const_cast<float *>(v.b[k][l]);
    }
  if (!actor_only) at.p[u->n_tensors - 1] = const_cast<float *>(v.std);
  for (int t = 0; t < n_extra; ++t) at.p[u->n_tensors + t] = u->extra_param[t];
  hipLaunchKernelGGL(norm_partial_kernel, dim3((unsigned)blocks, (unsigned)total), dim3(256), 0, s, nt, partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(norm_kernel, dim3(1), dim3(kNormThreads), 0, s, total * blocks, partials, u->norm);
  HIP_TRY(hipGetLastError());
  ppo::AdamCfg cfg{beta1, beta2, eps, 1.0 - std::pow(beta1, (double)step), std::pow(1.0 - std::pow(beta2, (double)step), 0.5)};
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((maxn + 255) / 256), (unsigned)total), dim3(256), 0, s, at, cfg, (float)max_norm, u->norm, d_lr);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}
}  // namespace

extern "C" {

int mpc_ppo_update_apply(mpc_ppo_update *u, double max_norm, double beta1, double beta2, double eps, int step, const double *d_lr, void *stream) {
  return apply("mpc_ppo_update_apply", false, u, max_norm, beta1, beta2, eps, step, d_lr, stream);
}

int mpc_ppo_update_apply_actor(mpc_ppo_update *u, double max_norm, double beta1, double beta2, double eps, int step, const double *d_lr, void *stream) {
  return apply("mpc_ppo_update_apply_actor", true, u, max_norm, beta1, beta2, eps, step, d_lr, stream);
}

int mpc_ppo_update_set_distill_targets(mpc_ppo_update *u, const float *d_teacher_actions) {
  if (!mpchost::aligned16(d_teacher_actions)) return fail(MPC_E_ARG, "mpc_ppo_update_set_distill_targets: d_teacher_actions must be 16-byte aligned");
  if (!u) return fail(MPC_E_ARG, "mpc_ppo_update_set_distill_targets: bad argument");
  u->distill_targets = d_teacher_actions;       // (null: cleared)
  return MPC_OK;
}

int mpc_ppo_update_grads_distill(mpc_ppo_update *u, int rows, const long long *d_idx, int loss_type, float *d_terms, void *stream) {
  if (!u || !d_idx || !d_terms) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: bad argument");
  if (rows <= 0 || rows > u->max_rows) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: rows must lie in 1 .. max_rows");
  if (loss_type != ppo::kBcMse && loss_type != ppo::kBcHuber) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: loss_type is 0 (mse) or 1 (huber)");
  if (!u->grads_bound) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: no gradients bound (mpc_ppo_update_bind)");
  if (!u->storage_set) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: no storage set (mpc_ppo_update_set_storage)");
  if (!u->distill_targets) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: no targets set (mpc_ppo_update_set_distill_targets)");
  mpc_ac_view v;
  if (!mpc_ac_get_view(u->ac, &v) || !v.bound) return fail(MPC_E_ARG, "mpc_ppo_update_grads_distill: the mpc_ac has no parameters bound");
  DeviceGuard guard_(u->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = forward_pass(u, v, 1, false, rows, d_idx, s)) return rc;
  const int hb = (rows + kHeadThreads - 1) / kHeadThreads, la = u->nl[kActor] - 1;
  hipLaunchKernelGGL(bc_head_kernel, dim3((unsigned)hb), dim3(kHeadThreads), 0, s, rows, d_idx, u->st.total_rows, loss_type, ppo::bc_norm(loss_type, rows),
                     u->distill_targets, u->Y[kActor][la], u->dY[kActor][la], u->partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(bc_reduce_kernel, dim3(1), dim3(64), 0, s, hb, rows, u->partials, d_terms);
  HIP_TRY(hipGetLastError());
  return backward_pass(u, v, 1, false, rows, d_idx, s);
}

}  // extern "C"
