// mpc_recurrent_bptt.hip -- the C ABI of mpc_recurrent_bptt.h: the recurrent actor-critic's update through time on the device (recurrent_bptt.h).
//   seq_forward_kernel   grid (ceil(B / 16), memories): all T steps of 16 environments in one launch, h in LDS, c in registers; keeps the gate
//                        activations, c' and the state each step started from in the handle's workspace
//   transpose_kernel     W_hh -> W_hh^T, once per backward call
//   seq_backward_kernel  the same grid, t descending: dG[t] to LDS and the workspace, dh_rec = dG[t] W_hh on the MFMA pipe, dc_rec in registers
//   pgemm::launch        backward weight (ppo_gemm.h's gemm_kernel, which mpc_ppo_gemm.hip owns): dW_ih = dG^T X (X through the row index the
//                        forward launch wrote), then dW_hh = dG^T h_used; both memories in one launch each
//   column_sum_kernel    the column sums of dG per chunk of 256 rows, in float64
//   pgemm::reduce        the chunks in index order into the caller's gradient arrays
// The parameters are read through the caller's pointers.  No atomics, no scratch; nothing synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "mpc_host.h"
#include "mpc_recurrent_bptt.h"
#include "recurrent_bptt.h"
#include "recurrent_host.h"

using mpchost::aligned16;
using mpchost::any_overlap;
using mpchost::DeviceArray;
using mpchost::DeviceGuard;
using mpchost::Range;

static_assert(MPC_RECURRENT_BPTT_MEMORIES == recurrent::kMemories, "mpc_recurrent_bptt.h and recurrent_cell.h disagree");
static_assert(bptt::kSumRows == pgemm::kMinChunk, "the column sums' partials are counted with the GEMMs'");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

mpchost::LdsLimit g_forward_limit(bptt::seq_forward_kernel), g_backward_limit(bptt::seq_backward_kernel);
}  // namespace

struct mpc_recurrent_bptt {
  int memories = 0, device = -1, max_steps = 0, max_rows = 0, max_chunks = 0;
  recurrent::Cell cell[recurrent::kMemories]{};
  bptt::Work work[recurrent::kMemories]{};
  float *part_ih[recurrent::kMemories]{}, *part_hh[recurrent::kMemories]{}, *part_b[recurrent::kMemories]{};      // inside ws
  DeviceArray<float> ws[recurrent::kMemories];
  DeviceArray<long long> x_index[recurrent::kMemories];
  DeviceArray<int> flags;
  bptt::Seq fwd[recurrent::kMemories]{};      // the last forward call's rows
  size_t lds_forward = 0, lds_backward = 0;
  int fwd_T = 0, fwd_B = 0, fwd_first = 0, fwd_count = 0;      // fwd_count 0: none
  bool bound = false, went_back = false;      // went_back: dG is the last forward call's

  size_t rows() const { return (size_t)max_steps * max_rows; }
  size_t ws_floats(int k) const {
    const size_t H = cell[k].H, I = cell[k].I;
    return 11 * H * rows() + 4 * H * bptt::padded_cols((int)H) + (size_t)max_chunks * (4 * H * I + 4 * H * H + 4 * H);
  }
};

extern "C" {

const char *mpc_recurrent_bptt_last_error(void) { return g_err.c_str(); }

void mpc_recurrent_bptt_destroy(mpc_recurrent_bptt *h) { mpchost::destroy_handle(h); }

long long mpc_recurrent_bptt_workspace_bytes(const mpc_recurrent_bptt *h) {
  if (!h) return -1;
  size_t bytes = sizeof(int) * h->rows();
  for (int k = 0; k < h->memories; ++k) bytes += sizeof(float) * h->ws_floats(k) + sizeof(long long) * h->rows();
  return (long long)bytes;
}

int mpc_recurrent_bptt_dgates(const mpc_recurrent_bptt *h, int memory, const float **d_dg) {
  const std::string who = "mpc_recurrent_bptt_dgates: ";
  if (!h || !d_dg) return fail(MPC_E_ARG, who + "null argument");
  if (memory < 0 || memory >= h->memories) return fail(MPC_E_ARG, who + "memory " + std::to_string(memory) + " of a handle with " + std::to_string(h->memories));
  if (h->device < 0) return fail(MPC_E_ARG, who + "no workspace before mpc_recurrent_bptt_bind");
  *d_dg = h->work[memory].dG;
  return MPC_OK;
}

int mpc_recurrent_bptt_create(mpc_recurrent_bptt **out, int memories, const int *input_sizes, const int *hidden_sizes, int max_steps, int max_rows) {
  const std::string who = "mpc_recurrent_bptt_create: ";
  if (!out || !input_sizes || !hidden_sizes) return fail(MPC_E_ARG, who + "null argument");
  if (memories < 1 || memories > recurrent::kMemories) return fail(MPC_E_ARG, who + "one or two memories");
  if (max_steps < 1) return fail(MPC_E_ARG, who + "max_steps must be at least 1");
  if (max_rows < 1) return fail(MPC_E_ARG, who + "max_rows must be at least 1");
  size_t lf = 0, lb = 0;
  for (int k = 0; k < memories; ++k) {
    const int I = input_sizes[k], H = hidden_sizes[k];
    const std::string mem = who + "memory " + std::to_string(k) + ": ";
    const std::string why = recurrent::size_refusal(I, H);
    if (!why.empty()) return fail(MPC_E_ARG, mem + why);
    const size_t f = bptt::forward_lds_bytes(I, H), b = bptt::backward_lds_bytes(H);
    if (f > (size_t)MPC_RECURRENT_BPTT_MAX_LDS)
      return fail(MPC_E_ARG, mem + "the forward pass's two buffers of 16 rows of " + std::to_string(I) + " + " + std::to_string(H) + " floats need " + std::to_string(f) +
                                 " bytes of LDS, more than one CU's 160 KB");
    if (b > (size_t)MPC_RECURRENT_BPTT_MAX_LDS)
      return fail(MPC_E_ARG, mem + "the backward pass's 16 rows of 4 x " + std::to_string(H) + " floats need " + std::to_string(b) + " bytes of LDS, more than one CU's 160 KB");
    if ((long long)max_steps * max_rows * 4 * H > 0x7fffffffLL)
      return fail(MPC_E_ARG, mem + std::to_string(max_steps) + " x " + std::to_string(max_rows) + " rows of " + std::to_string(4 * H) + " floats pass 2^31 elements");
    lf = f > lf ? f : lf;
    lb = b > lb ? b : lb;
  }
  static_assert(16 * bptt::kWaves * bptt::kMaxSlots >= 624 && bptt::kQuadCols * bptt::kWaves * bptt::kMaxQuads >= 624, "the LDS bound (H <= 624) must fit the kernels' slots");
  mpc_recurrent_bptt *h = new mpc_recurrent_bptt();
  h->memories = memories;
  h->max_steps = max_steps;
  h->max_rows = max_rows;
  h->max_chunks = (int)((h->rows() + pgemm::kMinChunk - 1) / pgemm::kMinChunk);
  h->lds_forward = lf;
  h->lds_backward = lb;
  for (int k = 0; k < memories; ++k) {
    h->cell[k].I = input_sizes[k];
    h->cell[k].H = hidden_sizes[k];
  }
  *out = h;
  return MPC_OK;
}

int mpc_recurrent_bptt_bind(mpc_recurrent_bptt *h, const float *const *d_w_ih, const float *const *d_w_hh, const float *const *d_b_ih, const float *const *d_b_hh) {
  const std::string who = "mpc_recurrent_bptt_bind: ";
  if (!h) return fail(MPC_E_ARG, who + "null argument");
  const recurrent::Parameters params{d_w_ih, d_w_hh, d_b_ih, d_b_hh};
  const std::string why = recurrent::bind_refusal(params, h->memories);
  if (!why.empty()) return fail(MPC_E_ARG, who + why);
  if (h->device < 0) {                 // the first bind: the workspace
    const int dev = mpchost::current_device();
    if (dev < 0) return fail(MPC_E_NODEVICE, who + "no HIP device");
    const size_t R = h->rows();
    HIP_TRY(h->flags.alloc(R));
    for (int k = 0; k < h->memories; ++k) {
      const size_t H = h->cell[k].H, I = h->cell[k].I, wt = 4 * H * bptt::padded_cols((int)H);
      HIP_TRY(h->ws[k].alloc(h->ws_floats(k)));
      HIP_TRY(h->x_index[k].alloc(R));
      float *p = h->ws[k];
      bptt::Work &w = h->work[k];
      w.gates = p; p += 4 * H * R;
      w.c_new = p; p += H * R;
      w.h_used = p; p += H * R;
      w.c_used = p; p += H * R;
      w.dG = p; p += 4 * H * R;
      w.w_hh_t = p; p += wt;
      h->part_ih[k] = p; p += (size_t)h->max_chunks * 4 * H * I;
      h->part_hh[k] = p; p += (size_t)h->max_chunks * 4 * H * H;
      h->part_b[k] = p;
      w.db_part = p;
      w.x_index = h->x_index[k];
      HIP_TRY(hipMemset(w.w_hh_t, 0, sizeof(float) * wt));      // the rows past H stay zero
    }
    HIP_TRY(g_forward_limit.raise(dev, h->lds_forward));
    HIP_TRY(g_backward_limit.raise(dev, h->lds_backward));
    h->device = dev;
  }
  recurrent::bind(h->cell, params, h->memories);
  h->bound = true;
  return MPC_OK;
}

namespace {
int check_call(const std::string &who, const mpc_recurrent_bptt *h, int T, int B, int first, int count) {
  if (T < 1 || T > h->max_steps) return fail(MPC_E_ARG, who + "T = " + std::to_string(T) + " is outside 1 .. " + std::to_string(h->max_steps) + " (max_steps)");
  if (B < 1 || B > h->max_rows) return fail(MPC_E_ARG, who + "B = " + std::to_string(B) + " is outside 1 .. " + std::to_string(h->max_rows) + " (max_rows)");
  if (first < 0 || count < 1 || first + count > h->memories)
    return fail(MPC_E_ARG, who + "memories " + std::to_string(first) + " .. " + std::to_string(first + count - 1) + " of a handle with " + std::to_string(h->memories));
  return MPC_OK;
}
}  // namespace

int mpc_recurrent_bptt_forward(mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_io *io, const long long *d_reset, void *stream) {
  const std::string who = "mpc_recurrent_bptt_forward: ";
  if (!h || !io) return fail(MPC_E_ARG, who + "null argument");
  if (int rc = check_call(who, h, T, B, first, count)) return rc;
  if (reinterpret_cast<uintptr_t>(d_reset) & 7u) return fail(MPC_E_ARG, who + "d_reset must be 8-byte aligned");
  bptt::Seq seq[recurrent::kMemories]{};
  Range outs[2 * recurrent::kMemories];
  int n_outs = 0;
  for (int k = 0; k < count; ++k) {
    const mpc_recurrent_bptt_io &m = io[k];
    const int I = h->cell[first + k].I, H = h->cell[first + k].H;
    const std::string mem = who + "memory " + std::to_string(first + k) + ": ";
    if (!m.d_x || !m.d_h0 || !m.d_c0 || !m.d_y) return fail(MPC_E_ARG, mem + "d_x, d_h0, d_c0 or d_y is null");
    if (!aligned16(m.d_x) || !aligned16(m.d_h0) || !aligned16(m.d_c0) || !aligned16(m.d_y) || !aligned16(m.d_c_last))
      return fail(MPC_E_ARG, mem + "every pointer must be 16-byte aligned");
    if (m.x_stride < I || m.x_stride % 4 != 0)
      return fail(MPC_E_ARG, mem + "the x stride " + std::to_string(m.x_stride) + " must be a multiple of 4 floats and at least " + std::to_string(I) + " (one row)");
    outs[n_outs++] = Range{m.d_y, sizeof(float) * (size_t)T * B * H};
    outs[n_outs++] = Range{m.d_c_last, sizeof(float) * (size_t)B * H};
    seq[first + k] = bptt::Seq{m.d_x, m.x_stride, m.d_h0, m.d_c0, m.d_y, m.d_c_last, nullptr};
  }
  if (any_overlap(outs, n_outs)) return fail(MPC_E_ARG, who + "the output arrays must not overlap");
  if (!h->bound) return fail(MPC_E_ARG, who + "no parameters bound (mpc_recurrent_bptt_bind)");
  DeviceGuard guard_(h->device);
  bptt::Launch a{};
  for (int k = 0; k < h->memories; ++k) {
    a.cell[k] = h->cell[k];
    a.work[k] = h->work[k];
    a.seq[k] = seq[k];
    h->fwd[k] = seq[k];
  }
  h->fwd_count = 0;
  h->went_back = false;
  const dim3 grid((unsigned)((B + recurrent::kRows - 1) / recurrent::kRows), (unsigned)count);
  hipLaunchKernelGGL(bptt::seq_forward_kernel, grid, dim3(recurrent::kThreads), h->lds_forward, reinterpret_cast<hipStream_t>(stream), a, first, T, B, d_reset,
                     h->flags.get());
  HIP_TRY(hipGetLastError());
  h->fwd_T = T; h->fwd_B = B; h->fwd_first = first; h->fwd_count = count;
  return MPC_OK;
}

namespace {
// through_time: the transposition and the launch through time, then the weight gradients; without it the weight gradients of the dG that is there
int backward(const std::string &who, mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_grads *grads, void *stream, bool through_time) {
  if (!h || !grads) return fail(MPC_E_ARG, who + "null argument");
  if (int rc = check_call(who, h, T, B, first, count)) return rc;
  Range outs[4 * recurrent::kMemories];
  int n_outs = 0;
  for (int k = 0; k < count; ++k) {
    const mpc_recurrent_bptt_grads &g = grads[k];
    const size_t I = h->cell[first + k].I, H = h->cell[first + k].H;
    const std::string mem = who + "memory " + std::to_string(first + k) + ": ";
    if (!g.d_dy || !g.d_w_ih || !g.d_w_hh || !g.d_b_ih || !g.d_b_hh) return fail(MPC_E_ARG, mem + "d_dy or a gradient output is null");
    if (!aligned16(g.d_dy) || !aligned16(g.d_w_ih) || !aligned16(g.d_w_hh) || !aligned16(g.d_b_ih) || !aligned16(g.d_b_hh))
      return fail(MPC_E_ARG, mem + "every pointer must be 16-byte aligned");
    outs[n_outs++] = Range{g.d_w_ih, sizeof(float) * 4 * H * I};
    outs[n_outs++] = Range{g.d_w_hh, sizeof(float) * 4 * H * H};
    outs[n_outs++] = Range{g.d_b_ih, sizeof(float) * 4 * H};
    outs[n_outs++] = Range{g.d_b_hh, sizeof(float) * 4 * H};
  }
  if (any_overlap(outs, n_outs)) return fail(MPC_E_ARG, who + "the gradient arrays must not overlap");
  if (h->fwd_count == 0) return fail(MPC_E_ARG, who + "no forward call to go back through (mpc_recurrent_bptt_forward)");
  if (T != h->fwd_T || B != h->fwd_B || first != h->fwd_first || count != h->fwd_count)
    return fail(MPC_E_ARG, who + "T = " + std::to_string(T) + ", B = " + std::to_string(B) + ", memories " + std::to_string(first) + " .. " +
                               std::to_string(first + count - 1) + " do not match the last forward call's T = " + std::to_string(h->fwd_T) + ", B = " +
                               std::to_string(h->fwd_B) + ", memories " + std::to_string(h->fwd_first) + " .. " + std::to_string(h->fwd_first + h->fwd_count - 1));
  if (!through_time && !h->went_back) return fail(MPC_E_ARG, who + "no backward call since the last forward call: there is no dG (mpc_recurrent_bptt_backward)");
  DeviceGuard guard_(h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  bptt::Launch a{};
  for (int k = 0; k < h->memories; ++k) {
    a.cell[k] = h->cell[k];
    a.work[k] = h->work[k];
    a.seq[k] = h->fwd[k];
  }
  int maxhh = 0;
  for (int k = 0; k < count; ++k) {
    a.seq[first + k].dy = grads[k].d_dy;
    const int H = h->cell[first + k].H;
    maxhh = 4 * H * H > maxhh ? 4 * H * H : maxhh;
  }
  if (through_time) {
    hipLaunchKernelGGL(bptt::transpose_kernel, dim3((unsigned)((maxhh + recurrent::kThreads - 1) / recurrent::kThreads), (unsigned)count), dim3(recurrent::kThreads), 0, s,
                       a, first);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((B + recurrent::kRows - 1) / recurrent::kRows), (unsigned)count);
    hipLaunchKernelGGL(bptt::seq_backward_kernel, grid, dim3(recurrent::kThreads), h->lds_backward, s, a, first, T, B, h->flags.get());
    HIP_TRY(hipGetLastError());
    h->went_back = true;
  }

  // dW_ih, then dW_hh, then the column sums of dG: the memories side by side in each launch
  const int R = T * B;
  pgemm::Launch Wi{}, Wh{};
  for (int k = 0; k < count; ++k) {
    const int m = first + k, I = h->cell[m].I, H = h->cell[m].H;
    pgemm::Problem &p = Wi.p[k];
    p.A = h->work[m].dG; p.lda = 4 * H;
    p.B = h->fwd[m].x; p.ldb = 4;      // row (t, b) starts x_index quads of 4 floats after x
    p.idx = h->work[m].x_index;
    p.idx_limit = (((long long)(T - 1) * h->fwd[m].x_stride + (long long)(B - 1) * I) >> 2) + 1;
    p.C = h->part_ih[m]; p.ldc = I;
    p.M = 4 * H; p.N = I; p.K = R;
    p.chunks = 1;                      // (pgemm::launch sets the chunking)
    pgemm::Problem &q = Wh.p[k];
    q.A = h->work[m].dG; q.lda = 4 * H;
    q.B = h->work[m].h_used; q.ldb = H;
    q.C = h->part_hh[m]; q.ldc = H;
    q.M = 4 * H; q.N = H; q.K = R;
    q.chunks = 1;
  }
  for (pgemm::Launch *L : {&Wi, &Wh}) {
    pgemm::launch(pgemm::kBackwardWeight, *L, s);
    HIP_TRY(hipGetLastError());
  }
  int maxg = 0;
  for (int k = 0; k < count; ++k) maxg = 4 * h->cell[first + k].H > maxg ? 4 * h->cell[first + k].H : maxg;
  const int sum_chunks = (R + bptt::kSumRows - 1) / bptt::kSumRows;
  hipLaunchKernelGGL(bptt::column_sum_kernel, dim3((unsigned)((maxg + recurrent::kThreads - 1) / recurrent::kThreads), (unsigned)sum_chunks, (unsigned)count),
                     dim3(recurrent::kThreads), 0, s, a, first, R);
  HIP_TRY(hipGetLastError());
  pgemm::ReduceTable rt{};
  int ne = 0, maxn = 0;
  for (int k = 0; k < count; ++k) {
    const int m = first + k, I = h->cell[m].I, H = h->cell[m].H;
    rt.e[ne++] = pgemm::ReduceEntry{h->part_ih[m], grads[k].d_w_ih, 4 * H * I, Wi.p[k].chunks};
    rt.e[ne++] = pgemm::ReduceEntry{h->part_hh[m], grads[k].d_w_hh, 4 * H * H, Wh.p[k].chunks};
    rt.e[ne++] = pgemm::ReduceEntry{h->part_b[m], grads[k].d_b_ih, 4 * H, sum_chunks};
    rt.e[ne++] = pgemm::ReduceEntry{h->part_b[m], grads[k].d_b_hh, 4 * H, sum_chunks};
    const int big = 4 * H * (I > H ? I : H);
    maxn = big > maxn ? big : maxn;
  }
  pgemm::reduce(rt, ne, maxn, s);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}
}  // namespace

int mpc_recurrent_bptt_backward(mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_grads *grads, void *stream) {
  return backward("mpc_recurrent_bptt_backward: ", h, T, B, first, count, grads, stream, true);
}

int mpc_recurrent_bptt_weight_gradients(mpc_recurrent_bptt *h, int T, int B, int first, int count, const mpc_recurrent_bptt_grads *grads, void *stream) {
  return backward("mpc_recurrent_bptt_weight_gradients: ", h, T, B, first, count, grads, stream, false);
}

}  // extern "C"
