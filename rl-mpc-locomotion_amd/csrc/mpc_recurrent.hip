// mpc_recurrent.hip -- the C ABI of mpc_recurrent.h: the LSTM cell step of the recurrent actor-critic's memories (recurrent_cell.h) on the device.
//   cell_kernel        grid (ceil(n / 16), memories), blockIdx.y picks the memory, so the critic's workgroups run beside the actor's (ac_kernel's
//                      arrangement).  A workgroup stages the x and h rows of 16 environments in LDS (the reset applied to h there, the saved
//                      copy written from there), then each wave takes blocks of 16 state columns with their four gate blocks on the fp32 MFMA pipe
//                      and finishes the cell in registers.  The parameters are read through the caller's pointers: nothing is copied at bind time
//                      or later.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "mpc_host.h"
#include "mpc_recurrent.h"
#include "recurrent_cell.h"
#include "recurrent_host.h"

using mpchost::aligned16;
using mpchost::DeviceGuard;

static_assert(MPC_RECURRENT_MEMORIES == recurrent::kMemories, "mpc_recurrent.h and recurrent_cell.h disagree");
static_assert(sizeof(mpc_recurrent_io) == sizeof(recurrent::Io), "mpc_recurrent_io is recurrent::Io");

namespace {
using namespace recurrent;

thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

// grid (ceil(n / 16), memories); memory = first + blockIdx.y.  reset [n] int64 or null: where non-zero, the state of that row is taken as zero.
// commit 0: h and c are left as they are and h_out alone is written.
__global__ __launch_bounds__(kThreads) void cell_kernel(Launch a, int first, int n, const long long *__restrict__ reset, int commit) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int which = first + (int)blockIdx.y;
  const Cell &m = a.cell[which];
  const Io &io = a.io[which];
  const int I = m.I, H = m.H, xs = I + kPad, hs = H + kPad;
  float *xb = lds, *hb = lds + kRows * xs;
  const int r0 = blockIdx.x * kRows;
  stage<kThreads>(xb, xs, io.x, nullptr, I, r0, n, nullptr);
  stage<kThreads>(hb, hs, io.h, io.h_saved, H, r0, n, reset);
  __syncthreads();                     // every read of this workgroup's rows of h lies before it, every store to them after it
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  for (int nb = wave; nb * 16 < H; nb += kWaves) {
    f32x4 acc[kGates];
#pragma unroll
    for (int g = 0; g < kGates; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    accumulate(acc, xb, xs, m.w_ih, I, H, nb);
    accumulate(acc, hb, hs, m.w_hh, H, H, nb);
    const int j = nb * 16 + col;
    float bias[kGates];
#pragma unroll
    for (int g = 0; g < kGates; ++g) bias[g] = m.b_ih[g * H + j] + m.b_hh[g * H + j];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {  // C layout of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg
      const int row = r0 + 4 * q + reg;
      if (row >= n) continue;
      const size_t o = (size_t)row * H + j;
      const float c0 = (reset && reset[row] != 0) ? 0.f : io.c[o];
      const Step s = finish(acc, bias, reg, c0);
      if (io.c_saved) io.c_saved[o] = c0;
      if (commit) {
        io.c[o] = s.c;
        io.h[o] = s.h;
      }
      if (io.h_out) io.h_out[o] = s.h;
    }
  }
}

mpchost::LdsLimit g_cell_limit(cell_kernel);
}  // namespace

struct mpc_recurrent {
  int memories = 0, device = -1;
  recurrent::Cell cell[recurrent::kMemories]{};
  size_t lds = 0;                      // the wider memory's
  bool bound = false;
};

extern "C" {

const char *mpc_recurrent_last_error(void) { return g_err.c_str(); }

void mpc_recurrent_destroy(mpc_recurrent *h) { delete h; }      // owns no device memory: parameters and state are the caller's

int mpc_recurrent_create(mpc_recurrent **out, int memories, const int *input_sizes, const int *hidden_sizes) {
  if (!out || !input_sizes || !hidden_sizes) return fail(MPC_E_ARG, "mpc_recurrent_create: null argument");
  if (memories < 1 || memories > recurrent::kMemories) return fail(MPC_E_ARG, "mpc_recurrent_create: one or two memories");
  size_t lds = 0;
  for (int k = 0; k < memories; ++k) {
    const int I = input_sizes[k], H = hidden_sizes[k];
    const std::string mem = "mpc_recurrent_create: memory " + std::to_string(k) + ": ";
    const std::string why = recurrent::size_refusal(I, H);
    if (!why.empty()) return fail(MPC_E_ARG, mem + why);
    const size_t b = recurrent::lds_bytes(I, H);
    if (b > (size_t)MPC_RECURRENT_MAX_LDS)
      return fail(MPC_E_ARG, mem + "16 rows of " + std::to_string(I) + " + " + std::to_string(H) + " floats need " + std::to_string(b) +
                                 " bytes of LDS, more than one CU's 160 KB");
    lds = b > lds ? b : lds;
  }
  mpc_recurrent *h = new mpc_recurrent();
  h->memories = memories;
  h->lds = lds;
  for (int k = 0; k < memories; ++k) {
    h->cell[k].I = input_sizes[k];
    h->cell[k].H = hidden_sizes[k];
  }
  *out = h;
  return MPC_OK;
}

int mpc_recurrent_bind(mpc_recurrent *h, const float *const *d_w_ih, const float *const *d_w_hh, const float *const *d_b_ih, const float *const *d_b_hh) {
  if (!h) return fail(MPC_E_ARG, "mpc_recurrent_bind: null argument");
  const recurrent::Parameters params{d_w_ih, d_w_hh, d_b_ih, d_b_hh};
  const std::string why = recurrent::bind_refusal(params, h->memories);
  if (!why.empty()) return fail(MPC_E_ARG, "mpc_recurrent_bind: " + why);
  const int dev = mpchost::current_device();
  if (dev < 0) return fail(MPC_E_NODEVICE, "mpc_recurrent_bind: no HIP device");
  if (g_cell_limit.raise(dev, h->lds) != hipSuccess) return fail(MPC_E_HIP, "mpc_recurrent_bind: device set-up failed");
  recurrent::bind(h->cell, params, h->memories);
  h->device = dev;
  h->bound = true;
  return MPC_OK;
}

int mpc_recurrent_step(mpc_recurrent *h, int n, int first, int count, const mpc_recurrent_io *io, const long long *d_reset, int commit, void *stream) {
  if (!h || !io) return fail(MPC_E_ARG, "mpc_recurrent_step: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_recurrent_step: n must be at least 1");
  if (first < 0 || count < 1 || first + count > h->memories)
    return fail(MPC_E_ARG, "mpc_recurrent_step: memories " + std::to_string(first) + " .. " + std::to_string(first + count - 1) + " of a handle with " +
                               std::to_string(h->memories));
  if (reinterpret_cast<uintptr_t>(d_reset) & 7u) return fail(MPC_E_ARG, "mpc_recurrent_step: d_reset must be 8-byte aligned");
  recurrent::Launch a{};
  for (int k = 0; k < h->memories; ++k) a.cell[k] = h->cell[k];
  for (int k = 0; k < count; ++k) {
    const mpc_recurrent_io &m = io[k];
    const std::string who = "mpc_recurrent_step: memory " + std::to_string(first + k) + ": ";
    if (!m.d_x || !m.d_h || !m.d_c) return fail(MPC_E_ARG, who + "d_x, d_h or d_c is null");
    if (!aligned16(m.d_x) || !aligned16(m.d_h) || !aligned16(m.d_c) || !aligned16(m.d_h_saved) || !aligned16(m.d_c_saved) || !aligned16(m.d_h_out))
      return fail(MPC_E_ARG, who + "every pointer must be 16-byte aligned");
    if (m.d_h == m.d_c || m.d_h_out == m.d_h || m.d_h_out == m.d_c || m.d_h_saved == m.d_h || m.d_c_saved == m.d_c ||
        (m.d_h_out && (m.d_h_out == m.d_h_saved || m.d_h_out == m.d_c_saved)) || (m.d_h_saved && m.d_h_saved == m.d_c_saved))
      return fail(MPC_E_ARG, who + "the arrays must not overlap");
    a.io[first + k] = recurrent::Io{m.d_x, m.d_h, m.d_c, m.d_h_saved, m.d_c_saved, m.d_h_out};
  }
  if (!h->bound) return fail(MPC_E_ARG, "mpc_recurrent_step: no parameters bound (mpc_recurrent_bind)");
  DeviceGuard guard_(h->device);
  const dim3 grid((unsigned)((n + recurrent::kRows - 1) / recurrent::kRows), (unsigned)count);
  hipLaunchKernelGGL(cell_kernel, grid, dim3(recurrent::kThreads), h->lds, reinterpret_cast<hipStream_t>(stream), a, first, n, d_reset, commit != 0 ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
