// recurrent_policy.h -- one tick of a deployed recurrent weight policy for N robots in ONE launch: the actor's memory (recurrent_cell.h's LSTM
// step), the actor's MLP on h' (policy_mlp.h's layers), clamp to [-1, 1] and the affine map to MPC weights.
//   gates = x W_ih^T + b_ih + h W_hh^T + b_hh;   i, f, o = sigmoid, g = tanh;   c' = f c + i g;   h' = o tanh(c')
//   a = actor(h');   weights = clamp(a, -1, 1) * scale + shift
//
// The shape is the one recurrent_cell.h and policy_mlp.h share: a workgroup carries 16 robots, activations stay in LDS (rows padded by kPad),
// the weights stream from L2 as 16-byte loads, the products run on v_mfma_f32_16x16x4_f32.  policy::layer strides by policy::kThreads, so the
// workgroup is that wide (8 waves at the default 512); recurrent::accumulate and recurrent::finish are per wave and recurrent::stage takes the
// workgroup's thread count, so all three are used as they stand.
//
// Phases of a workgroup:
//   1. x [16][I] and h [16][H] into LDS, 16 bytes per lane and trip; rows past n as zeros, and h as zeros where the row's reset flag is set (x is
//      the robot's fresh observation: a reset clears the memory, never the row it reads -- cell_kernel's rule).  Barrier: every read of this
//      workgroup's rows of h lies before it, every store to them after it.
//   2. the cell: wave w takes the state-column blocks nb = w, w + kWaves, ... with their four gate blocks, K over I against W_ih and then over H
//      against W_hh into the same four accumulators; biases, sigmoid, tanh, c' and h' in registers: recurrent::finish, cell_kernel's
//      epilogue.  c is read from global memory, one element per lane (zero on a flagged row).  c' and h' go to the state in place (rows < n), h'
//      goes into the LDS buffer the MLP's first layer reads (rows past n: zeros, as mlp_kernel stages them).  The gate pre-activations never
//      reach LDS or HBM, and h' reaches HBM as the state only.  Barrier.
//   3. policy::layer over the actor's layers, ping-ponging two LDS buffers as mlp_kernel does, a barrier after each.
//   4. mlp_kernel's epilogue: the raw actions (optional) and the weights.
// Every output element is summed in the order cell_kernel and mlp_kernel sum it, so the launch equals their composition bit for bit.
//
// LDS: four regions that do NOT alias -- x [16][I + kPad], h [16][H + kPad], and the MLP's two buffers as policy::lds_bytes sizes them (buffer 0
// holds dims[0] = H, dims[2], ...; buffer 1 dims[1], dims[3], ...).  The cell writes h' into buffer 0 while other waves still read the staged h,
// so those two must be distinct; keeping x apart as well costs 16 (I + kPad) floats and saves a barrier.  At I = 48, H = 256 and the actor
// 256-512-256-128-12: 16 (52 + 260 + 260 + 516) floats = 69 632 bytes.
// No atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "policy_mlp.h"
#include "recurrent_cell.h"

namespace recurrent_policy {

constexpr int kRows = policy::kRows;
constexpr int kThreads = policy::kThreads;      // policy::layer's stride
constexpr int kWaves = kThreads / 64;
constexpr int kPad = policy::kPad;
static_assert(recurrent::kRows == policy::kRows && recurrent::kPad == policy::kPad, "recurrent_cell.h and policy_mlp.h share one tile");

struct Launch {
  recurrent::Cell cell;              // the actor's memory
  policy::Net net;                   // the actor's layers; dims[0] == cell.H
};

inline size_t lds_bytes(int I, int H, const policy::Net &net) { return recurrent::lds_bytes(I, H) + policy::lds_bytes(net); }

// grid ceil(n / 16).  x [n][I]; h, c [n][H] the state, updated in place; reset [n] int64 or null; actions [n][dims[L]] or null; weights [n][dims[L]].
__global__ __launch_bounds__(kThreads) void step_kernel(Launch a, int n, const float *__restrict__ x, float *h, float *c, const long long *__restrict__ reset,
                                                       float *__restrict__ actions, float *__restrict__ weights) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const recurrent::Cell &m = a.cell;
  const policy::Net &net = a.net;
  const int I = m.I, H = m.H, xs = I + kPad, hs = H + kPad;
  int wmax_even = 0, wmax_odd = 0;   // widest activation held by the MLP's buffer 0 (layers 0, 2, ...) / buffer 1
  for (int l = 0; l <= net.n_layers; ++l) {
    int &w = (l & 1) ? wmax_odd : wmax_even;
    w = net.dims[l] > w ? net.dims[l] : w;
  }
  float *xb = lds, *hb = xb + kRows * xs;
  float *buf[2] = {hb + kRows * hs, hb + kRows * hs + kRows * (wmax_even + kPad)};
  const int stride[2] = {wmax_even + kPad, wmax_odd + kPad};
  const int r0 = blockIdx.x * kRows;
  recurrent::stage<kThreads>(xb, xs, x, nullptr, I, r0, n, nullptr);
  recurrent::stage<kThreads>(hb, hs, h, nullptr, H, r0, n, reset);
  __syncthreads();                     // every read of this workgroup's rows of h lies before it, every store to them after it
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  for (int nb = wave; nb * 16 < H; nb += kWaves) {
    recurrent::f32x4 acc[recurrent::kGates];
#pragma unroll
    for (int g = 0; g < recurrent::kGates; ++g) acc[g] = recurrent::f32x4{0.f, 0.f, 0.f, 0.f};
    recurrent::accumulate(acc, xb, xs, m.w_ih, I, H, nb);
    recurrent::accumulate(acc, hb, hs, m.w_hh, H, H, nb);
    const int j = nb * 16 + col;
    float bias[recurrent::kGates];
#pragma unroll
    for (int g = 0; g < recurrent::kGates; ++g) bias[g] = m.b_ih[g * H + j] + m.b_hh[g * H + j];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {  // C layout of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg
      const int row = r0 + 4 * q + reg;
      float h1 = 0.f;
      if (row < n) {
        const size_t o = (size_t)row * H + j;
        const float c0 = (reset && reset[row] != 0) ? 0.f : c[o];
        const recurrent::Step s = recurrent::finish(acc, bias, reg, c0);
        h1 = s.h;
        c[o] = s.c;
        h[o] = s.h;
      }
      buf[0][(4 * q + reg) * stride[0] + j] = h1;
    }
  }
  __syncthreads();
  for (int l = 0; l < net.n_layers; ++l) {
    policy::layer(buf[l & 1], stride[l & 1], buf[(l + 1) & 1], stride[(l + 1) & 1], net.w[l], net.b[l], net.dims[l], net.dims[l + 1], l + 1 < net.n_layers);
    __syncthreads();
  }
  const int L = net.n_layers, dl = net.dims[L];
  const float *res = buf[L & 1];
  for (int e = threadIdx.x; e < kRows * dl; e += kThreads) {
    const int r = e / dl, k = e - r * dl;
    if (r0 + r >= n) continue;
    const float v = res[r * stride[L & 1] + k];
    if (actions) actions[(size_t)(r0 + r) * dl + k] = v;
    const float cl = fminf(fmaxf(v, -1.f), 1.f);         // torch.clamp(current_action, -1, 1), as mlp_kernel
    weights[(size_t)(r0 + r) * dl + k] = cl * net.scale[k] + net.shift[k];
  }
}

}  // namespace recurrent_policy
