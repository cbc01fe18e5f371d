// recurrent_cell.h -- one LSTM step (one layer, torch's nn.LSTM parameter layout) for N environments: the memory in front of the actor's and
// the critic's MLP (rsl_rl v1.0.2's Memory in its stepping mode), float32 throughout.
//   gates = x W_ih^T + b_ih + h W_hh^T + b_hh        W_ih [4H][I], W_hh [4H][H], rows in torch's order i, f, g, o
//   i, f, o = sigmoid, g = tanh;   c' = f c + i g;   h' = o tanh(c')
//
// The shape is policy_mlp.h's: a workgroup carries 16 environments, their x and h rows are staged in LDS (padded as there), the weights stream
// from L2 as 16-byte loads and the products run on v_mfma_f32_16x16x4_f32.  Rows of the MFMA tile are environments, columns are state elements.
// A wave takes one block of 16 state columns j and with it the FOUR gate blocks of those columns -- rows g H + j of the weight matrices: four
// independent accumulation chains fed by one read of the activations, policy::blocks<4>'s shape -- and runs the K loop first over I against
// W_ih, then over H against W_hh, into the same accumulators.  The four gates of a state element then sit in the same lane and register: biases,
// sigmoid, tanh, c' and h' are computed in registers, and the gate pre-activations never reach LDS or HBM.  c is read from global memory, one
// element per lane, in the epilogue; the stores follow it.
//
// The state is updated in place.  A workgroup reads the state rows of its own 16 environments only: it stages h (with the reset applied) in
// LDS, and a barrier stands between that staging and the first store; a lane reads and writes one and the same element of c.
//
// LDS: 16 (I + H + 2 kPad) floats -- 33 280 bytes at I = H = 256.  cell_kernel itself is mpc_recurrent.hip's; what it shares with
// bptt::seq_forward_kernel and recurrent_policy::step_kernel -- accumulate, stage, finish -- is here; the host's share is recurrent_host.h.
#pragma once
#include <hip/hip_runtime.h>

namespace recurrent {

constexpr int kRows = 16;            // environments per workgroup (MFMA M)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPad = 4;              // floats of row padding in LDS, as in policy_mlp.h
constexpr int kGates = 4;            // i, f, g, o
constexpr int kMemories = 2;         // actor's, critic's

struct Cell {
  int I, H;
  const float *w_ih, *w_hh;          // [4H][I], [4H][H] row-major (nn.LSTM.weight_ih_l0 / weight_hh_l0)
  const float *b_ih, *b_hh;          // [4H]
};

struct Io {
  const float *x;                    // [n][I]
  float *h, *c;                      // [n][H] the persistent state: read, then (commit) overwritten
  float *h_saved, *c_saved;          // [n][H] or null: the state the step started from, after the reset's zeroing
  float *h_out;                      // [n][H] or null: h'
};

struct Launch {
  Cell cell[kMemories];
  Io io[kMemories];
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline size_t lds_bytes(int I, int H) { return sizeof(float) * kRows * ((size_t)I + kPad + (size_t)H + kPad); }

__device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// acc[g] += in[16][K] (W rows g H + n)^T for the four gates g of state column n = 16 nb + (lane & 15).  K % 16 == 0.  The operand maps are
// policy::blocks': A row = lane & 15, k = 4 (lane >> 4) + i in MFMA i of a chunk of 16; B column = lane & 15, the same k.
__device__ __forceinline__ void accumulate(f32x4 (&acc)[kGates], const float *in, int in_stride, const float *__restrict__ W, int K, int H, int nb) {
  const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  const float *wr[kGates];
  float4 wn[kGates];
#pragma unroll
  for (int g = 0; g < kGates; ++g) {
    wr[g] = W + (size_t)(g * H + nb * 16 + col) * K + 4 * q;
    wn[g] = *reinterpret_cast<const float4 *>(wr[g]);
  }
  const float *ar = in + col * in_stride + 4 * q;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const float4 a4 = *reinterpret_cast<const float4 *>(ar + k0);
    float4 w4[kGates];
#pragma unroll
    for (int g = 0; g < kGates; ++g) {
      w4[g] = wn[g];
      if (k0 + 16 < K) wn[g] = *reinterpret_cast<const float4 *>(wr[g] + k0 + 16);      // the next trip's weights
    }
#pragma unroll
    for (int g = 0; g < kGates; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, w4[g].x, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < kGates; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, w4[g].y, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < kGates; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, w4[g].z, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < kGates; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, w4[g].w, acc[g], 0, 0, 0);
  }
}

// rows [16][width] of a row-major matrix [n][width] into LDS, 16 bytes per lane and trip; rows past n, and rows whose flag is set, as zeros.
// `copy` (may be null): the staged rows < n are written there as well, at the same place.  width % 4 == 0.  THREADS: the workgroup's.
template <int THREADS>
__device__ __forceinline__ void stage(float *dst, int stride, const float *__restrict__ src, float *copy, int width, int r0, int n,
                                      const long long *__restrict__ reset) {
  const int quads = width >> 2;
  for (int e = threadIdx.x; e < kRows * quads; e += THREADS) {
    const int r = e / quads, k = 4 * (e - r * quads), row = r0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n) {
      const size_t o = (size_t)row * width + k;
      if (!(reset && reset[row] != 0)) v = *reinterpret_cast<const float4 *>(src + o);
      if (copy) *reinterpret_cast<float4 *>(copy + o) = v;
    }
    *reinterpret_cast<float4 *>(dst + r * stride + k) = v;
  }
}

// The cell once the four gate accumulators are there, for register reg of the tile (C layout of the 16x16 MFMA: col = lane & 15,
// row = 4 (lane >> 4) + reg) and the element c0 of the state it starts from.  c' = f c + i g is torch's: a product, a product, a sum -- every
// unit that includes this is compiled without contraction.  cell_kernel, bptt::seq_forward_kernel and recurrent_policy::step_kernel finish
// their steps here and nowhere else, which is what makes them agree bit for bit; each keeps its own stores, rows past n and resets.
struct Step { float i, f, g, o, c, h; };      // the gate activations, c', h'
__device__ __forceinline__ Step finish(const f32x4 (&acc)[kGates], const float (&bias)[kGates], int reg, float c0) {
  const float ig = sigmoid(acc[0][reg] + bias[0]), fg = sigmoid(acc[1][reg] + bias[1]);
  const float gg = tanhf(acc[2][reg] + bias[2]), og = sigmoid(acc[3][reg] + bias[3]);
  const float c1 = fg * c0 + ig * gg;
  return Step{ig, fg, gg, og, c1, og * tanhf(c1)};
}

}  // namespace recurrent
