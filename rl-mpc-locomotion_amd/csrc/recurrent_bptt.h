// recurrent_bptt.h -- the recurrent actor-critic's update through time: recurrent_cell.h's LSTM step rolled over the T slots of a rollout for a block
// of B environments, forward and backward, float32 throughout.  The recurrence is per environment, so a workgroup that owns 16 environments runs all T
// steps of its rows in ONE launch with no dependence on another workgroup: no per-step launches, no grid synchronisation.  No padding either: the state
// is zeroed before step t where reset[t][e] is set, which is what the padded trajectories of a block of environments are.
//
//   seq_forward_kernel   grid (ceil(B / 16), memories), t = 0 .. T-1.  h stays in LDS between the steps (two buffers: step t reads one and writes
//                        h' -- zeroed where reset[t+1] is set -- into the other, so ONE barrier per step stands between every read of a buffer and
//                        the next write to it); c stays in registers, one element per lane, the same lane every step.  A step is cell_kernel's:
//                        recurrent::accumulate over I against W_ih, then over H against W_hh, into the four gate accumulators, then cell_kernel's
//                        epilogue, recurrent::finish -- y[t] equals T launches of cell_kernel bit for bit.  Per step it keeps what the backward
//                        pass reads: the gate activations i, f, g, o, c', and the state the step started from (h_used, c_used).  x[t+1] is staged
//                        into the other x buffer after step t's products.
//   transpose_kernel     W_hh [4H][H] -> W_hh^T [H rounded up to 64][4H], once per backward call (the weights change after every optimiser step).
//                        The backward step's product dG[t] W_hh reads W_hh along its OUTPUT index; from the transposed copy they are the same 16-byte
//                        loads along the reduction that accumulate issues forward, and the copy (1 MB at H = 256) stays in the XCD's 4 MB L2 for
//                        all T steps of all workgroups.  Read in place, a lane's four k-consecutive values would be four 4-byte loads H floats apart.
//   seq_backward_kernel  the same grid, t = T-1 .. 0.  A step computes dG[t] (16 x 4H) element-wise from the kept activations, writes it to LDS and to
//                        the workspace, and after a barrier forms dh_rec = dG[t] W_hh as accumulate over K = 4H against W_hh^T: a wave takes FOUR
//                        CONSECUTIVE blocks of 16 state columns (accumulate's four chains, "H" = 16) and owns the same columns in the element-wise
//                        part, so dh_rec and dc_rec stay in registers.  Both are zeroed on rows where reset[t] is set: nothing reaches step t - 1.
//   weight gradients     dW_ih = dG^T X, dW_hh = dG^T h_used over all T B rows: pgemm::gemm_kernel's backward-weight kind (chunk partials,
//                        reduce_kernel in index order), launched by the unit through mpc_ppo_gemm.hip.  X is read in place from the rollout storage through an index: row
//                        (t, b) starts (t stride + b I) / 4 quads after the block's first row, so with ldb = 4 the index is exact for any slot stride
//                        that is a multiple of 4 floats.
//   column_sum_kernel    db = the column sums of dG: per chunk of 256 rows a float64 sum in row order, rounded once; reduce_kernel adds the chunks.
//                        (gemm_kernel's own dbias adds a chunk's rows one by one in float32: measured against torch's float32 autograd that chain
//                        alone put db at 5.2 x torch's own distance from float64 on a 64-element tensor over 165 rows, where the rule allows 4.)
// No atomics; every sum is in a fixed order, so a rerun is bit-identical.  All LDS is dynamic:
//   forward   2 x 16 (I + H + 2 kPad) floats -- 66 560 bytes at I = H = 256
//   backward  16 (4 H + kPad) floats         -- 65 792 bytes at H = 256
#pragma once
#include <hip/hip_runtime.h>

#include "ppo_gemm_plan.h"
#include "recurrent_cell.h"

namespace bptt {

using recurrent::f32x4;
using recurrent::kGates;
using recurrent::kMemories;
using recurrent::kPad;
using recurrent::kRows;
using recurrent::kThreads;
using recurrent::kWaves;

constexpr int kMaxSlots = 10;          // forward: blocks of 16 state columns per wave -- H <= 640 (the backward pass's LDS stops at H = 624)
constexpr int kMaxQuads = 3;           // backward: quads of such blocks per wave -- H <= 768
constexpr int kSumRows = 256;          // rows per chunk of the column sums (pgemm::kMinChunk: as many partials as the GEMMs' workspace holds)
constexpr int kQuadCols = 64;          // W_hh^T's rows are padded (zeros) to a multiple of this: a quad reads whole

struct Seq {                           // what one memory reads and writes in a call
  const float *x;                      // row (t, b) at x + t x_stride + b I
  long long x_stride;                  // floats between two slots
  const float *h0, *c0;                // [B][H]
  float *y;                            // [T][B][H]: h'
  float *c_last;                       // [B][H] or null: c' of step T - 1
  const float *dy;                     // backward: [T][B][H]
};

struct Work {                          // one memory's workspace, rows (t, b) at t B + b
  float *gates;                        // [T B][4H] the activations i, f, g, o
  float *c_new;                        // [T B][H]  c'
  float *h_used, *c_used;              // [T B][H]  the state the step started from, after the reset's zeroing
  float *dG;                           // [T B][4H]
  float *w_hh_t;                       // [H rounded up to 64][4H]
  long long *x_index;                  // [T B]     (t x_stride + b I) / 4
  float *db_part;                      // [chunks of kSumRows rows][4H] column sums of dG
};

struct Launch {
  recurrent::Cell cell[kMemories];
  Seq seq[kMemories];
  Work work[kMemories];
};

inline size_t forward_lds_bytes(int I, int H) { return 2 * recurrent::lds_bytes(I, H); }
inline size_t backward_lds_bytes(int H) { return sizeof(float) * kRows * (4 * (size_t)H + kPad); }
inline int padded_cols(int H) { return (H + kQuadCols - 1) / kQuadCols * kQuadCols; }

// grid (ceil(B / 16), memories); memory = first + blockIdx.y.  reset [T][B] int64 or null; flags [T B] receives reset != 0 for the backward pass.
__global__ __launch_bounds__(kThreads) void seq_forward_kernel(Launch a, int first, int T, int B, const long long *__restrict__ reset, int *__restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int which = first + (int)blockIdx.y;
  const recurrent::Cell &m = a.cell[which];
  const Seq &s = a.seq[which];
  const Work &w = a.work[which];
  const int I = m.I, H = m.H, xs = I + kPad, hs = H + kPad;
  float *xb = lds, *hb = lds + 2 * kRows * xs;      // two buffers each: step t uses number t & 1
  const int r0 = blockIdx.x * kRows;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;

  for (int e = threadIdx.x; e < T * kRows; e += kThreads) {      // what the backward pass and the weight-gradient GEMM read per row
    const int t = e / kRows, row = r0 + (e - t * kRows);
    if (row >= B) continue;
    const size_t r = (size_t)t * B + row;
    w.x_index[r] = ((long long)t * s.x_stride + (long long)row * I) >> 2;
    if (blockIdx.y == 0) flags[r] = (reset && reset[r] != 0) ? 1 : 0;
  }
  recurrent::stage<kThreads>(xb, xs, s.x, nullptr, I, r0, B, nullptr);
  recurrent::stage<kThreads>(hb, hs, s.h0, w.h_used, H, r0, B, reset);      // h_used[0]: h0 with reset[0] applied
  float c[kMaxSlots][4];
#pragma unroll
  for (int sl = 0; sl < kMaxSlots; ++sl) {
    const int j = (wave + kWaves * sl) * 16 + col;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = r0 + 4 * q + reg;
      c[sl][reg] = (j < H && row < B && !(reset && reset[row] != 0)) ? s.c0[(size_t)row * H + j] : 0.f;
    }
  }

  for (int t = 0; t < T; ++t) {
    __syncthreads();                   // x[t] and h are staged; every read of the buffers step t writes lies before it
    const float *xc = xb + (t & 1) * kRows * xs, *hc = hb + (t & 1) * kRows * hs;
    float *hn = hb + ((t + 1) & 1) * kRows * hs;
    const long long *rn = (reset && t + 1 < T) ? reset + (size_t)(t + 1) * B : nullptr;
#pragma unroll
    for (int sl = 0; sl < kMaxSlots; ++sl) {
      int nb = wave + kWaves * sl;
      asm volatile("" : "+s"(nb));     // opaque per step: the ten slots' weight addresses and first loads are formed here, not hoisted out of the t loop (spills)
      if (nb * 16 < H) {
        f32x4 acc[kGates];
#pragma unroll
        for (int g = 0; g < kGates; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        recurrent::accumulate(acc, xc, xs, m.w_ih, I, H, nb);
        recurrent::accumulate(acc, hc, hs, m.w_hh, H, H, nb);
        const int j = nb * 16 + col;
        float bias[kGates];
#pragma unroll
        for (int g = 0; g < kGates; ++g) bias[g] = m.b_ih[g * H + j] + m.b_hh[g * H + j];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {  // C layout of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg
          const int lr = 4 * q + reg, row = r0 + lr;
          const float c0 = c[sl][reg];
          const recurrent::Step st = recurrent::finish(acc, bias, reg, c0);
          const float ig = st.i, fg = st.f, gg = st.g, og = st.o, c1 = st.c, h1 = st.h;
          const bool live = row < B;
          const bool cut = live && rn && rn[row] != 0;      // the next step starts this row from zero
          const float hnext = (live && !cut) ? h1 : 0.f;
          hn[lr * hs + j] = hnext;                           // (rows past B as zeros, as stage leaves them)
          c[sl][reg] = cut ? 0.f : c1;
          if (!live) continue;
          const size_t r = (size_t)t * B + row, o = r * H + j, o4 = r * 4 * H + j;
          w.gates[o4] = ig;
          w.gates[o4 + H] = fg;
          w.gates[o4 + 2 * H] = gg;
          w.gates[o4 + 3 * H] = og;
          w.c_new[o] = c1;
          w.c_used[o] = c0;
          s.y[o] = h1;
          if (t + 1 < T) w.h_used[o + (size_t)B * H] = hnext;
          else if (s.c_last) s.c_last[(size_t)row * H + j] = c1;
        }
      }
    }
    if (t + 1 < T) recurrent::stage<kThreads>(xb + ((t + 1) & 1) * kRows * xs, xs, s.x + (size_t)(t + 1) * s.x_stride, nullptr, I, r0, B, nullptr);
  }
}

// grid (ceil(4 H H / 256), memories): out [padded_cols(H)][4H], rows past H stay as the unit zeroed them
__global__ __launch_bounds__(kThreads) void transpose_kernel(Launch a, int first) {
  const int which = first + (int)blockIdx.y;
  const int H = a.cell[which].H, K = 4 * H;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= K * H) return;
  const int j = e / K, k = e - j * K;
  a.work[which].w_hh_t[e] = a.cell[which].w_hh[(size_t)k * H + j];
}

// grid (ceil(4 H / 256), ceil(R / kSumRows), memories): db_part[chunk][col] = the sum of dG[r][col] over the chunk's rows r < R, float64, in row order
__global__ __launch_bounds__(kThreads) void column_sum_kernel(Launch a, int first, int R) {
  const int which = first + (int)blockIdx.z;
  const Work &w = a.work[which];
  const int G = 4 * a.cell[which].H, colm = blockIdx.x * kThreads + threadIdx.x;
  if (colm >= G) return;
  const int r_begin = blockIdx.y * kSumRows, r_end = r_begin + kSumRows < R ? r_begin + kSumRows : R;
  double sum = 0.0;
  for (int r = r_begin; r < r_end; ++r) sum += (double)w.dG[(size_t)r * G + colm];
  w.db_part[(size_t)blockIdx.y * G + colm] = (float)sum;
}

// grid (ceil(B / 16), memories); consumes what seq_forward_kernel left in the workspace for the same T, B and memories
__global__ __launch_bounds__(kThreads) void seq_backward_kernel(Launch a, int first, int T, int B, const int *__restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int which = first + (int)blockIdx.y;
  const Seq &s = a.seq[which];
  const Work &w = a.work[which];
  const int H = a.cell[which].H, G = 4 * H, gs = G + kPad;
  const int r0 = blockIdx.x * kRows;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  float dc_rec[kMaxQuads][kGates][4];
  f32x4 dh_rec[kMaxQuads][kGates];
#pragma unroll
  for (int sl = 0; sl < kMaxQuads; ++sl)
#pragma unroll
    for (int b = 0; b < kGates; ++b) {
      dh_rec[sl][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) dc_rec[sl][b][reg] = 0.f;
    }

  for (int t = T - 1; t >= 0; --t) {
#pragma unroll
    for (int sl = 0; sl < kMaxQuads; ++sl) {
      int nq = wave + kWaves * sl;
      asm volatile("" : "+s"(nq));     // opaque per step, as in the forward kernel: the slots' addresses are formed here, not kept across the t loop
#pragma unroll
      for (int b = 0; b < kGates; ++b) {                     // the quad's four column blocks
        const int j = (nq * kGates + b) * 16 + col;
        if (j - col < H) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int lr = 4 * q + reg, row = r0 + lr;
            float di = 0.f, df = 0.f, dg = 0.f, dout = 0.f;
            if (row < B) {
              const size_t r = (size_t)t * B + row, o = r * H + j, o4 = r * G + j;
              const float ig = w.gates[o4], fg = w.gates[o4 + H], gg = w.gates[o4 + 2 * H], og = w.gates[o4 + 3 * H];
              const float dh = s.dy[o] + dh_rec[sl][b][reg];
              const float tc = tanhf(w.c_new[o]);
              // the derivatives s(1-s) = s - s s and 1 - th^2, and the sum into dc, as written fused multiply-adds: one rounding each
              dout = dh * tc * fmaf(-og, og, og);
              const float dc = fmaf(dh * og, fmaf(-tc, tc, 1.0f), dc_rec[sl][b][reg]);
              di = dc * gg * fmaf(-ig, ig, ig);
              df = dc * w.c_used[o] * fmaf(-fg, fg, fg);
              dg = dc * ig * fmaf(-gg, gg, 1.0f);
              dc_rec[sl][b][reg] = flags[r] ? 0.f : dc * fg;
              w.dG[o4] = di;
              w.dG[o4 + H] = df;
              w.dG[o4 + 2 * H] = dg;
              w.dG[o4 + 3 * H] = dout;
            }
            float *d = lds + lr * gs + j;
            d[0] = di;
            d[H] = df;
            d[2 * H] = dg;
            d[3 * H] = dout;
          }
        }
      }
    }
    __syncthreads();                   // dG[t] is whole
    if (t > 0) {
#pragma unroll
      for (int sl = 0; sl < kMaxQuads; ++sl) {
        int nq = wave + kWaves * sl;
        asm volatile("" : "+s"(nq));
        if (nq * kQuadCols < H) {
          f32x4 acc[kGates];
#pragma unroll
          for (int b = 0; b < kGates; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
          recurrent::accumulate(acc, lds, gs, w.w_hh_t, G, 16, kGates * nq);      // "gate" b = column block 4 nq + b: rows 16 b + 64 nq + col of W_hh^T
#pragma unroll
          for (int b = 0; b < kGates; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int row = r0 + 4 * q + reg;
              dh_rec[sl][b][reg] = (row < B && !flags[(size_t)t * B + row]) ? acc[b][reg] : 0.f;
            }
        }
      }
    }
    __syncthreads();                   // every read of dG[t] lies before the next step's writes
  }
}

}  // namespace bptt
