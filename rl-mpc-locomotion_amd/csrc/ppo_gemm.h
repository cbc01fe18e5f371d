// ppo_gemm.h -- the three GEMMs of a Linear / ELU stack's forward and backward pass on the exact-fp32 MFMA pipe (v_mfma_f32_32x32x2_f32: a k-ordered
// fp32 fma chain per output element, so a result differs from a CPU sgemm only by the summation order), one LDS-tiled kernel template:
//   forward          Y  = ELU(X W^T + b)        X [rows][K] (layer 0: rows read through the mini-batch index), W [N][K]; Y is all the backward pass needs
//   backward data    dX = (dY W) * ELU'(X)      ELU' from the stored activation: 1 for y > 0, y + 1 otherwise
//   ... linear       dX = dY W                  the same loaders and products, no factor: the gradient of rows no activation produced (the outputs of the
//                                               memories in front of a recurrent actor-critic's first layers)
//   backward weight  dW = dY^T X                split over the rows into chunks of at most kChunk: chunk c writes its own [N][K] partial (and the column
//                                               sums of its dY rows) to a workspace; reduce_kernel adds the chunks in index order.  No atomics.
// A workgroup is 4 waves in a 2 x 2 arrangement, each wave owns TM x TN tiles of 32 x 32 (TM x TN independent accumulator chains), so the block tile is
// 64 TM x 64 TN; the reduction advances 32 at a time.  Both operands sit in LDS reduction-major ([32][tile + pad]): lane l of an MFMA reads
// A[i = l & 31][k = l >> 5], which is then one word per lane on consecutive addresses.  An operand whose reduction index is contiguous in memory
// (X and W forward, dY backward data) is read as 16-byte loads along it and transposed on the LDS write; one whose tile index is contiguous (W backward
// data, dY and X backward weight) is copied as 16-byte rows.  The next tile's global loads are issued before the current tile's products.  The fp32 MFMA
// runs at 1/16 of the bf16 rate, so a 128 x 128 x 32 tile is 4096 cycles of matrix pipe per SIMD against 32 KB of loads, and two or three workgroups per CU
// cover each other's barriers.  Measured on the 24 576-row mini-batch: 42 .. 56 TF per kind, 79 TF for the largest forward layer.
// Two problems (actor, critic) travel in one launch: blockIdx.y picks the problem, a workgroup past its problem's tiles leaves.
// Every bound is checked: rows, columns and reduction may be any count >= 1; leading dimensions are multiples of 4 floats (16-byte loads).
#pragma once
#include <hip/hip_runtime.h>

#include "ppo_gemm_plan.h"      // Kind, kChunk, kMinChunk, the launch plan and the structs a caller fills (no HIP in it)

namespace pgemm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kBK = 32;                // reduction rows per LDS tile
constexpr int kKQ = kBK / 4;          // 16-byte loads along one row of a reduction-contiguous tile
constexpr int kPad = 4;
// kChunk (most rows per backward-weight chunk: the longest fp32 chain) and kMinChunk (fewest: what sizes the workspace) are ppo_gemm_plan.h's

__device__ __forceinline__ float4 mask4(float4 v, int left) {   // keep the first `left` components
  if (left < 4) { v.w = 0.f; if (left < 3) v.z = 0.f; if (left < 2) v.y = 0.f; if (left < 1) v.x = 0.f; }
  return v;
}

__device__ __forceinline__ long long row_of(const long long *idx, long long limit, int row) {
  if (!idx) return row;
  long long r = idx[row];
  return r < 0 ? 0 : (r >= limit ? limit - 1 : r);
}

// tile rows r0 .. r0 + BT (valid below R) of a matrix whose reduction index is contiguous: 16 bytes along k per lane
template <int BT>
__device__ __forceinline__ void fetch_kcontig(float4 (&reg)[BT / 32], const float *__restrict__ src, int ld, const long long *idx, long long limit, int r0,
                                              int R, int k0, int k_end) {
  const int r = threadIdx.x / kKQ, k = k0 + 4 * (threadIdx.x % kKQ);
#pragma unroll
  for (int i = 0; i < BT / 32; ++i) {
    const int row = r0 + r + 32 * i;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < R && k < k_end) v = mask4(*reinterpret_cast<const float4 *>(src + (size_t)row_of(idx, limit, row) * ld + k), k_end - k);
    reg[i] = v;
  }
}
template <int BT>
__device__ __forceinline__ void store_kcontig(const float4 (&reg)[BT / 32], float *dst) {
  constexpr int LD = BT + kPad;
  const int r = threadIdx.x / kKQ, kq = 4 * (threadIdx.x % kKQ);
#pragma unroll
  for (int i = 0; i < BT / 32; ++i) {
    float *d = dst + kq * LD + r + 32 * i;
    d[0] = reg[i].x; d[LD] = reg[i].y; d[2 * LD] = reg[i].z; d[3 * LD] = reg[i].w;
  }
}

// reduction rows k0 .. k0 + 32 (valid below k_end) of a matrix whose tile index is contiguous: columns c0 .. c0 + BT (valid below Cn)
template <int BT>
__device__ __forceinline__ void fetch_mcontig(float4 (&reg)[BT / 32], const float *__restrict__ src, int ld, const long long *idx, long long limit, int c0,
                                              int Cn, int k0, int k_end) {
  constexpr int C4 = BT / 4;
#pragma unroll
  for (int i = 0; i < BT / 32; ++i) {
    const int e = threadIdx.x + kThreads * i;
    const int krow = k0 + e / C4, col = c0 + 4 * (e % C4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (krow < k_end && col < Cn) v = mask4(*reinterpret_cast<const float4 *>(src + (size_t)row_of(idx, limit, krow) * ld + col), Cn - col);
    reg[i] = v;
  }
}
template <int BT>
__device__ __forceinline__ void store_mcontig(const float4 (&reg)[BT / 32], float *dst) {
  constexpr int C4 = BT / 4, LD = BT + kPad;
#pragma unroll
  for (int i = 0; i < BT / 32; ++i) {
    const int e = threadIdx.x + kThreads * i;
    *reinterpret_cast<float4 *>(dst + (e / C4) * LD + 4 * (e % C4)) = reg[i];
  }
}

// grid (max over the problems of tiles_m tiles_n chunks, 2)
template <int KIND, int TM, int TN>
__global__ __launch_bounds__(kThreads) void gemm_kernel(Launch launch) {
  static_assert(KIND >= kForward && KIND <= kBackwardDataLinear, "the loaders below know four kinds: kBackwardDataLinear takes backward data's by falling through their tests");
  constexpr int BM = 64 * TM, BN = 64 * TN, LDA = BM + kPad, LDB = BN + kPad;
  __shared__ __attribute__((aligned(16))) float As[kBK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[kBK * LDB];
  const Problem &p = launch.p[blockIdx.y];
  const int per_chunk = p.tiles_m * p.tiles_n;
  int tile = blockIdx.x;
  if (tile >= per_chunk * p.chunks) return;
  const int chunk = tile / per_chunk;
  tile -= chunk * per_chunk;
  const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN, M = p.M, N = p.N;
  const float *__restrict__ A = p.A;
  const float *__restrict__ B = p.B;
  const int lda = p.lda, ldb = p.ldb;
  const long long *idx = p.idx;
  const long long limit = p.idx_limit;
  int k_begin = 0, k_end = p.K;
  if (KIND == kBackwardWeight) {
    k_begin = chunk * p.chunk_rows;
    k_end = k_begin + p.chunk_rows < k_end ? k_begin + p.chunk_rows : k_end;
  }

  float4 ra[BM / 32], rb[BN / 32];
  auto fetch = [&](int k0) {
    if (KIND == kBackwardWeight) fetch_mcontig<BM>(ra, A, lda, nullptr, 0, m0, M, k0, k_end);
    else fetch_kcontig<BM>(ra, A, lda, KIND == kForward ? idx : nullptr, limit, m0, M, k0, k_end);
    if (KIND == kForward) fetch_kcontig<BN>(rb, B, ldb, nullptr, 0, n0, N, k0, k_end);
    else fetch_mcontig<BN>(rb, B, ldb, KIND == kBackwardWeight ? idx : nullptr, limit, n0, N, k0, k_end);
  };

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int wm0 = (wave >> 1) * 32 * TM, wn0 = (wave & 1) * 32 * TN;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float dbacc = 0.f;
  const bool do_db = KIND == kBackwardWeight && tn == 0 && p.dbias != nullptr && (int)threadIdx.x < BM;

  fetch(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += kBK) {
    if (KIND == kBackwardWeight) store_mcontig<BM>(ra, As); else store_kcontig<BM>(ra, As);
    if (KIND == kForward) store_kcontig<BN>(rb, Bs); else store_mcontig<BN>(rb, Bs);
    __syncthreads();
    if (k0 + kBK < k_end) fetch(k0 + kBK);
    if (do_db) {
#pragma unroll
      for (int kk = 0; kk < kBK; ++kk) dbacc += As[kk * LDA + threadIdx.x];      // (rows past k_end are zeros)
    }
#pragma unroll
    for (int kk = 0; kk < kBK; kk += 2) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[(kk + half) * LDA + wm0 + 32 * i + l31];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[(kk + half) * LDB + wn0 + 32 * j + l31];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  if (do_db && m0 + (int)threadIdx.x < M) p.dbias[(size_t)chunk * M + m0 + threadIdx.x] = dbacc;
  float *__restrict__ C = p.C + (KIND == kBackwardWeight ? (size_t)chunk * M * p.ldc : 0);
  const int ldc = p.ldc;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn0 + 32 * j + l31;                  // C layout of the 32 x 32 MFMA: column = lane & 31
    if (n >= N) continue;
    const float bias = KIND == kForward ? p.aux[n] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;      // row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        if (m >= M) continue;
        float v = acc[i][j][r];
        if (KIND == kForward) {
          v = v + bias;
          if (p.elu) v = v > 0.f ? v : expm1f(v);
        } else if (KIND == kBackwardData) {
          const float y = p.aux[(size_t)m * p.ldaux + n];
          v = v * (y > 0.f ? 1.0f : y + 1.0f);
        }
        C[(size_t)m * ldc + n] = v;
      }
  }
}

// the second half of backward weight (ppo_gemm_plan.h's ReduceTable): out[e] = sum over the chunks in index order (float64, rounded once) of part[c][e]
// grid (ceil(max numel / 256), entries)
__global__ __launch_bounds__(kThreads) void reduce_kernel(ReduceTable t) {
  const ReduceEntry &e = t.e[blockIdx.y];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= e.numel) return;
  double s = 0.0;
  for (int c = 0; c < e.chunks; ++c) s += (double)e.part[(size_t)c * e.numel + i];
  e.out[i] = (float)s;
}

}  // namespace pgemm
