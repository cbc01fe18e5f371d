// ppo_gemm_plan.h -- which instantiation of ppo_gemm.h's kernel a launch runs, and how backward weight is chunked: a pure function of the two problems'
// (M, N, K) and the kind, with no HIP in it, so the host tests compile it with g++ and pin which shapes reach which kernel (tests/test_ppo_gemm_plan.py).
//   backward weight  the reduction (the mini-batch's rows) is split into chunks of the largest of 1024, 512, 256 rows that gives the chip two workgroups
//                    per CU, counted in 128 x 64 tiles (a chunk's workgroup walks its rows alone)
//   tile             128 x 128 where every problem's columns fill such tiles and there is one for every CU; 128 x 64 otherwise
#pragma once

namespace pgemm {

enum Kind { kForward = 0, kBackwardData = 1, kBackwardWeight = 2, kBackwardDataLinear = 3 };      // (3: backward data with no activation factor; planned as 1)

constexpr int kChunk = 1024;          // most rows per backward-weight chunk: the longest fp32 chain
constexpr int kMinChunk = 256;        // fewest: a workspace holds ceil(max_rows / kMinChunk) partials per layer
constexpr int kMinWorkgroups = 512;   // two per CU: a longer chunk is taken only where it leaves this many workgroups
constexpr int kMinWideTiles = 256;    // one per CU: fewer 128 x 128 tiles than this run as 128 x 64

struct Shape { int M, N, K; };        // output M x N, reduction K; M <= 0: the slot is empty

struct ProblemPlan { int tiles_m, tiles_n, chunks; };      // an empty slot: 0, 0, 1

struct Plan {
  int chunk_rows;                     // backward weight: reduction rows per chunk; 0 for the other kinds
  bool wide;                          // gemm_kernel<KIND, 2, 2> (128 x 128), else gemm_kernel<KIND, 2, 1> (128 x 64)
  unsigned grid_x;                    // the largest tiles_m tiles_n chunks of the two problems; 0: nothing to launch
  ProblemPlan p[2];
};

inline Plan plan_gemm(int kind, const Shape (&shape)[2]) {
  Plan plan{};
  for (auto &q : plan.p) q.chunks = 1;
  if (kind == kBackwardWeight) {
    int rows_per = kChunk;
    for (;; rows_per /= 2) {
      long long wgs = 0;
      for (const Shape &s : shape)
        if (s.M > 0) wgs += (long long)((s.M + 127) / 128) * ((s.N + 63) / 64) * ((s.K + rows_per - 1) / rows_per);
      if (wgs >= kMinWorkgroups || rows_per == kMinChunk) break;
    }
    plan.chunk_rows = rows_per;
    for (int k = 0; k < 2; ++k)
      if (shape[k].M > 0) plan.p[k].chunks = (shape[k].K + rows_per - 1) / rows_per;
  }
  plan.wide = true;
  long long tiles128 = 0;
  for (int k = 0; k < 2; ++k) {
    const Shape &s = shape[k];
    if (s.M <= 0) continue;
    if (s.N % 128 != 0) plan.wide = false;
    tiles128 += (long long)((s.M + 127) / 128) * ((s.N + 127) / 128) * plan.p[k].chunks;
  }
  if (tiles128 < kMinWideTiles) plan.wide = false;
  const int bn = plan.wide ? 128 : 64;
  for (int k = 0; k < 2; ++k) {
    const Shape &s = shape[k];
    ProblemPlan &q = plan.p[k];
    if (s.M <= 0) { q.tiles_m = q.tiles_n = 0; q.chunks = 1; continue; }
    q.tiles_m = (s.M + 127) / 128;
    q.tiles_n = (s.N + bn - 1) / bn;
    const unsigned g = (unsigned)(q.tiles_m * q.tiles_n * q.chunks);
    plan.grid_x = g > plan.grid_x ? g : plan.grid_x;
  }
  return plan;
}

// ---- what a caller of the GEMMs fills; the kernels (ppo_gemm.h) live in mpc_ppo_gemm.hip alone and are reached through launch and reduce below
struct Problem {
  const float *A, *B;                 // see ppo_gemm.h's loaders for each kind's layout
  float *C;                           // [M][ldc]; backward weight: [chunks][M][ldc]
  const float *aux;                   // forward: bias [N]; backward data: the stored activation [M][ldaux]; backward data linear: not read
  const long long *idx;               // rows of X are idx[row] (forward: of A; backward weight: of B); null: the rows themselves
  float *dbias;                       // backward weight: [chunks][M] column sums of dY (null: none)
  long long idx_limit;                // idx values are clamped to [0, idx_limit)
  int M, N, K;                        // output M x N, reduction K
  int lda, ldb, ldc, ldaux;
  int elu;                            // forward: apply ELU
  int tiles_m, tiles_n, chunks;       // tiles_m = 0: nothing to do
  int chunk_rows;                     // backward weight: reduction rows per chunk
};

struct Launch { Problem p[2]; };

// the second half of backward weight: out[e] = sum over the chunks in index order (float64, rounded once) of part[c][e]
constexpr int kMaxReduce = 32;
struct ReduceEntry {
  const float *part;      // [chunks][numel]
  float *out;             // [numel]
  int numel, chunks;
};
struct ReduceTable { ReduceEntry e[kMaxReduce]; };

// mpc_ppo_gemm.hip.  launch: plan_gemm's plan filled into L (the caller reads the chunk counts back) and the instantiation it names started on
// `stream` (a hipStream_t).  reduce: reduce_kernel over the first `entries` of t, the longest max_numel elements.  The caller asks hipGetLastError.
void launch(Kind kind, Launch &L, void *stream);
void reduce(const ReduceTable &t, int entries, int max_numel, void *stream);

}  // namespace pgemm
