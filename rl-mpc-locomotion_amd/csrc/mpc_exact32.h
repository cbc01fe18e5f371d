// mpc_exact32.h -- the exact mode's working-set search in float32 (tuning hook MPC_EXACT_F32_SEED=1, default off).
//
// The QP of the exact mode has a unique optimum (P = alpha I + BB^T Theta BB > 0), so WHERE the active-set method starts changes how
// long it runs, not where it ends.  mpc_exact32_kernel<H> runs Goldfarb-Idnani's dual method in float32 on the swing-eliminated QP of the
// current call and hands its final working set to the fp64 active-set kernel (mpc_exact_kernel<H>, unchanged) as that kernel's seed; the
// fp64 kernel refines on it and certifies the point with the exact mode's optimality test (1e-10), and a robot it cannot certify takes
// the ADMM route as before.  Every returned point is an fp64-certified point of the exact mode; the float32 stage only decides where the
// fp64 method starts.
//
// One wavefront per robot.  Stance variables only (a foot whose five rows are equalities -- a swing foot -- is fixed at zero), in the
// Ruiz-scaled variables of the scale record (x = D^-1 f: the scaling is what keeps float32 usable, cond(P) unscaled reaches 1e7):
//   Hs = D P D  formed from the QP record's wrench description (U1 = B6^T th1 B6, U2 = B6^T diag(th2) B6, mpc_core.h build_tile),
//   Hs^-1 by symmetric sweeps in place (dense, LDS), then the dual method with the inverse Gram matrix of the working rows kept
//   explicitly (bordering on an add, rank-one downdate on a drop).
// A robot with more than NMAX stance variables, a non-finite value or a working set that overflows KMAX leaves its seed record as it
// is (the set its previous call ended on), so that robot runs exactly as in MPC_SOLVER_EXACT.
#pragma once
#include <hip/hip_runtime.h>

#include "mpc_horizon.h"

namespace mpc {

template <int H>
struct Ex32Cfg {
  static constexpr int N = 12 * H, NF = 4 * H;
  static constexpr int NMAX = N < 120 ? N : 120;   // stance variables held (Hs^-1: 57.6 KB of LDS at 120 -- two workgroups per CU)
  static constexpr int KMAX = 64;                  // working rows
  static constexpr int FMAX = NMAX / 3;            // stance feet
  static constexpr int CMAX = FMAX * 10;           // constraint sides: five rows per foot, lower and upper
};

template <int H>
struct Ex32Shared {
  using C = Ex32Cfg<H>;
  float hi[C::NMAX * C::NMAX];        // Hs, then Hs^-1 (full square)
  float gi[C::KMAX * C::KMAX];        // (N_W^T Hs^-1 N_W)^-1 of the working rows
  float u12[288];                     // U1, U2 (12 x 12 each)
  float x[C::NMAX], q[C::NMAX], z[C::NMAX], hn[C::NMAX], dv[C::NMAX], piv[C::NMAX], piv2[C::NMAX];   // (piv / piv2: the sweep's pivot column, double-buffered)
  float u[C::KMAX], w[C::KMAX], lam[C::KMAX];
  float bnd[C::FMAX * 3];             // l of row 4, u of rows 0-3, u of row 4 (unscaled, QP record)
  float cone[16];
  int foot[C::FMAX];                  // stance foot -> foot index f (its variables are 3 f .. 3 f + 2, stance slots 3 s .. 3 s + 2)
  int wrow[C::KMAX];                  // working row: stance foot * 10 + row * 2 + side (side 0: lower bound, 1: upper)
  int ns, nfs, k, fail, pick, block;
  float tstep;
};

// one constraint side in the scaled variables: n^T x >= b over the three variables of stance foot s
template <int H>
__device__ __forceinline__ void ex32_row(const Ex32Shared<H> &s, int code, float *n, float &b) {
  const int fs = code / 10, r = (code % 10) >> 1, up = code & 1;
  const float sg = up ? -1.0f : 1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = sg * s.cone[3 * r + c] * s.dv[3 * fs + c];
  const float lo = r < 4 ? 0.0f : s.bnd[3 * fs], hi = r < 4 ? s.bnd[3 * fs + 1] : s.bnd[3 * fs + 2];
  b = up ? -hi : lo;
}

template <int H>
__device__ __forceinline__ bool ex32_side_exists(const Ex32Shared<H> &s, int code) {
  const int fs = code / 10, r = (code % 10) >> 1, up = code & 1;
  if (!up) return r < 4 || s.bnd[3 * fs] > -1e29f;
  return (r < 4 ? s.bnd[3 * fs + 1] : s.bnd[3 * fs + 2]) < 1e29f;
}

// Hs^-1 n for one constraint side (three nonzeros of n), every lane its rows
template <int H>
__device__ __forceinline__ void ex32_hinv_n(const Ex32Shared<H> &s, int code, float coef, float *out, bool accumulate) {
  using C = Ex32Cfg<H>;
  float n[3], b;
  ex32_row(s, code, n, b);
  const int v0 = 3 * (code / 10);
  for (int i = threadIdx.x; i < s.ns; i += 64) {
    const float *row = s.hi + i * C::NMAX + v0;
    const float v = coef * (row[0] * n[0] + row[1] * n[1] + row[2] * n[2]);
    out[i] = accumulate ? out[i] + v : v;
  }
}

template <int H>
__device__ __forceinline__ float ex32_dot(const Ex32Shared<H> &s, int code, const float *v) {
  float n[3], b;
  ex32_row(s, code, n, b);
  const int v0 = 3 * (code / 10);
  return n[0] * v[v0] + n[1] * v[v0 + 1] + n[2] * v[v0 + 2];
}

__device__ __forceinline__ void ex32_sync() { __syncthreads(); }

// the float32 stage of one robot; returns true when `seed` was written
template <int H>
__device__ bool ex32_search(Ex32Shared<H> &s, const RobotModel &mdl, const double *__restrict__ qp, const double *__restrict__ sc, int *__restrict__ seed) {
  using C = Cfg<H>;
  using E = Ex32Cfg<H>;
  const int tid = threadIdx.x;
  // ---- stance feet, U1 / U2, scaled q
  if (tid == 0) {
    int nfs = 0, fail = 0;
    for (int f = 0; f < C::NF; ++f) {
      const double l4 = qp[C::QP_BND + 3 * f], u03 = qp[C::QP_BND + 3 * f + 1], u4 = qp[C::QP_BND + 3 * f + 2];
      const bool fixed = u03 <= 0.0 && u4 - l4 <= 0.0;      // every row an equality at zero: a swing foot (eliminated, like the reference)
      if (fixed) continue;
      if (nfs >= E::FMAX) { fail = 1; break; }
      s.foot[nfs] = f;
      s.bnd[3 * nfs] = (float)l4; s.bnd[3 * nfs + 1] = (float)u03; s.bnd[3 * nfs + 2] = (float)u4;
      ++nfs;
    }
    s.nfs = nfs; s.ns = 3 * nfs; s.fail = fail; s.k = 0;
  }
  if (tid < 15) s.cone[tid] = (float)qp[C::QP_CONE + tid];
  for (int e = tid; e < 288; e += 64) {
    const int which = e / 144, ab = e - 144 * which, a = ab / 12, b = ab - 12 * a;
    const double *B6 = qp + C::QP_B6;
    double acc = 0.0;
    if (which == 0) {
      for (int p = 0; p < 6; ++p) {
        double row = 0.0;
        for (int r = 0; r < 6; ++r) row += qp[C::QP_TH1 + 6 * p + r] * B6[12 * r + b];
        acc += B6[12 * p + a] * row;
      }
    } else {
      for (int p = 0; p < 6; ++p) acc += B6[12 * p + a] * (qp[C::QP_TH2 + p] * B6[12 * p + b]);
    }
    s.u12[e] = (float)acc;
  }
  ex32_sync();
  if (s.fail || s.nfs == 0) return false;
  const int ns = s.ns;
  for (int i = tid; i < ns; i += 64) {
    const int gv = 3 * s.foot[i / 3] + i % 3;
    const double d = sc[C::SC_D + gv];
    s.dv[i] = (float)d;
    s.q[i] = (float)(d * qp[C::QP_Q + gv]);
  }
  ex32_sync();
  // ---- Hs = D P D (P[(t, a), (t', b)] = s2 U1[a][b] + m U2[a][b] + [same entry] alpha, m = H - max(t, t'), d = |t - t'|)
  const float alpha = (float)mdl.alpha;
  // (every phase from here to the dual method works on the rows its lane owns: row i belongs to lane i mod 64)
  for (int i = tid; i < ns; i += 64) {
    const int fi = s.foot[i / 3], ti = fi >> 2, a = 3 * (fi & 3) + i % 3;
    for (int fj = 0; fj < s.nfs; ++fj) {
      const int ff = s.foot[fj], tj = ff >> 2;
      const float m = (float)(H - (ti > tj ? ti : tj)), d = (float)(ti > tj ? ti - tj : tj - ti);
      const float s2 = m * (4.0f * m * m - 1.0f) / 12.0f + d * (m * m) * 0.5f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int j = 3 * fj + c, b = 3 * (ff & 3) + c;
        float v = s2 * s.u12[12 * a + b] + m * s.u12[144 + 12 * a + b];
        if (i == j) v += alpha;
        s.hi[i * E::NMAX + j] = s.dv[i] * v * s.dv[j];
      }
    }
  }
  // ---- Hs^-1 by symmetric sweeps: after every pivot is swept, hi = -Hs^-1.  Lane-owned rows: a lane publishes its entry of the pivot column,
  // one barrier, then it updates its own rows (the column is double-buffered, so the next pivot's publication needs no second barrier).
  for (int kk = 0; kk < ns; ++kk) {
    float *pc = (kk & 1) ? s.piv2 : s.piv;
    for (int i = tid; i < ns; i += 64) pc[i] = s.hi[i * E::NMAX + kk];
    ex32_sync();
    const float dk = pc[kk];
    if (!(dk > 0.0f)) { if (tid == 0) s.fail = 1; }
    const float rdk = 1.0f / dk;
    for (int i = tid; i < ns; i += 64) {
      float *row = s.hi + i * E::NMAX;
      const float pi = pc[i] * rdk;
      if (i == kk) {
        for (int j = 0; j < ns; ++j) row[j] = pc[j] * rdk;
        row[kk] = -rdk;
      } else {
        for (int j = 0; j < ns; ++j) row[j] -= pi * pc[j];
        row[kk] = pi;
      }
    }
  }
  ex32_sync();
  if (s.fail) return false;
  for (int i = tid; i < ns; i += 64)
    for (int j = 0; j < ns; ++j) s.hi[i * E::NMAX + j] = -s.hi[i * E::NMAX + j];
  // ---- unconstrained minimiser x = -Hs^-1 q
  for (int i = tid; i < ns; i += 64) {
    float acc = 0.0f;
    for (int j = 0; j < ns; ++j) acc += s.hi[i * E::NMAX + j] * s.q[j];
    s.x[i] = -acc;
  }
  ex32_sync();
  // ---- the dual method
  const int nc = 10 * s.nfs;
  const int max_pass = 3 * ns + 32;
  bool done = false;
  for (int pass = 0; pass < max_pass && !done; ++pass) {
    // the most violated side not in the working set (relative violation), wavefront arg-min
    float best = 0.0f;
    int bi = -1;
    for (int c = tid; c < nc; c += 64) {
      if (!ex32_side_exists(s, c)) continue;
      bool in = false;
      for (int j = 0; j < s.k; ++j) in |= s.wrow[j] == c;
      if (in) continue;
      float n[3], b;
      ex32_row(s, c, n, b);
      const int v0 = 3 * (c / 10);
      const float ax = n[0] * s.x[v0] + n[1] * s.x[v0 + 1] + n[2] * s.x[v0 + 2];
      const float scale = 1.0f + fabsf(b) + fabsf(n[0] * s.x[v0]) + fabsf(n[1] * s.x[v0 + 1]) + fabsf(n[2] * s.x[v0 + 2]);
      const float viol = (ax - b) / scale;
      if (viol < best) { best = viol; bi = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (ob < best || (ob == best && oi >= 0 && (bi < 0 || oi < bi))) { best = ob; bi = oi; }
    }
    if (bi < 0 || best > -1e-6f) { done = true; break; }
    const int p = bi;
    float lamp = 0.0f;
    bool added = false;
    // steps towards row p: partial steps drop blocking rows, a full step adds p
    for (int inner = 0; inner <= E::KMAX; ++inner) {
      const int k = s.k;
      ex32_hinv_n(s, p, 1.0f, s.hn, false);
      ex32_sync();
      for (int j = tid; j < k; j += 64) s.u[j] = ex32_dot(s, s.wrow[j], s.hn);
      ex32_sync();
      for (int j = tid; j < k; j += 64) {
        float acc = 0.0f;
        for (int l = 0; l < k; ++l) acc += s.gi[j * E::KMAX + l] * s.u[l];
        s.w[j] = acc;
      }
      ex32_sync();
      for (int i = tid; i < ns; i += 64) s.z[i] = s.hn[i];
      for (int j = 0; j < k; ++j) { ex32_hinv_n(s, s.wrow[j], -s.w[j], s.z, true); }
      ex32_sync();
      if (tid == 0) {
        float np[3], bp;
        ex32_row(s, p, np, bp);
        const float zn = ex32_dot(s, p, s.z);
        const float slack = ex32_dot(s, p, s.x) - bp;
        float t1 = 3e38f; int blk = -1;
        for (int j = 0; j < k; ++j)
          if (s.w[j] > 0.0f && s.lam[j] / s.w[j] < t1) { t1 = s.lam[j] / s.w[j]; blk = j; }
        const float zz = ex32_dot(s, p, s.hn);
        const bool full_ok = zn > 1e-7f * (zz > 0.0f ? zz : 1.0f) && slack < 0.0f;
        const float t2 = full_ok ? -slack / zn : 3e38f;
        if (blk < 0 && !full_ok) { s.fail = 1; s.block = -2; }
        else if (full_ok && t2 <= t1) { s.tstep = t2; s.block = -1; }
        else { s.tstep = t1; s.block = blk; }
        if (!(s.tstep < 3e38f) || s.tstep != s.tstep) s.fail = 1;
        s.pick = full_ok ? 1 : 0;
        s.piv[0] = zn;
      }
      ex32_sync();
      if (s.fail) return false;
      const float t = s.tstep;
      const int blk = s.block;
      if (s.pick) for (int i = tid; i < ns; i += 64) s.x[i] += t * s.z[i];
      for (int j = tid; j < k; j += 64) s.lam[j] -= t * s.w[j];
      lamp += t;
      ex32_sync();
      if (blk < 0) {      // full step: p joins the working set (the inverse Gram matrix bordered)
        if (k >= E::KMAX) { return false; }
        const float d = s.piv[0];
        const float rd = 1.0f / d;
        for (int i = tid; i <= k; i += 64)
          for (int j = 0; j <= k; ++j) {
            float v;
            if (i < k && j < k) v = s.gi[i * E::KMAX + j] + s.w[i] * s.w[j] * rd;
            else if (i < k) v = -s.w[i] * rd;
            else if (j < k) v = -s.w[j] * rd;
            else v = rd;
            s.gi[i * E::KMAX + j] = v;
          }
        if (tid == 0) { s.wrow[k] = p; s.lam[k] = lamp; s.k = k + 1; }
        ex32_sync();
        added = true;
        break;
      }
      // partial step: the blocking row leaves (moved to the last slot, then the rank-one downdate of the leading block)
      const int last = k - 1;
      if (blk != last) {
        for (int i = tid; i < k; i += 64) {       // swap rows blk and last
          const float a = s.gi[blk * E::KMAX + i], b = s.gi[last * E::KMAX + i];
          s.gi[blk * E::KMAX + i] = b; s.gi[last * E::KMAX + i] = a;
        }
        ex32_sync();
        for (int i = tid; i < k; i += 64) {       // ... and columns
          const float a = s.gi[i * E::KMAX + blk], b = s.gi[i * E::KMAX + last];
          s.gi[i * E::KMAX + blk] = b; s.gi[i * E::KMAX + last] = a;
        }
        if (tid == 0) {
          const int wr = s.wrow[blk]; s.wrow[blk] = s.wrow[last]; s.wrow[last] = wr;
          const float lm = s.lam[blk]; s.lam[blk] = s.lam[last]; s.lam[last] = lm;
        }
        ex32_sync();
      }
      for (int i = tid; i < last; i += 64) s.piv[i] = s.gi[i * E::KMAX + last];
      ex32_sync();
      const float rb = 1.0f / s.gi[last * E::KMAX + last];
      for (int i = tid; i < last; i += 64)
        for (int j = 0; j < last; ++j) s.gi[i * E::KMAX + j] -= s.piv[i] * s.piv[j] * rb;
      if (tid == 0) s.k = last;
      ex32_sync();
    }
    if (!added) return false;      // (every row dropped and still no full step: the dual state is not consistent any more -- give up)
  }
  if (!done) return false;
  // ---- the seed record (mpc_wrench.h seed_code: 2 bits per row, 1 lower / 2 upper; bit 10 fixed foot; bit 11 valid).  The fp64 kernel
  // first tries the previous call's set moved by one horizon step (code of step k read from slot k + 1), so this call's set is written
  // moved the other way: slot k + 1 holds step k's code, slot 0 step 0's; the last step then starts from step H - 2's rows.
  for (int f = tid; f < C::NF; f += 64) {
    int code = (1 << 11);
    int fs = -1;
    for (int j = 0; j < s.nfs; ++j) fs = s.foot[j] == f ? j : fs;
    if (fs < 0) code |= 1 << 10;
    else {
      int cnt = 0;
      for (int j = 0; j < s.k; ++j) {
        const int c = s.wrow[j];
        if (c / 10 != fs || cnt >= 3) continue;
        code |= ((c & 1) ? 2 : 1) << (2 * ((c % 10) >> 1));
        ++cnt;
      }
    }
    const int step = f >> 2, leg = f & 3;
    if (step + 1 < H) seed[(step + 1) * 4 + leg] = code;
    if (step == 0) seed[leg] = code;
  }
  return true;
}

// one workgroup (one wavefront) per robot of the launch's job list
template <int H>
__global__ __launch_bounds__(64, 1) void mpc_exact32_kernel(const RobotModel *__restrict__ models, const double *__restrict__ qp, const double *__restrict__ sc,
                                                            const int *__restrict__ order, const int *__restrict__ sched, int *__restrict__ seed) {
  __shared__ __attribute__((aligned(16))) Ex32Shared<H> sh;
  using C = Cfg<H>;
  if ((int)blockIdx.x >= sched[kSchedJobs]) return;
  const int robot = order[blockIdx.x];
  (void)ex32_search<H>(sh, models[robot], qp + (size_t)robot * C::QP_LEN, sc + (size_t)robot * C::SC_LEN, seed + (size_t)robot * C::NF);
}

}  // namespace mpc
