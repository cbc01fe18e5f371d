// obs_norm.h -- the arithmetic of the running observation normaliser, shared by the device kernels (mpc_obs_norm.hip, include/mpc_obs_norm.h) and
// host C++ (the CPU tests compile this header with g++ and drive it against tests/obs_norm_ref.py).
//
// What it restates: rsl_rl 2.x's EmpiricalNormalization, by its published formulas (rsl_rl's source is not in the reference tree).  Per column of
// [n, D] float32 observations the state is mean, var and a row count; an update on a batch x is
//   count += n; rate = n / count
//   delta = mean_x - mean; mean += rate * delta
//   var  += rate * (var_x - var + delta * (mean_x - mean_new));  std = sqrt(var)
// with mean_x and var_x the batch mean and POPULATION variance, and normalisation is y = (x - mean) / (std + eps).  `until`: an update that finds
// count >= until is skipped.  Algebraically the state is the pooled mean and population variance of every row seen so far.
//
// What rsl_rl leaves open and this header fixes:
//   state       mean and var are float64, count is int64.  A fresh state is rsl_rl's: count 0, mean 0, var 1.  The first update that uses a row
//               ASSIGNS mean_x and var_x (the formula's value at rate = 1, without the rounding of 1 + (var_x - 1)).
//   batch       float64, two-pass inside a block of kBlockRows rows (the block's mean by one chain of adds in row order, then the squared deviations
//               from it by another), blocks joined in index order by the pooled-moments formula (join).  No sum of x^2 anywhere: a column
//               1e4 + 1e-2 z keeps its variance.
//   published   _mean, _var, _std float32 = the roundings of mean, var and sqrt(var) in float64; normalisation is float32 on those: one
//               subtraction, one addition std + eps, one division (normalize), never contracted.
//   non-finite  a row with any NaN or infinity is left out of the update and not counted (a deviation from rsl_rl, where one NaN observation ends
//               a run for good); it passes through normalize as arithmetic leaves it.  A batch with no finite row leaves the state bit-identical.
#pragma once

#include <stdint.h>

#include "rl_task.h"

namespace obs_norm {

constexpr int kBlockRows = 32;         // rows per block: the mask of the rows a block uses is one 32-bit word
constexpr int kMaxObs = 256;           // the widest observation (the device stages a block of rows in LDS)

MPC_HD bool is_finite(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, sizeof b);
  return (b & 0x7F800000u) != 0x7F800000u;
}

// the row stride of a staged block: odd, so that neither a walk along a row by consecutive rows nor one down a column by consecutive columns
// puts two lanes of a group on one LDS bank
MPC_HD int padded_stride(int D) { return D | 1; }

// count, mean and sum of squared deviations from that mean (M2) of one column over some rows
struct Moments {
  long long n;
  double mean, m2;
};

MPC_HD bool row_is_finite(const float *row, int D) {
  bool ok = true;
  for (int c = 0; c < D; ++c) ok = ok && is_finite(row[c]);
  return ok;
}

// one column of one block: col[r * stride] for r < rows (<= kBlockRows), the rows whose bit is set in `used`
MPC_HD Moments block_moments(const float *col, int stride, int rows, uint32_t used) {
  Moments m{0, 0.0, 0.0};
  double s = 0.0;
  for (int r = 0; r < rows; ++r)
    if ((used >> r) & 1u) {
      s = s + (double)col[r * stride];
      m.n += 1;
    }
  if (m.n == 0) return m;
  m.mean = s / (double)m.n;
  for (int r = 0; r < rows; ++r)
    if ((used >> r) & 1u) {
      const double d = (double)col[r * stride] - m.mean;
      m.m2 = m.m2 + d * d;
    }
  return m;
}

// the pooled moments of a (the rows before) and b (the next block)
MPC_HD Moments join(Moments a, Moments b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  const long long n = a.n + b.n;
  const double w = (double)b.n / (double)n, delta = b.mean - a.mean;
  Moments m;
  m.n = n;
  m.mean = a.mean + delta * w;
  m.m2 = a.m2 + b.m2 + delta * delta * ((double)a.n * w);
  return m;
}

// `until` < 0: never frozen
MPC_HD bool frozen(long long count, long long until) { return until >= 0 && count >= until; }

// the update of the running state by a batch with b.n >= 1 rows; count0 is the count before it (the caller adds b.n)
MPC_HD void merge(double &mean, double &var, long long count0, Moments b) {
  const double var_x = b.m2 / (double)b.n;
  if (count0 == 0) {
    mean = b.mean;
    var = var_x;
    return;
  }
  const double rate = (double)b.n / (double)(count0 + b.n);
  const double delta = b.mean - mean;
  const double mean_new = mean + rate * delta;
  var = var + rate * (var_x - var + delta * (b.mean - mean_new));
  mean = mean_new;
}

MPC_HD float normalize(float x, float mean, float std, float eps) {
  const float a = x - mean;
  const float b = std + eps;
  return a / b;
}

// ---- the host statement of one call: what the device kernels compute in three launches, walked serially ---------------------------------------
struct State {
  int D;
  float eps;
  long long until;            // < 0: none
  double *mean, *var;         // [D]
  long long *count;           // [1]
  float *pub_mean, *pub_var, *pub_std;   // [D] each
};

inline void publish(State &s) {
  for (int c = 0; c < s.D; ++c) {
    s.pub_mean[c] = (float)s.mean[c];
    s.pub_var[c] = (float)s.var[c];
    s.pub_std[c] = (float)__builtin_sqrt(s.var[c]);
  }
}

inline void clear(State &s) {
  *s.count = 0;
  for (int c = 0; c < s.D; ++c) { s.mean[c] = 0.0; s.var[c] = 1.0; }
  publish(s);
}

inline void update(State &s, const float *x, long long n) {
  if (frozen(*s.count, s.until)) return;
  const int D = s.D;
  long long used_rows = 0;
  for (int c = 0; c < D; ++c) {
    Moments acc{0, 0.0, 0.0};
    for (long long r0 = 0; r0 < n; r0 += kBlockRows) {
      const int rows = (int)(n - r0 < kBlockRows ? n - r0 : kBlockRows);
      uint32_t used = 0;
      for (int r = 0; r < rows; ++r)
        if (row_is_finite(x + (r0 + r) * D, D)) used |= 1u << r;
      acc = join(acc, block_moments(x + r0 * D + c, D, rows, used));
    }
    used_rows = acc.n;
    if (acc.n > 0) merge(s.mean[c], s.var[c], *s.count, acc);
  }
  if (used_rows > 0) {
    *s.count += used_rows;
    publish(s);
  }
}

inline void apply(State &s, const float *x, float *y, long long n, int do_update) {
  if (do_update) update(s, x, n);
  for (long long r = 0; r < n; ++r)
    for (int c = 0; c < s.D; ++c) y[r * s.D + c] = normalize(x[r * s.D + c], s.pub_mean[c], s.pub_std[c], s.eps);
}

}  // namespace obs_norm
