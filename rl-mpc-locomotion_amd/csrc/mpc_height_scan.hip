// mpc_height_scan.hip -- the C ABI of mpc_height_scan.h: the terrain height scan (height_scan.h) on the device, in one kernel.
//   height_scan_kernel   one wavefront per environment, four to a workgroup.  Lane l handles columns l, l + 64, l + 128, ... of the environment's
//                        wide row: a column below in_width is copied from the narrow buffer, one of the next P is a scan value (the point rotated by
//                        the base's yaw, the plant's own cell index, three int16 gathers, the clips), the rest is the zero pad.  Every store of a
//                        wave covers consecutive words of one row.  What belongs to the environment (five floats of the root state, the two float64
//                        words of its origin) is addressed by a wave-uniform index, so it is loaded once per wave through the scalar cache; the
//                        points table and the field are read-only.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "height_scan.h"
#include "mpc_height_scan.h"
#include "mpc_host.h"
#include "mpc_sim_internal.h"

using hscan::Config;
using hscan::Field;
using mpchost::DeviceGuard;

static_assert(MPC_HSCAN_MAX_POINTS == hscan::kMaxPoints, "mpc_height_scan.h and height_scan.h disagree");

namespace {
thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;      // 4096 environments are 1024 workgroups of four waves: one wave per SIMD of a CU
constexpr int kThreads = kWave * kWavesPerBlock;
constexpr int kMaxInWidth = 65536;

__global__ __launch_bounds__(kThreads) void height_scan_kernel(Config c, Field f, int n, int P, int in_width, int out_width,
                                                               const float *__restrict__ points, const float *__restrict__ root,
                                                               const double *__restrict__ origin, const float *__restrict__ obs_in,
                                                               float *__restrict__ obs_out, float *__restrict__ heights) {
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));      // wave-uniform
  if (r >= n) return;
  const float *rs = root + (size_t)r * 13;
  const float base[7] = {rs[0], rs[1], rs[2], 0.0f, 0.0f, rs[5], rs[6]};      // the position and the quaternion's z, w: x, y are set to 0 anyway
  const double o[2] = {origin[2 * (size_t)r], origin[2 * (size_t)r + 1]};
  const float *in = obs_in + (size_t)r * (size_t)in_width;
  float *out = obs_out + (size_t)r * (size_t)out_width;
  const int scan_end = in_width + P;
  for (int col = lane; col < out_width; col += kWave) {
    float v = 0.0f;                                                            // the pad
    if (col < in_width) {
      v = in[col];
    } else if (col < scan_end) {
      const int p = col - in_width;
      const float2 pt = reinterpret_cast<const float2 *>(points)[p];
      const float xy[2] = {pt.x, pt.y};
      float h;
      hscan::scan_point(c, f, base, o, xy, h, v);
      if (heights) heights[(size_t)r * (size_t)P + (size_t)p] = h;
    }
    out[col] = v;
  }
}
}  // namespace

struct mpc_hscan {
  int n = 0, device = 0, P = 0;
  Config c{};
  mpchost::DeviceArray<float> d_points;        // [P][2]
  Field f{};                           // the bound sim's field (null until mpc_hscan_bind)
  const double *d_origin = nullptr;    // the bound sim's own array [n][2]
};

extern "C" {

const char *mpc_hscan_last_error(void) { return g_err.c_str(); }

int mpc_hscan_width(int in_width, int P) {
  if (in_width < 0 || in_width > kMaxInWidth) return fail(MPC_E_ARG, "mpc_hscan_width: in_width must lie in [0, 65536]");
  if (P < 1 || P > MPC_HSCAN_MAX_POINTS) return fail(MPC_E_ARG, "mpc_hscan_width: P must lie in [1, 208]");
  return hscan::roundup16(in_width + P);
}

void mpc_hscan_destroy(mpc_hscan *h) { mpchost::destroy_handle(h); }

int mpc_hscan_create(mpc_hscan **out, int n, int P, const float *h_points, double offset, double clip, double scale, double obs_clip) {
  // everything is validated before the device is touched
  if (!out || !h_points) return fail(MPC_E_ARG, "mpc_hscan_create: null argument");
  if (n < 1) return fail(MPC_E_ARG, "mpc_hscan_create: n must be at least 1");
  if (P < 1 || P > MPC_HSCAN_MAX_POINTS) return fail(MPC_E_ARG, "mpc_hscan_create: P must lie in [1, 208]");
  for (int i = 0; i < 2 * P; ++i)
    if (!std::isfinite(h_points[i])) return fail(MPC_E_ARG, "mpc_hscan_create: point " + std::to_string(i / 2) + " is not finite");
  if (!std::isfinite(offset)) return fail(MPC_E_ARG, "mpc_hscan_create: offset must be finite");
  if (!std::isfinite(clip) || !(clip >= 0.0)) return fail(MPC_E_ARG, "mpc_hscan_create: clip must be finite and >= 0");
  if (!std::isfinite(scale)) return fail(MPC_E_ARG, "mpc_hscan_create: scale must be finite");
  if (!std::isfinite(obs_clip) || !(obs_clip >= 0.0)) return fail(MPC_E_ARG, "mpc_hscan_create: obs_clip must be finite and >= 0");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_hscan_create: no HIP device");
  mpc_hscan *h = new mpc_hscan();
  h->n = n;
  h->device = device;
  h->P = P;
  h->c = Config{(float)offset, (float)clip, (float)scale, (float)obs_clip};
  hipError_t e;
  if ((e = h->d_points.alloc_copy(h_points, 2 * (size_t)P)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
    mpc_hscan_destroy(h);
    return fail(MPC_E_HIP, std::string("mpc_hscan_create: ") + hipGetErrorString(e));
  }
  *out = h;
  return MPC_OK;
}

int mpc_hscan_bind(mpc_hscan *h, mpc_sim *s) {
  if (!h) return fail(MPC_E_ARG, "mpc_hscan_bind: null scan handle");
  if (!s) return fail(MPC_E_ARG, "mpc_hscan_bind: null sim handle");
  if (!s->d_heights || !s->d_origin || s->rows < 2 || s->cols < 2) return fail(MPC_E_ARG, "mpc_hscan_bind: the sim has no terrain attached");
  if (s->n != h->n)
    return fail(MPC_E_ARG, "mpc_hscan_bind: the sim has " + std::to_string(s->n) + " robots, the scan " + std::to_string(h->n) + " environments");
  if (s->device != h->device) return fail(MPC_E_ARG, "mpc_hscan_bind: the sim lives on another device");
  h->f = Field{s->d_heights, s->rows, s->cols, s->hscale, s->vscale, s->x0, s->y0};
  h->d_origin = s->d_origin;
  return MPC_OK;
}

int mpc_hscan_run(mpc_hscan *h, const float *d_root, const float *d_obs_in, int in_width, float *d_obs_out, float *d_heights, void *stream) {
  if (!h || !d_root || !d_obs_out) return fail(MPC_E_ARG, "mpc_hscan_run: bad argument");
  if (in_width < 0 || in_width > kMaxInWidth) return fail(MPC_E_ARG, "mpc_hscan_run: in_width must lie in [0, 65536]");
  if (in_width > 0 && !d_obs_in) return fail(MPC_E_ARG, "mpc_hscan_run: d_obs_in is null and in_width is not 0");
  if (d_obs_in == d_obs_out) return fail(MPC_E_ARG, "mpc_hscan_run: d_obs_out must not be d_obs_in (the rows have different widths)");
  if (!h->d_origin || !h->f.h) return fail(MPC_E_ARG, "mpc_hscan_run: no sim bound (mpc_hscan_bind)");
  DeviceGuard guard_(h->device);
  const int out_width = hscan::roundup16(in_width + h->P);
  hipLaunchKernelGGL(height_scan_kernel, dim3((unsigned)((h->n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), h->c, h->f, h->n, h->P, in_width, out_width, h->d_points, d_root, h->d_origin, d_obs_in,
                     d_obs_out, d_heights);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
