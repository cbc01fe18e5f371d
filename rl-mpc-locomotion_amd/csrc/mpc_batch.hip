// mpc_batch.hip -- the solver handle of include/mpc_batch.h (mpc_batch_*): record buffers, warm starts, launches, and the device clock probe.
// The solver kernels are instantiated per planning horizon in mpc_horizon.hip (one translation unit per horizon, mpc_horizon.h) and
// reached through their HorizonOps entries.  The per-tick controller and FSM are mpc_ctrl.hip, the weight policy is mpc_policy.hip; what they
// may know of this unit is mpc_batch_internal.h, and their errors land in this unit's slot (one mpc_last_error for the three).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mpc_batch.h"
#include "mpc_batch_internal.h"
#include "mpc_model.h"

using namespace mpc;
using mpchost::DeviceArray;
using mpchost::DeviceGuard;

#define MPC_DECL_OPS(HH) extern "C" const mpc::HorizonOps *mpc_horizon_ops_##HH(void);
MPC_HORIZON_LIST(MPC_DECL_OPS)
#undef MPC_DECL_OPS

namespace {

thread_local mpchost::ErrorSlot g_err;
int fail(int code, const std::string &msg) { return g_err.fail(code, msg); }

// the kernel set of a planning horizon, or null when the library was built without it (-DMPC_HORIZON_LIST)
const HorizonOps *horizon_ops(int h) {
#define MPC_ITEM(HH) if (h == HH) return mpc_horizon_ops_##HH();
  MPC_HORIZON_LIST(MPC_ITEM)
#undef MPC_ITEM
  return nullptr;
}

__global__ void reset_kernel(double *state, int state_len, const int *ids, int k, int n, int *seed, int seed_len) {
  const int r = blockIdx.x;
  const int robot = ids ? ids[r] : r;
  if (r >= k || robot < 0 || robot >= n) return;
  for (int i = threadIdx.x; i < state_len; i += blockDim.x) state[(size_t)robot * state_len + i] = 0.0;
  for (int i = threadIdx.x; i < seed_len; i += blockDim.x) seed[(size_t)robot * seed_len + i] = 0;      // (a new ConvexMpc object knows no working set either)
}

// mpc_device_clock: one dependent float64 multiply-add chain per lane (v_mul_f64 + v_add_f64 pairs: the unit is built without contraction),
// one wave per SIMD on every CU (the solve kernel's own regime); shader cycles (s_memtime) of workgroup 0 over the HIP-event time of the
// launch = the shader clock the device grants under that load, whichever instructions the chain is made of.
__global__ __launch_bounds__(64) void clock_probe_kernel(long long *out, int iters) {
  double a = threadIdx.x * 1e-3 + 1.0, b = 1.0000001, c = 1e-9;
  const long long t0 = __builtin_readcyclecounter();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int k = 0; k < 32; ++k) a = a * b + c;
  }
  const long long t1 = __builtin_readcyclecounter();
  if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0 + (a == 0.5 ? 1 : 0);
}

// The whole batch as new ConvexMpc objects: no warm start (d_state) and no working set (d_seed).  The per-robot form is reset_kernel's.
size_t state_bytes(const mpc_batch *b) { return sizeof(double) * (size_t)b->n * b->state_len; }
hipError_t clear_state(mpc_batch *b, hipStream_t st) { return hipMemsetAsync(b->d_state, 0, state_bytes(b), st); }
hipError_t clear_seed(mpc_batch *b, hipStream_t st) { return hipMemsetAsync(b->d_seed, 0, sizeof(int) * (size_t)b->n * batchint::seed_len(b), st); }
int cold_start(mpc_batch *b, hipStream_t st) {
  HIP_TRY(clear_state(b, st));
  HIP_TRY(clear_seed(b, st));
  return MPC_OK;
}

// the input records [n, 56 + 4 h] of a launch, as float32, float64 or float16: exactly one is set
struct Records { const float *f32; const double *f64; const _Float16 *f16; };
Records records(const float *d_in) { return {d_in, nullptr, nullptr}; }
Records records(const double *d_in) { return {nullptr, d_in, nullptr}; }
Records records(const unsigned short *d_in) { return {nullptr, nullptr, reinterpret_cast<const _Float16 *>(d_in)}; }

// one solver launch on b's robots (+ the dispatch order for the next one)
int launch_solver(mpc_batch *b, Records in, double *d_forces, int *d_info, const int *d_active, hipStream_t st) {
  DeviceGuard guard_(b->device);
  const int slot = (int)(b->order_launches++ % kOrderHistory);
  if (b->exact) HIP_TRY(clear_state(b, st));   // no warm start in that branch (mpc_osqp.cc:906-919)
  hipEvent_t *ev = b->timing ? b->ev[b->launches % kTimingRing] : nullptr;
  const LaunchArgs a{b->n, b->d_models, in.f32, in.f64, in.f16, b->d_state, b->d_qp, b->d_sc, d_forces, d_info, b->d_prof, d_active, b->d_order, b->d_hist, slot, ev, st, b->exact,
                     b->max_iter, b->d_sched, b->d_ready, b->job_slots, b->warm_sets ? b->d_seed : nullptr,
                     b->warm_sets && b->f32_seed};
  const hipError_t e = (hipError_t)b->ops->launch(a);
  if (e != hipSuccess) return fail(MPC_E_HIP, std::string("solver launch: ") + hipGetErrorString(e));
  b->launches++;
  return MPC_OK;
}

// mpc_batch_solve, _f64, _f16: the records are on the device
int solve_device(const char *who, mpc_batch *b, Records in, double *d_forces, int *d_info, void *stream) {
  if (!b || !(in.f32 || in.f64 || in.f16) || !d_forces) return fail(MPC_E_ARG, std::string(who) + ": bad argument");
  return launch_solver(b, in, d_forces, d_info ? d_info : b->d_info, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// mpc_batch_solve_host, _f64: the records come from and the forces go to host memory, through staging buffers kept for the life of the handle
template <typename T>
int solve_host(const char *who, mpc_batch *b, DeviceArray<T> mpc_batch::*staging, const T *h_in, double *h_forces, int *h_info) {
  if (!b || !h_in || !h_forces) return fail(MPC_E_ARG, std::string(who) + ": bad argument");
  DeviceGuard guard_(b->device);
  DeviceArray<T> &d_in = b->*staging;
  const size_t inlen = 56 + 4 * (size_t)b->h, N = 12 * (size_t)b->h;
  if (!d_in) {
    HIP_TRY(d_in.alloc(b->n * inlen));
    if (!b->d_host_f) HIP_TRY(b->d_host_f.alloc(b->n * N));
  }
  HIP_TRY(hipMemcpy(d_in, h_in, sizeof(T) * b->n * inlen, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_host_f, h_forces, sizeof(double) * b->n * N, hipMemcpyHostToDevice));   // rows of unsolved robots stay as passed in
  const int rc = solve_device(who, b, records(d_in.get()), b->d_host_f, nullptr, nullptr);
  if (rc != MPC_OK) return rc;
  HIP_TRY(hipMemcpy(h_forces, b->d_host_f, sizeof(double) * b->n * N, hipMemcpyDeviceToHost));     // (synchronises with the null stream)
  if (h_info) HIP_TRY(hipMemcpy(h_info, b->d_info, sizeof(int) * b->n * kInfoLen, hipMemcpyDeviceToHost));
  return MPC_OK;
}

// mpc_batch_reset, _device: the robots of an id list as new ConvexMpc objects
int reset_ids(mpc_batch *b, const int *ids, int k, mpchost::Ids where, hipStream_t st) {
  const auto launch = [&](const int *d_ids, int cnt) {
    hipLaunchKernelGGL(reset_kernel, dim3(cnt), dim3(256), 0, st, b->d_state, b->state_len, d_ids, cnt, b->n, b->d_seed, batchint::seed_len(b));
  };
  HIP_TRY(mpchost::launch_over_ids(ids, k, b->n, where, st, launch));
  return MPC_OK;
}

int fetch_records(mpc_batch *b, double *h_qp, double *h_sc) {
  const size_t ql = b->ops->qp_len, sl = b->ops->sc_len, xql = b->ops->xqp_len, xsl = b->ops->xsc_len;
  std::vector<double> qp((size_t)b->n * ql), sc((size_t)b->n * sl);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(qp.data(), b->d_qp, sizeof(double) * qp.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sc.data(), b->d_sc, sizeof(double) * sc.size(), hipMemcpyDeviceToHost));
  for (int r = 0; r < b->n; ++r)
    b->ops->expand(qp.data() + (size_t)r * ql, sc.data() + (size_t)r * sl, h_qp ? h_qp + (size_t)r * xql : nullptr, h_sc ? h_sc + (size_t)r * xsl : nullptr);
  return MPC_OK;
}

}  // namespace

int batchint::launch(mpc_batch *b, const float *d_rec, double *d_forces, int *d_info, const int *d_active, hipStream_t stream) {
  return launch_solver(b, records(d_rec), d_forces, d_info, d_active, stream);
}
int batchint::set_error(int code, const std::string &msg) { return fail(code, msg); }

extern "C" {

const char *mpc_last_error(void) { return g_err.c_str(); }
int mpc_input_len(int horizon) { return 56 + 4 * horizon; }
int mpc_supported_horizons(int *out, int cap) {
#define MPC_ITEM(HH) HH,
  const int hs[] = {MPC_HORIZON_LIST(MPC_ITEM)};
#undef MPC_ITEM
  const int cnt = (int)(sizeof hs / sizeof *hs);
  for (int i = 0; i < cnt && i < cap; ++i) out[i] = hs[i];
  return cnt;
}

int mpc_batch_create(mpc_batch **out, int n, int horizon, double timestep, double alpha, const double *mass,
                     const double *inertia9) {
  if (!out || n <= 0 || !mass || !inertia9) return fail(MPC_E_ARG, "mpc_batch_create: bad argument");
  const HorizonOps *ops = horizon_ops(horizon);
  if (!ops) return fail(MPC_E_HORIZON, "mpc_batch_create: planning horizon outside the built range (mpc_supported_horizons: 2 .. 20 in the shipped library)");
  const int device = mpchost::current_device();
  if (device < 0) return fail(MPC_E_NODEVICE, "mpc_batch_create: no HIP device");
  mpc_batch *b = new mpc_batch();
  b->device = device;
  b->n = n;
  b->h = horizon;
  b->ops = ops;
  const size_t qp_len = ops->qp_len, sc_len = ops->sc_len;
  b->state_len = (int)(64 * horizon + 2);
  std::vector<RobotModel> models(n);
  for (int i = 0; i < n; ++i) models[i] = make_model(mass[i], inertia9 + 9 * (size_t)i, timestep, alpha);
  const size_t N = (size_t)n;
  hipError_t e;
  if ((e = b->d_models.alloc_copy(models.data(), N)) != hipSuccess || (e = b->d_state.alloc_zero(N * b->state_len)) != hipSuccess ||
      (e = b->d_qp.alloc(N * qp_len)) != hipSuccess || (e = b->d_sc.alloc(N * sc_len)) != hipSuccess ||
      (e = b->d_info.alloc(N * kInfoLen)) != hipSuccess || (e = b->d_prof.alloc_zero(N * kProfLen)) != hipSuccess ||
      (e = b->d_order.alloc(N)) != hipSuccess || (e = b->d_hist.alloc_zero(N * kOrderHistory)) != hipSuccess ||
      (e = b->d_sched.alloc(kSchedLen)) != hipSuccess || (e = b->d_ready.alloc(N)) != hipSuccess ||
      (e = b->d_seed.alloc_zero(N * batchint::seed_len(b))) != hipSuccess) {
    mpc_batch_destroy(b);
    return fail(MPC_E_HIP, std::string("mpc_batch_create: ") + hipGetErrorString(e));
  }
  {   // the persistent job kernel runs one workgroup per wave slot: four single-wave workgroups per CU (one per SIMD, full register budget)
    hipDeviceProp_t prop;
    const char *env = getenv("MPC_SOLVE_JOBS");      // tuning hook: 0 = one workgroup per robot (the round-2 launch), N > 0 = that many slots
    if (hipGetDeviceProperties(&prop, b->device) == hipSuccess) b->job_slots = 4 * prop.multiProcessorCount;
    if (env) {   // (anything that is not a number, or negative, is ignored; fewer slots than one multi-wave workgroup needs means "not persistent")
      char *end = nullptr;
      const long v = strtol(env, &end, 10);
      if (end != env && *end == '\0' && v >= 0 && v <= (1 << 20)) b->job_slots = v < 2 ? 0 : (int)v;
    }
  }
  if (const char *ew = getenv("MPC_EXACT_WARM")) b->warm_sets = !(ew[0] == '0' && ew[1] == '\0');      // tuning hook: 0 = the exact mode's active-set method starts empty on every call
  if (const char *fs = getenv("MPC_EXACT_F32_SEED")) b->f32_seed = fs[0] == '1' && fs[1] == '\0';   // tuning hook: 1 = seed from the float32 search
  b->bytes = (long long)(sizeof(RobotModel) * n + sizeof(double) * (size_t)n * (b->state_len + qp_len + sc_len) + sizeof(int) * (size_t)n * kInfoLen);
  *out = b;
  return MPC_OK;
}

void mpc_batch_destroy(mpc_batch *b) { mpchost::destroy_handle(b); }

int mpc_batch_solve(mpc_batch *b, const float *d_in, double *d_forces, int *d_info, void *stream) {
  return solve_device("mpc_batch_solve", b, records(d_in), d_forces, d_info, stream);
}
int mpc_batch_solve_f64(mpc_batch *b, const double *d_in, double *d_forces, int *d_info, void *stream) {
  return solve_device("mpc_batch_solve_f64", b, records(d_in), d_forces, d_info, stream);
}
int mpc_batch_solve_f16(mpc_batch *b, const unsigned short *d_in, double *d_forces, int *d_info, void *stream) {
  return solve_device("mpc_batch_solve_f16", b, records(d_in), d_forces, d_info, stream);
}
int mpc_batch_solve_host(mpc_batch *b, const float *h_in, double *h_forces, int *h_info) {
  return solve_host("mpc_batch_solve_host", b, &mpc_batch::d_host_in, h_in, h_forces, h_info);
}
int mpc_batch_solve_host_f64(mpc_batch *b, const double *h_in, double *h_forces, int *h_info) {
  return solve_host("mpc_batch_solve_host_f64", b, &mpc_batch::d_host_in64, h_in, h_forces, h_info);
}

int mpc_batch_set_solver(mpc_batch *b, int solver) {
  if (!b || (solver != MPC_SOLVER_OSQP && solver != MPC_SOLVER_EXACT)) return fail(MPC_E_ARG, "mpc_batch_set_solver: MPC_SOLVER_OSQP (0) or MPC_SOLVER_EXACT (1)");
  const bool exact = solver == MPC_SOLVER_EXACT;
  if (exact != b->exact && b->d_seed) {      // a working set left by an earlier stretch in the exact mode is not this stretch's
    DeviceGuard guard_(b->device);
    HIP_TRY(hipDeviceSynchronize());      // (no stream argument here: solves in flight on any stream, non-blocking ones included, are over before the working sets go ...
    HIP_TRY(clear_seed(b, nullptr));
    HIP_TRY(hipDeviceSynchronize());      // ... and the clear is complete before a solve launched right after on such a stream can read them)
  }
  b->exact = exact;
  return MPC_OK;
}

int mpc_batch_set_max_iter(mpc_batch *b, int max_iter) {
  if (!b || max_iter <= 0 || max_iter % kCheck != 0) return fail(MPC_E_ARG, "mpc_batch_set_max_iter: a positive multiple of 25 (OSQP's check_termination interval)");
  b->max_iter = max_iter;
  return MPC_OK;
}

int mpc_batch_reset(mpc_batch *b, const int *ids, int k, void *stream) {
  if (!b) return fail(MPC_E_ARG, "mpc_batch_reset: bad argument");
  DeviceGuard guard_(b->device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return ids ? reset_ids(b, ids, k, mpchost::Ids::host, st) : cold_start(b, st);
}

int mpc_batch_reset_device(mpc_batch *b, const int *d_ids, int k, void *stream) {
  if (!b || !d_ids || k < 0) return fail(MPC_E_ARG, "mpc_batch_reset_device: bad argument");
  DeviceGuard guard_(b->device);
  return reset_ids(b, d_ids, k, mpchost::Ids::device, reinterpret_cast<hipStream_t>(stream));
}

int mpc_batch_enable_timing(mpc_batch *b) {
  if (!b) return fail(MPC_E_ARG, "mpc_batch_enable_timing: bad argument");
  if (!b->timing) {
    for (auto &e3 : b->ev) for (auto &e : e3) HIP_TRY(hipEventCreate(&e));
    b->timing = true;
    b->launches = 0;
  }
  return MPC_OK;
}
int mpc_batch_kernel_times(mpc_batch *b, int last_k, float *ms_assemble, float *ms_solve) {
  if (!b || !b->timing || last_k <= 0 || last_k > kTimingRing || last_k > b->launches || !ms_assemble || !ms_solve)
    return fail(MPC_E_ARG, "mpc_batch_kernel_times: bad argument (enable timing first; at most 64 launches back)");
  DeviceGuard guard_(b->device);
  HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < last_k; ++i) {
    hipEvent_t *e = b->ev[(b->launches - last_k + i) % kTimingRing];
    HIP_TRY(hipEventElapsedTime(ms_assemble + i, e[0], e[1]));
    HIP_TRY(hipEventElapsedTime(ms_solve + i, e[1], e[2]));
  }
  return MPC_OK;
}
int mpc_batch_size(const mpc_batch *b) { return b ? b->n : 0; }
int mpc_batch_horizon(const mpc_batch *b) { return b ? b->h : 0; }
long long mpc_batch_device_bytes(const mpc_batch *b) { return b ? b->bytes : 0; }
int mpc_batch_state_len(const mpc_batch *b) { return b ? b->state_len : 0; }
int mpc_batch_get_state(mpc_batch *b, double *h_state) {
  if (!b || !h_state) return fail(MPC_E_ARG, "mpc_batch_get_state: bad argument");
  DeviceGuard guard_(b->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_state, b->d_state, state_bytes(b), hipMemcpyDeviceToHost));
  return MPC_OK;
}
// Test / debugging access to what the prep kernel handed to the solve kernel in the last launch
int mpc_batch_qp_len(const mpc_batch *b) { return b ? b->ops->xqp_len : 0; }
int mpc_batch_scale_len(const mpc_batch *b) { return b ? b->ops->xsc_len : 0; }
int mpc_batch_get_qp(mpc_batch *b, double *h_qp) {
  if (!b || !h_qp) return fail(MPC_E_ARG, "mpc_batch_get_qp: bad argument");
  DeviceGuard guard_(b->device);
  return fetch_records(b, h_qp, nullptr);
}
int mpc_batch_get_scale(mpc_batch *b, double *h_sc) {
  if (!b || !h_sc) return fail(MPC_E_ARG, "mpc_batch_get_scale: bad argument");
  DeviceGuard guard_(b->device);
  return fetch_records(b, nullptr, h_sc);
}
int mpc_batch_get_profile(mpc_batch *b, long long *h_prof) {
  if (!b || !h_prof) return fail(MPC_E_ARG, "mpc_batch_get_profile: bad argument");
  DeviceGuard guard_(b->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_prof, b->d_prof, sizeof(long long) * (size_t)b->n * kProfLen, hipMemcpyDeviceToHost));
  return MPC_OK;
}
int mpc_batch_set_state(mpc_batch *b, const double *h_state) {
  if (!b || !h_state) return fail(MPC_E_ARG, "mpc_batch_set_state: bad argument");
  DeviceGuard guard_(b->device);
  HIP_TRY(hipDeviceSynchronize());      // (the null stream does not order against non-blocking streams: nothing may be in flight on the state ...
  HIP_TRY(hipMemcpy(b->d_state, h_state, state_bytes(b), hipMemcpyHostToDevice));
  HIP_TRY(clear_seed(b, nullptr));      // the working sets belonged to the state that was replaced
  HIP_TRY(hipDeviceSynchronize());      // ... and both are complete before the caller's next launch on any stream)
  return MPC_OK;
}

int mpc_device_clock(int device, int busy_ms, double *ghz, double *ms) {
  if (!ghz || busy_ms <= 0 || busy_ms > 1000) return fail(MPC_E_ARG, "mpc_device_clock: bad argument (1 .. 1000 ms)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(MPC_E_NODEVICE, "mpc_device_clock: no such HIP device");
  DeviceGuard guard_(device);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  const int blocks = 4 * prop.multiProcessorCount;       // one single-wave workgroup per SIMD
  struct Probe {      // released on every path out
    long long *d_out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st = nullptr;
    ~Probe() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      if (d_out) (void)hipFree(d_out);
      if (st) (void)hipStreamDestroy(st);
    }
  } pr;
  HIP_TRY(hipMalloc(&pr.d_out, sizeof(long long) * blocks));
  HIP_TRY(hipStreamCreateWithFlags(&pr.st, hipStreamNonBlocking));      // a stream of its own: the null stream would serialise with the caller's work
  HIP_TRY(hipEventCreate(&pr.e0)); HIP_TRY(hipEventCreate(&pr.e1));
  // 32 dependent multiply-adds per trip; the trip count was sized for ~10 k trips per ms at 2.1 GHz, and *ms reports what the launch took
  hipLaunchKernelGGL(clock_probe_kernel, dim3(blocks), dim3(64), 0, pr.st, pr.d_out, 2000);
  HIP_TRY(hipEventRecord(pr.e0, pr.st));
  hipLaunchKernelGGL(clock_probe_kernel, dim3(blocks), dim3(64), 0, pr.st, pr.d_out, 10000 * busy_ms);
  HIP_TRY(hipEventRecord(pr.e1, pr.st));
  HIP_TRY(hipEventSynchronize(pr.e1));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, pr.e0, pr.e1));
  long long cyc = 0;
  HIP_TRY(hipMemcpyAsync(&cyc, pr.d_out, sizeof cyc, hipMemcpyDeviceToHost, pr.st));
  HIP_TRY(hipStreamSynchronize(pr.st));
  *ghz = t > 0.f ? (double)cyc / ((double)t * 1e6) : 0.0;
  if (ms) *ms = t;
  return MPC_OK;
}

}  // extern "C"
