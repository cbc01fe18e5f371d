// mpc_batch_internal.h -- what the three units of include/mpc_batch.h may know of each other.  Of an mpc_batch: the handle, the solver launch on
// a record with an active mask, the per-robot cold-start buffers and the error slot behind mpc_last_error.  mpc_batch.hip owns the handle and
// every launch of the per-horizon kernel sets; mpc_ctrl.hip's ticks launch the solver between their two halves, and its FSM kernels make single
// robots' solvers cold (a new ConvexMpc object).  Of mpc_policy.hip: the launch of its observations_kernel, which mpc_ctrl_policy_observations
// runs on the controller's own estimate and state records.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "mpc_horizon.h"
#include "mpc_host.h"

constexpr int kTimingRing = 64;

struct mpc_batch {
  int n = 0, h = 0;
  const mpc::HorizonOps *ops = nullptr;   // the kernel set of this planning horizon (mpc_horizon.h)
  int state_len = 0;
  mpchost::DeviceArray<mpc::RobotModel> d_models;
  mpchost::DeviceArray<double> d_state, d_qp, d_sc;   // warm start, QP record (q, l, u, cone, wrench form of P), scale record
  mpchost::DeviceArray<int> d_info;       // used when the caller passes no info buffer
  mpchost::DeviceArray<long long> d_prof; // per-robot section cycle counts of the last solve
  mpchost::DeviceArray<int> d_order;      // job list of the solve kernel: the launch's active robots, longest expected solve first (order_block, written by the prep launch)
  mpchost::DeviceArray<int> d_sched;      // [kSchedLen] job counters of the launch; d_ready [n]: polish entries (mpc_solve_jobs_kernel)
  mpchost::DeviceArray<int> d_ready;
  mpchost::DeviceArray<int> d_seed;       // [n, seed_len] exact mode: the working set each robot's previous call ended on (seeds the active-set method; MPC_EXACT_WARM=0: never)
  bool warm_sets = true;
  bool f32_seed = false;         // MPC_EXACT_F32_SEED=1 (tuning hook, default off): the exact mode's seed comes from the float32 search of the call (mpc_exact32.h)
  int job_slots = 0;             // wave slots of the device for the persistent job kernel (0: one workgroup per robot)
  bool timing = false;           // mpc_batch_enable_timing: HIP events around the two kernels of each launch
  hipEvent_t ev[kTimingRing][3];
  long long launches = 0;
  mpchost::DeviceArray<float> d_host_in;      // staging for mpc_batch_solve_host, allocated on its first call
  mpchost::DeviceArray<double> d_host_in64;   // ... and mpc_batch_solve_host_f64
  mpchost::DeviceArray<double> d_host_f;
  mpchost::DeviceArray<unsigned char> d_hist; // [n][kOrderHistory] cycles / 16384 of the last solves (order_block's sort key is their maximum)
  unsigned long long order_launches = 0;
  int device = 0;                // the HIP device the handle was created on: every entry point runs under a DeviceGuard for it
  int exact = 0;                 // mpc_batch_set_solver: 1 = the QP's exact optimum (the reference's qpOASES branch), cold on every call
  int max_iter = mpc::kMaxIter;  // mpc_batch_set_max_iter: OSQP's max_iter setting (OSQP mode)
  long long bytes = 0;

  ~mpc_batch() {
    if (timing) for (auto &e3 : ev) for (auto &e : e3) (void)hipEventDestroy(e);
  }
};

namespace batchint {

// A robot's cold start is zeros in its state_len doubles of d_state and its seed_len ints of d_seed (a new ConvexMpc object: x = y = z = 0, no
// working set).  mpc_batch.hip's reset_kernel and mpc_ctrl.hip's FSM kernels write them robot by robot.
inline int seed_len(const mpc_batch *b) { return 4 * b->h; }

// one solver launch on the float32 records d_rec of b's robots whose d_active entry is set (null: all of them)
int launch(mpc_batch *b, const float *d_rec, double *d_forces, int *d_info, const int *d_active, hipStream_t stream);

// the error text of mpc_last_error (thread-local, owned by mpc_batch.hip); returns code
int set_error(int code, const std::string &msg);

// WeightPolicy.compute_observations for n robots (mpc_policy.hip); the ground normal of robot r is d_normal[r * normal_stride + 0 .. 2].  The
// caller has set the device and checked the pointers.
hipError_t launch_observations(int n, const float *d_dof, const float *d_est, const float *d_normal, int normal_stride, const float *d_cmd3,
                               const float *d_prev_actions, const float *scales4, float *d_obs, hipStream_t stream);

}  // namespace batchint
