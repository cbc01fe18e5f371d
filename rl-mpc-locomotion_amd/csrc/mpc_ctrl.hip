// mpc_ctrl.hip -- the per-tick controller and control FSM of include/mpc_batch.h (mpc_ctrl_*): controller.h's arithmetic, one thread per robot
// or per leg before and after the solve.  The solver it owns and launches is mpc_batch.hip's; the observation rows of
// mpc_ctrl_policy_observations are mpc_policy.hip's launch (both through mpc_batch_internal.h).  Errors land in mpc_batch.hip's slot (mpc_last_error).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mpc_batch.h"
#include "controller.h"
#include "mpc_batch_internal.h"

using namespace mpc;
using mpchost::DeviceArray;
using mpchost::DeviceGuard;

namespace {

int fail(int code, const std::string &msg) { return batchint::set_error(code, msg); }      // (mpc_batch.hip's slot: one mpc_last_error for the three units)

constexpr int kWaitVm0 = 0x0F70;   // s_waitcnt vmcnt(0) (gfx9 encoding: vmcnt = simm16[3:0] | [15:14], expcnt [6:4] = 7, lgkmcnt [11:8] = 15: not waited for)

constexpr int kCtrlThreads = 64;   // one wave per workgroup: 4096 robots spread over 64 CUs, and the register cap is 512 (no spills)
dim3 ctrl_grid(int threads) { return dim3((unsigned)((threads + kCtrlThreads - 1) / kCtrlThreads)); }

__global__ __launch_bounds__(kCtrlThreads) void ctrl_init_kernel(int n, CtrlState *st, const RobotConst *rc, const int *robot_type, const int *gait_id) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) ctrl_init(st[r], rc[robot_type[r]], robot_type[r], gait_id[r]);
}
__global__ __launch_bounds__(kCtrlThreads) void ctrl_reset_kernel(int n, CtrlState *st, const RobotConst *rc, const int *ids, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int r = ids ? ids[i] : i;
  if (r >= 0 && r < n) ctrl_reset(st[r], rc[st[r].robot_type]);
}
__global__ void ctrl_set_gait_kernel(int n, CtrlState *st, const int *gait_id) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n && gait_id[r] >= 0 && gait_id[r] < kNumGaitIds) st[r].gait_id = gait_id[r];      // (an id outside the dispatch leaves the robot's gait as it is)
}
__global__ void ctrl_set_iter_kernel(int n, CtrlState *st, const int *iter) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) st[r].iter = iter[r];
}
// The controller's two halves of a tick with ONE LANE PER LEG (four lanes per robot, a hardware quad): a lane works on a private copy of
// the robot's state, does its own leg's part (controller.h ctrl_pre_legs / ctrl_pre_rest / ctrl_post with the leg range [leg, leg + 1)) and
// writes back its leg's fields; what concerns the whole robot every lane computes alike and lane 0 writes.  One lane per robot made
// the tick's 24 double-precision sines and cosines and its float16-emulating arithmetic one dependent chain (estimator + pre + post:
// 43 us per tick at 4096 robots, 10 % of a tick).
static_assert(sizeof(CtrlState) == 888, "CtrlState changed: every field must be stored by store_leg_fields or store_robot_fields");
// (HIST = false: all but the contact history, which the fused pre kernel's wave 2 writes)
template <bool HIST = true>
__device__ __forceinline__ void store_leg_fields(CtrlState &d, const CtrlState &s, int leg) {
  d.first_swing[leg] = s.first_swing[leg];
  d.swing_time_remaining[leg] = s.swing_time_remaining[leg];
  d.swing_times[leg] = s.swing_times[leg];
  d.contact_phase[leg] = s.contact_phase[leg];
  d.contact_states[leg] = s.contact_states[leg];
  d.swing_states[leg] = s.swing_states[leg];
  for (int c = 3 * leg; c < 3 * leg + 3; ++c) {
    d.f_ff[c] = s.f_ff[c]; d.p0[c] = s.p0[c]; d.pf[c] = s.pf[c]; d.tp[c] = s.tp[c]; d.tv[c] = s.tv[c];
    if constexpr (HIST) d.hist[c] = s.hist[c];
    d.q[c] = s.q[c]; d.qd[c] = s.qd[c]; d.p[c] = s.p[c]; d.v[c] = s.v[c]; d.foot_positions[c] = s.foot_positions[c]; d.pfoot[c] = s.pfoot[c];
  }
  for (int c = 9 * leg; c < 9 * leg + 9; ++c) d.J[c] = s.J[c];
}
__device__ __forceinline__ void store_robot_fields(CtrlState &d, const CtrlState &s) {
  d.iter = s.iter; d.first_run = s.first_run; d.pos_z = s.pos_z; d.posz_tick = s.posz_tick; d.do_solve = s.do_solve;
  for (int c = 0; c < 3; ++c) { d.normal[c] = s.normal[c]; d.vbody[c] = s.vbody[c]; }
}
// The four lanes of a quad each copy the whole st[r] and then store disjoint parts of it back.  Every lane's loads of st[r] must be
// complete before any lane of the quad stores: the quad sits in one wavefront (whose memory instructions issue in program order), so
// what is needed is that the COMPILER keeps every load above this point and every store below it, and that the loads' data has arrived
// (a lane may read a sibling's field late otherwise): wavefront-scope fence + s_waitcnt vmcnt(0) + a scheduling barrier.
static_assert(kCtrlThreads % 4 == 0, "a robot's four leg lanes must not straddle wavefronts");
__device__ __forceinline__ void quad_reads_done() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  __builtin_amdgcn_wave_barrier();
}
__global__ __launch_bounds__(kCtrlThreads) void ctrl_pre_kernel(int n, CtrlState *st, const RobotConst *rc, GaitTable gt, CtrlParams cp, const float *dof,
                                const float *est, const float *cmd, float *rec, int *active) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, r = t >> 2, leg = t & 3;
  if (r >= n) return;           // (n robots = 4 n threads: whole quads leave together)
  CtrlState s = st[r];
  const RobotConst &k = rc[s.robot_type];
  ctrl_pre_legs(s, k, dof + (size_t)r * 24, leg, leg + 1);
  // every lane needs the foot positions of all four legs (centre-of-mass height, ground-normal fit, the solver record)
  const int q0 = (int)__lane_id() & ~3;      // first lane of my quad (four consecutive lanes of one wavefront: kCtrlThreads % 4 == 0)
  float fp[12];
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float mine = c == 0 ? s.foot_positions[3 * leg] : (c == 1 ? s.foot_positions[3 * leg + 1] : s.foot_positions[3 * leg + 2]);
      fp[3 * l + c] = __shfl(mine, q0 + l);
    }
#pragma unroll
  for (int c = 0; c < 12; ++c) s.foot_positions[c] = fp[c];
  ctrl_pre_rest(s, k, gt, cp, est + (size_t)r * kEstLen, cmd + (size_t)r * 16, rec + (size_t)r * (56 + 4 * cp.horizon), leg, leg + 1, leg == 0);
  quad_reads_done();
  store_leg_fields(st[r], s, leg);
  if (leg == 0) {
    store_robot_fields(st[r], s);
    active[r] = s.do_solve;
  }
}
// controller.run's first half as ONE kernel of three concurrent wavefronts per 16 robots (mpc_ctrl_run; mpc_ctrl_step, whose caller brings the
// estimator outputs, keeps ctrl_pre_kernel):
//   wave 0   the leg quads of ctrl_pre_kernel: leg kinematics, then -- after the barrier -- everything of ctrl_pre_rest but the ground-normal fit;
//   wave 1   StateEstimator.update of the 16 robots, one lane each (estimator_kernel's work: no separate launch), handed over through LDS;
//   wave 2   the contact history and the ground-normal fit (gelsd43.h: ~20 us of one dependent float32 chain per robot) from the foot positions
//            wave 0 publishes, next to wave 0's foot placement / gait tables / record -- it writes the history, the normal and the record's normal.
// Every value is computed by the same code as in the two-kernel form (bit-identical results); what changes is that three dependent chains run side by side.
constexpr int kFusedRobots = 16;
// WITH_POST: a tick on which the host knows that no robot is due for its MPC update (mpc_ctrl::mirror_valid) has no solver launch between the two halves,
// so wave 0 goes straight on into ctrl_post (swing / stance commands, torque map) with the state it holds: one kernel per tick instead of two.
template <bool WITH_POST>
__global__ __launch_bounds__(3 * 64) void ctrl_pre_fused_kernel(int n, CtrlState *st, const RobotConst *rc, GaitTable gt, CtrlParams cp, const float *dof, const float *body,
                                                               float *est_out, const float *cmd, float *rec, int *active, float *torques) {
  __shared__ float sh_est[kFusedRobots][kEstLen];
  __shared__ float sh_fp[kFusedRobots][12];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r0 = blockIdx.x * kFusedRobots;
  if (wave == 1) {
    const int r = r0 + lane;
    if (lane < kFusedRobots && r < n) {
      const float nrm[3] = {st[r].normal[0], st[r].normal[1], st[r].normal[2]};       // the estimate of the previous tick (StateEstimator.py:88-92)
      float e[kEstLen];
      estimator_update(body + (size_t)r * 13, nrm, e);
      for (int k = 0; k < kEstLen; ++k) { sh_est[lane][k] = e[k]; est_out[(size_t)r * kEstLen + k] = e[k]; }
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);      // (like waves 0 and 2: this wave's loads of the state -- the previous tick's normal -- have arrived before wave 2 may overwrite it)
    __syncthreads();
    return;
  }
  if (wave == 2) {
    const int r = r0 + lane;
    const bool on = lane < kFusedRobots && r < n && !cp.flat_ground;
    float hist[12], cph[4], nrm[3];
    int first_run = 0, due = 0;
    double body_height = 0.0;
    if (on) {
      for (int k = 0; k < 12; ++k) hist[k] = st[r].hist[k];
      for (int k = 0; k < 4; ++k) cph[k] = st[r].contact_phase[k];
      first_run = st[r].first_run;
      due = ((st[r].iter + 1) % cp.iters_between_mpc) == 0;      // ctrl_pre_rest's do_solve of this tick: iterationCounter += 1, then the test (wave 0 stores the counter after the barrier)
      body_height = rc[st[r].robot_type].body_height;
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);      // (the loads of the state are complete before wave 0 may store to it: it stores after the barrier)
    __syncthreads();
    if (on) {
      float fp[12];
      for (int k = 0; k < 12; ++k) fp[k] = sh_fp[lane][k];
      if (first_run) contact_history_init(hist, fp, body_height);
      ground_normal_update(hist, nrm, cph, fp);
      for (int k = 0; k < 12; ++k) st[r].hist[k] = hist[k];
      for (int k = 0; k < 3; ++k) st[r].normal[k] = nrm[k];
      if (due)      // the solver record is written on MPC ticks only, like the two-kernel path's (controller.h ctrl_pre_rest)
        for (int k = 0; k < 3; ++k) rec[(size_t)r * (56 + 4 * cp.horizon) + IN_NRM + k] = nrm[k];
    }
    return;
  }
  const int rl = lane >> 2, leg = lane & 3, r = r0 + rl;
  const bool on = r < n;
  CtrlState s;
  if (on) {
    s = st[r];
    ctrl_pre_legs(s, rc[s.robot_type], dof + (size_t)r * 24, leg, leg + 1);
    for (int c = 0; c < 3; ++c) sh_fp[rl][3 * leg + c] = c == 0 ? s.foot_positions[3 * leg] : (c == 1 ? s.foot_positions[3 * leg + 1] : s.foot_positions[3 * leg + 2]);
  }
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  __syncthreads();
  if (!on) return;
  const RobotConst &k = rc[s.robot_type];
  float e[kEstLen];
  for (int c = 0; c < 12; ++c) s.foot_positions[c] = sh_fp[rl][c];
  for (int c = 0; c < kEstLen; ++c) e[c] = sh_est[rl][c];
  ctrl_pre_rest(s, k, gt, cp, e, cmd + (size_t)r * 16, rec + (size_t)r * (56 + 4 * cp.horizon), leg, leg + 1, leg == 0, false);
  if constexpr (WITH_POST) ctrl_post(s, k, nullptr, 0, torques + (size_t)r * 12, leg, leg + 1);      // (do_solve is 0 for every robot: no forces are read)
  quad_reads_done();
  if (cp.flat_ground) store_leg_fields(st[r], s, leg);      // (no fit on flat ground: the history is this wave's, set once at the first run)
  else store_leg_fields<false>(st[r], s, leg);
  if (leg == 0) {
    st[r].iter = s.iter; st[r].first_run = s.first_run; st[r].pos_z = s.pos_z; st[r].posz_tick = s.posz_tick; st[r].do_solve = s.do_solve;
    for (int c = 0; c < 3; ++c) st[r].vbody[c] = s.vbody[c];
    active[r] = s.do_solve;
  }
}
__global__ __launch_bounds__(kCtrlThreads) void estimator_kernel(int n, const CtrlState *st, const float *body, float *est) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float nrm[3] = {st[r].normal[0], st[r].normal[1], st[r].normal[2]};
  float e[kEstLen];
  estimator_update(body + (size_t)r * 13, nrm, e);
  for (int k = 0; k < kEstLen; ++k) est[(size_t)r * kEstLen + k] = e[k];
}
// Entering LOCOMOTION runs cMPC.initialize (FSM_State_Locomotion.py:32-42 -> ConvexMPCLocomotion.py:102-108): a NEW ConvexMpc object, i.e.
// x = y = z = 0, rho = 0.1 and an "osqp_setup" first call -- robot r's next solve is a cold one, from the empty working set (exact mode).
__device__ __forceinline__ void cold_start_robot(double *solver_state, int state_len, int *seed, int seed_len, int r) {
  for (int q = 0; q < state_len; ++q) solver_state[(size_t)r * state_len + q] = 0.0;
  for (int q = 0; q < seed_len; ++q) seed[(size_t)r * seed_len + q] = 0;
}
__global__ __launch_bounds__(kCtrlThreads) void fsm_init_kernel(int n, CtrlState *st, FsmState *fs, const RobotConst *rc, const int *mode, int op_mode, const int *ids, int k, int fresh,
                                                                double *solver_state, int state_len, int *seed, int seed_len) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int r = ids ? ids[i] : i;
  if (r < 0 || r >= n) return;
  CtrlState s = st[r];
  FsmState f = fs[r];
  if (fresh) fsm_init(f, mode[r], op_mode, s, rc[s.robot_type], 0.f);
  else fsm_reinit(f, mode[r], op_mode, s, rc[s.robot_type], f.last_rb22);
  // (fsm_tick clears entered_loco at its top, so it is consumed here)
  if (f.entered_loco && solver_state) cold_start_robot(solver_state, state_len, seed, seed_len, r);
  st[r] = s; fs[r] = f;
}
// RobotRunnerFSM.run up to the solver launch: fsm_tick, then ctrl_pre for the robots whose state runs the locomotion controller
__global__ __launch_bounds__(kCtrlThreads) void fsm_pre_kernel(int n, CtrlState *st, FsmState *fs, const RobotConst *rc, GaitTable gt, CtrlParams cp, FsmParams fp,
                               const float *dof, const float *body, const float *est, const float *cmd, const int *request, float *rec,
                               int *active, double *solver_state, int state_len, int *seed, int seed_len) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  CtrlState s = st[r];
  FsmState f = fs[r];
  fsm_tick(f, s, rc[s.robot_type], fp, dof + (size_t)r * 24, body + (size_t)r * 13, request[r]);
  if (f.entered_loco) cold_start_robot(solver_state, state_len, seed, seed_len, r);
  int act = 0;
  if (f.run_loco) {
    ctrl_pre(s, rc[s.robot_type], gt, cp, dof + (size_t)r * 24, est + (size_t)r * kEstLen, cmd + (size_t)r * 16, rec + (size_t)r * (56 + 4 * cp.horizon));
    act = s.do_solve;
  }
  active[r] = act;
  st[r] = s; fs[r] = f;
}
// Does the controller take the solver's forces?  OSQP branch: only OSQP_SOLVED returns a vector (mpc_osqp.cc:781-794; with the empty list the
// reference's Python raises at ConvexMPCLocomotion.py:186-187 -- here f_ff keeps its value).  qpOASES branch (exact mode): the vector comes
// back whatever the solver's status (:906-947) and ConvexMPCLocomotion.py:186-187 adopts it unconditionally: every status for which the
// library wrote the row (SOLVED, SOLVED_INACCURATE, MAX_ITER_REACHED: mpc_wrench.h store()) -- only NON_CVX writes nothing.
__device__ __forceinline__ int adopts_forces(int status, int exact) {
  return exact ? (status == kStSolved || status == kStSolvedInaccurate || status == kStMaxIter) : status == kStSolved;
}
__global__ __launch_bounds__(kCtrlThreads) void fsm_post_kernel(int n, CtrlState *st, const FsmState *fs, const RobotConst *rc, int horizon, const double *forces, const int *info,
                                int exact, float *torques) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (fs[r].run_loco) {
    CtrlState s = st[r];
    ctrl_post(s, rc[s.robot_type], forces + (size_t)r * 12 * horizon, adopts_forces(info[(size_t)r * kInfoLen + 1], exact), torques + (size_t)r * 12);
    st[r] = s;
  } else {
    fsm_joint_torques(fs[r], st[r], torques + (size_t)r * 12);
  }
}
__global__ __launch_bounds__(kCtrlThreads) void ctrl_post_kernel(int n, CtrlState *st, const RobotConst *rc, int horizon, const double *forces, const int *info,
                                 int exact, float *torques) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, r = t >> 2, leg = t & 3;      // one lane per leg (see ctrl_pre_kernel)
  if (r >= n) return;
  CtrlState s = st[r];
  ctrl_post(s, rc[s.robot_type], forces + (size_t)r * 12 * horizon, adopts_forces(info[(size_t)r * kInfoLen + 1], exact), torques + (size_t)r * 12, leg, leg + 1);
  quad_reads_done();
  store_leg_fields(st[r], s, leg);
}
__global__ void ctrl_estimate_kernel(int n, const CtrlState *st, const float *est_in, float *est_out, float *normal_out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (est_out) for (int k = 0; k < 18; ++k) est_out[18 * r + k] = est_in[18 * r + k];
  if (normal_out) for (int k = 0; k < 3; ++k) normal_out[3 * r + k] = st[r].normal[k];
}

}  // namespace

struct mpc_ctrl {
  int n = 0;
  int device = 0;                 // the solver's
  mpc_batch *solver = nullptr;    // owned: destroyed with the controller
  DeviceArray<CtrlState> d_state;
  DeviceArray<RobotConst> d_rc;
  DeviceArray<int> d_robot_type, d_gait, d_active, d_info;
  DeviceArray<float> d_rec, d_est;
  DeviceArray<double> d_forces;
  GaitTable gt;
  CtrlParams cp;
  std::vector<int> h_iter;        // host mirror of every robot's iterationCounter (deterministic outside the FSM): lets a tick
  bool mirror_valid = true;       // on which no robot is due for an MPC update skip the solver launches
  DeviceArray<FsmState> d_fsm;    // control FSM (allocated by mpc_ctrl_fsm_init)
  DeviceArray<int> d_fsm_mode;    // per-robot control mode of the last (re)initialisation
  FsmParams fp{};
  int fsm_op_mode = kOpNormal;

  ~mpc_ctrl() { mpc_batch_destroy(solver); }
};

namespace {

// one tick: the pre kernel (with the caller's estimator outputs, or -- d_est null -- with StateEstimator.update from d_body fused in), the solver
// launch when a robot is due, the post kernel
int ctrl_tick(const char *who, mpc_ctrl *c, const float *d_dof, const float *d_est, const float *d_body, const float *d_cmd, float *d_torques, void *stream) {
  if (!c || !d_dof || !(d_est || d_body) || !d_cmd || !d_torques) return fail(MPC_E_ARG, std::string(who) + ": bad argument");
  DeviceGuard guard_(c->solver->device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n = c->n;
  const dim3 legs = ctrl_grid(4 * n), fused((n + kFusedRobots - 1) / kFusedRobots);      // (ctrl_pre / ctrl_post: one lane per leg)
  bool any_due = true;
  if (c->mirror_valid) {   // ConvexMPCLocomotion.run: iterationCounter += 1, MPC update when it is a multiple of iterationsBetweenMPC
    if ((int)c->h_iter.size() != n) c->h_iter.assign(n, 0);
    any_due = false;
    for (int r = 0; r < n; ++r) any_due |= (++c->h_iter[r] % c->cp.iters_between_mpc) == 0;
  }
  if (d_est) hipLaunchKernelGGL(ctrl_pre_kernel, legs, dim3(kCtrlThreads), 0, st, n, c->d_state, c->d_rc, c->gt, c->cp, d_dof, d_est, d_cmd, c->d_rec, c->d_active);
  else if (!any_due) {      // nobody is due (host mirror): the whole tick is one kernel
    hipLaunchKernelGGL(ctrl_pre_fused_kernel<true>, fused, dim3(3 * 64), 0, st, n, c->d_state, c->d_rc, c->gt, c->cp, d_dof, d_body, c->d_est, d_cmd, c->d_rec, c->d_active, d_torques);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
  }
  else hipLaunchKernelGGL(ctrl_pre_fused_kernel<false>, fused, dim3(3 * 64), 0, st, n, c->d_state, c->d_rc, c->gt, c->cp, d_dof, d_body, c->d_est, d_cmd, c->d_rec, c->d_active,
                          (float *)nullptr);
  HIP_TRY(hipGetLastError());
  mpc_batch *b = c->solver;
  if (any_due) {
    int rc = batchint::launch(b, c->d_rec, c->d_forces, c->d_info, c->d_active, st);
    if (rc != MPC_OK) return rc;
  }
  hipLaunchKernelGGL(ctrl_post_kernel, legs, dim3(kCtrlThreads), 0, st, n, c->d_state, c->d_rc, c->cp.horizon, c->d_forces, c->d_info, b->exact, d_torques);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int run_fsm(mpc_ctrl *c, const float *d_dof, const float *d_body, const float *d_cmd, const int *d_request, float *d_torques, void *stream, bool estimated) {
  if (!c || !d_dof || !d_body || !d_cmd || !d_request || !d_torques) return fail(MPC_E_ARG, "mpc_ctrl_run_fsm: bad argument");
  DeviceGuard guard_(c->solver->device);
  if (!c->d_fsm) return fail(MPC_E_ARG, "mpc_ctrl_run_fsm: call mpc_ctrl_fsm_init first");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n = c->n;
  const dim3 blocks = ctrl_grid(n);
  mpc_batch *b = c->solver;
  if (!estimated) hipLaunchKernelGGL(estimator_kernel, blocks, dim3(kCtrlThreads), 0, st, n, c->d_state, d_body, c->d_est);
  hipLaunchKernelGGL(fsm_pre_kernel, blocks, dim3(kCtrlThreads), 0, st, n, c->d_state, c->d_fsm, c->d_rc, c->gt, c->cp, c->fp, d_dof, d_body, c->d_est, d_cmd,
                     d_request, c->d_rec, c->d_active, b->d_state, b->state_len, b->d_seed, batchint::seed_len(b));
  HIP_TRY(hipGetLastError());
  int rc = batchint::launch(b, c->d_rec, c->d_forces, c->d_info, c->d_active, st);
  if (rc != MPC_OK) return rc;
  hipLaunchKernelGGL(fsm_post_kernel, blocks, dim3(kCtrlThreads), 0, st, n, c->d_state, c->d_fsm, c->d_rc, c->cp.horizon, c->d_forces, c->d_info, b->exact, d_torques);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

// mpc_ctrl_reset, _device: the solver's robots as new ConvexMpc objects (cold: ConvexMPCLocomotion.py:102-108), then the controller's own reset
int reset_robots(mpc_ctrl *c, const int *ids, int k, mpchost::Ids where, void *stream) {
  const int rc = where == mpchost::Ids::host ? mpc_batch_reset(c->solver, ids, k, stream) : mpc_batch_reset_device(c->solver, ids, k, stream);
  if (rc != MPC_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const auto launch = [&](const int *d_ids, int cnt) {
    hipLaunchKernelGGL(ctrl_reset_kernel, ctrl_grid(cnt), dim3(kCtrlThreads), 0, st, c->n, c->d_state, c->d_rc, d_ids, cnt);
  };
  HIP_TRY(mpchost::launch_over_ids(ids, k, c->n, where, st, launch));
  return MPC_OK;
}

// mpc_ctrl_fsm_reset, _device: the FSM of the listed robots starts again in its mode of d_fsm_mode; one that enters LOCOMOTION gets a cold solver
int fsm_reinit_robots(mpc_ctrl *c, const int *ids, int k, mpchost::Ids where, hipStream_t st) {
  mpc_batch *b = c->solver;
  const auto launch = [&](const int *d_ids, int cnt) {
    hipLaunchKernelGGL(fsm_init_kernel, ctrl_grid(cnt), dim3(kCtrlThreads), 0, st, c->n, c->d_state, c->d_fsm, c->d_rc, c->d_fsm_mode, c->fsm_op_mode, d_ids, cnt, 0, b->d_state,
                       b->state_len, b->d_seed, batchint::seed_len(b));
  };
  HIP_TRY(mpchost::launch_over_ids(ids, k, c->n, where, st, launch));
  return MPC_OK;
}

int check_control_modes(const char *who, const mpc_ctrl *c, const int *control_mode) {
  for (int r = 0; r < c->n; ++r)
    if (control_mode[r] != kFsmPassive && control_mode[r] != kFsmLocomotion && control_mode[r] != kFsmRecoveryStand)
      return fail(MPC_E_ARG, std::string(who) + ": control mode must be 0 (PASSIVE), 4 (LOCOMOTION) or 6 (RECOVERY_STAND)");
  return MPC_OK;
}

}  // namespace

extern "C" {

void mpc_ctrl_destroy(mpc_ctrl *c) { mpchost::destroy_handle(c); }

int mpc_ctrl_create(mpc_ctrl **out, int n, int horizon, double controller_dt, int iters_between_mpc, double alpha, int flat_ground,
                    const int *robot_type, const int *gait_id, int n_types, const double *robot_table, const int *gait_off,
                    const int *gait_dur) {
  if (!out || n <= 0 || !robot_type || !gait_id || n_types <= 0 || !robot_table || !gait_off || !gait_dur || iters_between_mpc <= 0)
    return fail(MPC_E_ARG, "mpc_ctrl_create: bad argument");
  std::vector<double> mass(n), inertia((size_t)n * 9, 0.0);
  for (int r = 0; r < n; ++r) {
    if (robot_type[r] < 0 || robot_type[r] >= n_types || gait_id[r] < 0 || gait_id[r] >= kNumGaitIds) return fail(MPC_E_ARG, "mpc_ctrl_create: robot_type / gait_id out of range");
    const double *row = robot_table + 25 * robot_type[r];
    mass[r] = row[6];
    inertia[9 * (size_t)r] = row[7]; inertia[9 * (size_t)r + 4] = row[8]; inertia[9 * (size_t)r + 8] = row[9];
  }
  mpc_ctrl *c = new mpc_ctrl();
  c->n = n;
  const double dt_mpc = controller_dt * iters_between_mpc;
  int rc0 = mpc_batch_create(&c->solver, n, horizon, dt_mpc, alpha, mass.data(), inertia.data());
  if (rc0 != MPC_OK) { delete c; return rc0; }
  c->device = c->solver->device;
  c->cp = CtrlParams{controller_dt, iters_between_mpc, dt_mpc, horizon, flat_ground};
  c->gt.n_seg = horizon;
  for (int g = 0; g < kNumGaitIds; ++g)
    for (int j = 0; j < 4; ++j) { c->gt.offsets[g][j] = (float)gait_off[4 * g + j]; c->gt.durations[g][j] = (float)gait_dur[4 * g + j]; }
  std::vector<RobotConst> rcs(n_types);
  for (int t = 0; t < n_types; ++t) {
    const double *row = robot_table + 25 * t;
    rcs[t].abad = row[0]; rcs[t].hip = row[1]; rcs[t].knee = row[2];
    for (int k = 0; k < 3; ++k) rcs[t].hiploc[k] = (float)row[3 + k];
    rcs[t].body_height = row[10]; rcs[t].mu = (float)row[11];
    for (int k = 0; k < 13; ++k) rcs[t].weights[k] = (float)row[12 + k];
  }
  const size_t N = (size_t)n, inlen = 56 + 4 * (size_t)horizon;
  hipError_t e;
  if ((e = c->d_state.alloc(N)) != hipSuccess || (e = c->d_rc.alloc_copy(rcs.data(), (size_t)n_types)) != hipSuccess ||
      (e = c->d_robot_type.alloc_copy(robot_type, N)) != hipSuccess || (e = c->d_gait.alloc_copy(gait_id, N)) != hipSuccess ||
      (e = c->d_active.alloc(N)) != hipSuccess || (e = c->d_info.alloc_zero(N * kInfoLen)) != hipSuccess ||
      (e = c->d_rec.alloc_zero(N * inlen)) != hipSuccess || (e = c->d_est.alloc(N * kEstLen)) != hipSuccess ||
      (e = c->d_forces.alloc_zero(N * 12 * horizon)) != hipSuccess) {
    mpc_ctrl_destroy(c);
    return fail(MPC_E_HIP, std::string("mpc_ctrl_create: ") + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(ctrl_init_kernel, ctrl_grid(n), dim3(kCtrlThreads), 0, nullptr, n, c->d_state, c->d_rc, c->d_robot_type, c->d_gait);
  if ((e = hipDeviceSynchronize()) != hipSuccess) { mpc_ctrl_destroy(c); return fail(MPC_E_HIP, std::string("mpc_ctrl_create: ") + hipGetErrorString(e)); }
  *out = c;
  return MPC_OK;
}

int mpc_ctrl_step(mpc_ctrl *c, const float *d_dof, const float *d_est, const float *d_cmd, float *d_torques, void *stream) {
  return ctrl_tick("mpc_ctrl_step", c, d_dof, d_est, nullptr, d_cmd, d_torques, stream);
}
int mpc_ctrl_run(mpc_ctrl *c, const float *d_dof, const float *d_body, const float *d_cmd, float *d_torques, void *stream) {
  return ctrl_tick("mpc_ctrl_run", c, d_dof, nullptr, d_body, d_cmd, d_torques, stream);
}

int mpc_ctrl_reset(mpc_ctrl *c, const int *ids, int k, void *stream) {
  if (!c) return fail(MPC_E_ARG, "mpc_ctrl_reset: bad argument");
  DeviceGuard guard_(c->solver->device);
  if (!ids) c->h_iter.assign(c->n, 0);
  else for (int i = 0; i < k; ++i) if (ids[i] >= 0 && ids[i] < c->n && (int)c->h_iter.size() == c->n) c->h_iter[ids[i]] = 0;
  return reset_robots(c, ids, k, mpchost::Ids::host, stream);
}

int mpc_ctrl_reset_device(mpc_ctrl *c, const int *d_ids, int k, void *stream) {
  if (!c || !d_ids || k < 0) return fail(MPC_E_ARG, "mpc_ctrl_reset_device: bad argument");
  DeviceGuard guard_(c->solver->device);
  if (k == 0) return MPC_OK;
  c->mirror_valid = false;     // the host copy of the MPC counters cannot follow ids it never sees: launch the solver on every tick (active mask)
  return reset_robots(c, d_ids, k, mpchost::Ids::device, stream);
}

int mpc_ctrl_set_solver(mpc_ctrl *c, int solver) {
  if (!c) return fail(MPC_E_ARG, "mpc_ctrl_set_solver: bad argument");
  return mpc_batch_set_solver(c->solver, solver);
}

int mpc_ctrl_set_gait(mpc_ctrl *c, const int *gait_id, void *stream) {
  if (!c || !gait_id) return fail(MPC_E_ARG, "mpc_ctrl_set_gait: bad argument");
  DeviceGuard guard_(c->solver->device);
  for (int r = 0; r < c->n; ++r) if (gait_id[r] < 0 || gait_id[r] >= kNumGaitIds) return fail(MPC_E_ARG, "mpc_ctrl_set_gait: gait id out of range");
  HIP_TRY(hipMemcpyAsync(c->d_gait, gait_id, sizeof(int) * c->n, hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)));
  return mpc_ctrl_set_gait_device(c, c->d_gait, stream);
}

int mpc_ctrl_set_gait_device(mpc_ctrl *c, const int *d_gait_id, void *stream) {
  if (!c || !d_gait_id) return fail(MPC_E_ARG, "mpc_ctrl_set_gait_device: bad argument");
  DeviceGuard guard_(c->solver->device);
  hipLaunchKernelGGL(ctrl_set_gait_kernel, ctrl_grid(c->n), dim3(kCtrlThreads), 0, reinterpret_cast<hipStream_t>(stream), c->n, c->d_state, d_gait_id);
  HIP_TRY(hipGetLastError());
  return MPC_OK;      // (stream-ordered: no host round trip, no synchronisation)
}

int mpc_ctrl_set_iteration(mpc_ctrl *c, const int *iteration, void *stream) {
  if (!c || !iteration) return fail(MPC_E_ARG, "mpc_ctrl_set_iteration: bad argument");
  DeviceGuard guard_(c->solver->device);
  for (int r = 0; r < c->n; ++r) if (iteration[r] < 0) return fail(MPC_E_ARG, "mpc_ctrl_set_iteration: negative counter");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(c->d_active, iteration, sizeof(int) * c->n, hipMemcpyHostToDevice, st));   // (d_active is rewritten by the next tick's ctrl_pre)
  hipLaunchKernelGGL(ctrl_set_iter_kernel, ctrl_grid(c->n), dim3(kCtrlThreads), 0, st, c->n, c->d_state, c->d_active);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));      // `iteration` is a host buffer
  c->h_iter.assign(iteration, iteration + c->n);
  return MPC_OK;
}

mpc_batch *mpc_ctrl_solver(mpc_ctrl *c) { return c ? c->solver : nullptr; }

int mpc_ctrl_solver_forces(mpc_ctrl *c, double *h_forces) {
  if (!c || !h_forces) return fail(MPC_E_ARG, "mpc_ctrl_solver_forces: bad argument");
  DeviceGuard guard_(c->solver->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_forces, c->d_forces, sizeof(double) * (size_t)c->n * 12 * c->cp.horizon, hipMemcpyDeviceToHost));
  return MPC_OK;
}

int mpc_ctrl_fsm_init(mpc_ctrl *c, const int *control_mode, int operating_mode, int check_safety, void *stream) {
  if (!c || !control_mode || (operating_mode != kOpTest && operating_mode != kOpNormal)) return fail(MPC_E_ARG, "mpc_ctrl_fsm_init: bad argument");
  DeviceGuard guard_(c->solver->device);
  if (int rc = check_control_modes("mpc_ctrl_fsm_init", c, control_mode)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!c->d_fsm) {
    HIP_TRY(c->d_fsm.alloc((size_t)c->n));
    HIP_TRY(c->d_fsm_mode.alloc((size_t)c->n));
  }
  c->mirror_valid = false;       // from here on the device decides which robots run the locomotion controller
  c->fp = fsm_params(c->cp.dt, check_safety);
  c->fsm_op_mode = operating_mode;
  HIP_TRY(hipMemcpyAsync(c->d_fsm_mode, control_mode, sizeof(int) * c->n, hipMemcpyHostToDevice, st));
  int rc = mpc_batch_reset(c->solver, nullptr, 0, stream);   // RobotRunnerFSM.init builds fresh objects
  if (rc != MPC_OK) return rc;
  hipLaunchKernelGGL(ctrl_init_kernel, ctrl_grid(c->n), dim3(kCtrlThreads), 0, st, c->n, c->d_state, c->d_rc, c->d_robot_type, c->d_gait);
  hipLaunchKernelGGL(fsm_init_kernel, ctrl_grid(c->n), dim3(kCtrlThreads), 0, st, c->n, c->d_state, c->d_fsm, c->d_rc, c->d_fsm_mode, operating_mode,
                     (const int *)nullptr, c->n, 1, (double *)nullptr, 0, (int *)nullptr, 0);   // (the whole solver was reset above)
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));                          // control_mode is a host buffer
  return MPC_OK;
}

int mpc_ctrl_fsm_reset(mpc_ctrl *c, const int *ids, int k, const int *control_mode, void *stream) {
  if (!c || !c->d_fsm || (ids && k < 0)) return fail(MPC_E_ARG, "mpc_ctrl_fsm_reset: bad argument (mpc_ctrl_fsm_init first)");
  DeviceGuard guard_(c->solver->device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (control_mode) {   // [n] entries, like mpc_ctrl_fsm_init
    if (int rc = check_control_modes("mpc_ctrl_fsm_reset", c, control_mode)) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_fsm_mode, control_mode, sizeof(int) * c->n, hipMemcpyHostToDevice, st));
  }
  if (int rc = fsm_reinit_robots(c, ids, k, mpchost::Ids::host, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));      // ids and control_mode are host buffers
  return MPC_OK;
}

int mpc_ctrl_fsm_reset_device(mpc_ctrl *c, const int *d_ids, int k, void *stream) {
  if (!c || !c->d_fsm || !d_ids || k < 0) return fail(MPC_E_ARG, "mpc_ctrl_fsm_reset_device: bad argument (mpc_ctrl_fsm_init first)");
  DeviceGuard guard_(c->solver->device);
  return fsm_reinit_robots(c, d_ids, k, mpchost::Ids::device, reinterpret_cast<hipStream_t>(stream));      // (stream-ordered: no host round trip, no synchronisation)
}

int mpc_ctrl_run_fsm(mpc_ctrl *c, const float *d_dof, const float *d_body, const float *d_cmd, const int *d_request, float *d_torques, void *stream) {
  return run_fsm(c, d_dof, d_body, d_cmd, d_request, d_torques, stream, false);
}
int mpc_ctrl_run_fsm_estimated(mpc_ctrl *c, const float *d_dof, const float *d_body, const float *d_cmd, const int *d_request, float *d_torques, void *stream) {
  return run_fsm(c, d_dof, d_body, d_cmd, d_request, d_torques, stream, true);
}

int mpc_ctrl_fsm_state(mpc_ctrl *c, int *h_out) {
  if (!c || !c->d_fsm || !h_out) return fail(MPC_E_ARG, "mpc_ctrl_fsm_state: bad argument");
  DeviceGuard guard_(c->solver->device);
  std::vector<FsmState> h(c->n);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h.data(), c->d_fsm, sizeof(FsmState) * c->n, hipMemcpyDeviceToHost));
  for (int r = 0; r < c->n; ++r) { h_out[4 * r] = h[r].cur; h_out[4 * r + 1] = h[r].op_mode; h_out[4 * r + 2] = h[r].rs_flag; h_out[4 * r + 3] = h[r].unsafe; }
  return MPC_OK;
}

int mpc_ctrl_solver_record(mpc_ctrl *c, float *h_rec) {
  if (!c || !h_rec) return fail(MPC_E_ARG, "mpc_ctrl_solver_record: bad argument");
  DeviceGuard guard_(c->solver->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_rec, c->d_rec, sizeof(float) * (size_t)c->n * (56 + 4 * (size_t)c->cp.horizon), hipMemcpyDeviceToHost));
  return MPC_OK;
}

int mpc_ctrl_solver_info(mpc_ctrl *c, int *h_info) {
  if (!c || !h_info) return fail(MPC_E_ARG, "mpc_ctrl_solver_info: bad argument");
  DeviceGuard guard_(c->solver->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_info, c->d_info, sizeof(int) * (size_t)c->n * kInfoLen, hipMemcpyDeviceToHost));
  return MPC_OK;
}

int mpc_ctrl_policy_observations(mpc_ctrl *c, const float *d_dof, const float *d_cmd3, const float *d_prev_actions, const float *scales4, float *d_obs, void *stream) {
  if (!c || !d_dof || !d_cmd3 || !d_prev_actions || !scales4 || !d_obs) return fail(MPC_E_ARG, "mpc_ctrl_policy_observations: bad argument");
  DeviceGuard guard_(c->solver->device);
  static_assert(sizeof(CtrlState) % sizeof(float) == 0, "the state records are read with a float stride");
  HIP_TRY(batchint::launch_observations(c->n, d_dof, c->d_est, &c->d_state[0].normal[0], (int)(sizeof(CtrlState) / sizeof(float)), d_cmd3, d_prev_actions, scales4, d_obs,
                                         (hipStream_t)stream));
  return MPC_OK;
}

int mpc_ctrl_update_estimate(mpc_ctrl *c, const float *d_body, void *stream) {
  if (!c || !d_body) return fail(MPC_E_ARG, "mpc_ctrl_update_estimate: bad argument");
  DeviceGuard guard_(c->solver->device);
  hipLaunchKernelGGL(estimator_kernel, ctrl_grid(c->n), dim3(kCtrlThreads), 0, (hipStream_t)stream, c->n, c->d_state, d_body, c->d_est);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

int mpc_ctrl_estimate(mpc_ctrl *c, float *d_est, float *d_ground_normal, void *stream) {
  if (!c || (!d_est && !d_ground_normal)) return fail(MPC_E_ARG, "mpc_ctrl_estimate: bad argument");
  DeviceGuard guard_(c->solver->device);
  hipLaunchKernelGGL(ctrl_estimate_kernel, ctrl_grid(c->n), dim3(kCtrlThreads), 0, (hipStream_t)stream, c->n, c->d_state, c->d_est, d_est, d_ground_normal);
  HIP_TRY(hipGetLastError());
  return MPC_OK;
}

}  // extern "C"
