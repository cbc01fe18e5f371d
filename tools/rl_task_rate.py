"""What the RL task's post-physics half costs: BatchedRLTask.step for 4096 Aliengo robots trotting, h = 10, against the loop of
tools/closed_loop_rate.py (controller + toy plant alone) and against the same half written as the plain torch composition with its
`reset_buf.nonzero()`.  Per tick, from HIP events inside the running loop (median over the ticks): the controller step, the toy plant's step, the
`begin` kernel, the device resets, the `finish` kernel; and the torch composition of begin + resets + finish.  Per loop, from the host clock around
blocks of ticks that end in a synchronise (median of the blocks, the three loops alternating): robot-ticks / s.  The shader clock is recorded as
bench.py --full records it (device_state).
    python tools/rl_task_rate.py [--ticks 100] [--blocks 7] [--out profiles/r08_rl_task.json]
The kernel-trace stats of the same step: rocprofv3 --kernel-trace --stats ... -- python tools/rl_task_rate.py --ticks 50 --quick"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_mpc_locomotion_amd  # noqa: E402,F401
from rl_mpc_locomotion_amd import _lib  # noqa: E402
from rl_mpc_locomotion_amd.rl_task import REWARD_TERMS, BatchedRLTask, TaskConfig  # noqa: E402

TROT = 0
# the closed-loop golden's trot command (0.5 m/s ahead) as a one-point command range; zero actions are its MPC weights (5 5 5 50 50 50 1 ...)
CFG = dict(command_x_range=(0.5, 0.5), command_y_range=(0.0, 0.0), command_yaw_range=(0.0, 0.0))


def make(n, dev):
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    task = BatchedRLTask([0] * n, [TROT] * n, cfg=TaskConfig(**CFG), horizon=10, yaw0=yaw, flat_ground=True, device=dev)
    task.reset()
    return task


def torch_half(task, actions, torques):
    """begin + resets + finish as the torch composition of vec_task.py:326-337 and aliengo.py:273-349, :357-444 on the same buffers (the toy's `fell`
    flag as base contact, no knee or hip contacts), `nonzero` and its host round trip included."""
    cfg, sim = task.cfg, task.sim
    rs = dict(zip(REWARD_TERMS, cfg.reward_scales()))
    task.timeout_buf[:] = torch.where(task.progress_buf >= cfg.max_episode_length - 1, torch.ones_like(task.timeout_buf), torch.zeros_like(task.timeout_buf))
    task.progress_buf += 1
    env_ids = task.reset_buf.nonzero(as_tuple=False).squeeze(-1)
    if len(env_ids) > 0:
        task.bridge.ctl.reset(env_ids)
        sim.reset_idx(env_ids)
        for a, (lo, hi) in enumerate((cfg.command_x_range, cfg.command_y_range, cfg.command_yaw_range)):
            task.commands[env_ids, a] = lo + (hi - lo) * torch.rand(len(env_ids), device=task.device)
        task.progress_buf[env_ids] = 0
        task.reset_buf[env_ids] = 1
    _, fell = sim.flags()
    root, commands = sim.root_states, task.commands

    def qri(q, v):
        q_w, q_vec = q[:, -1], q[:, :3]
        return v * (2.0 * q_w ** 2 - 1.0).unsqueeze(-1) - torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0 + q_vec * (q_vec * v).sum(-1, keepdim=True) * 2.0
    lin, ang = qri(root[:, 3:7], root[:, 7:10]), qri(root[:, 3:7], root[:, 10:13])
    dofv = sim.dof_state.view(task.n, 12, 2)
    default = torch.tensor(cfg.default_dof_pos, dtype=torch.float32, device=task.device)
    scaled = commands * torch.tensor([cfg.lin_vel_scale, cfg.lin_vel_scale, cfg.ang_vel_scale], device=task.device)
    obs = torch.cat((root[:, 0:3], lin * cfg.lin_vel_scale, ang * cfg.ang_vel_scale, scaled, (dofv[..., 0] - default) * cfg.dof_pos_scale,
                     dofv[..., 1] * cfg.dof_vel_scale, actions), dim=-1)
    task.obs_buf[:] = torch.clamp(obs, -cfg.clip_observations, cfg.clip_observations)
    lin_err = torch.sum(torch.square(commands[:, :2] - lin[:, :2]), dim=1)
    ang_err = torch.square(commands[:, 2] - ang[:, 2])
    total = (torch.exp(-lin_err / 0.25) * rs["lin_vel_xy"] + torch.square(lin[:, 2]) * rs["lin_vel_z"] + torch.sum(torch.square(ang[:, :2]), dim=1) * rs["ang_vel_xy"]
             + torch.exp(-ang_err / 0.25) * rs["ang_vel_z"] + torch.sum(torch.square(torques), dim=1) * rs["torque"])
    task.rew_buf[:] = torch.clip(total, 0., None)
    task.reset_buf[:] = fell | (task.progress_buf > cfg.max_episode_length)


def tick_fused(task, actions, ev=None):
    """BatchedRLTask.step's statements, with events between its parts"""
    sim, t = task.sim, task.task
    rec = (lambda i: ev[i].record()) if ev is not None else (lambda i: None)
    rec(0)
    tau = task.bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, task.commands)
    rec(1)
    sim.step(tau)
    rec(2)
    ids = t.begin()
    rec(3)
    task.bridge.ctl.reset(ids)
    sim.reset_idx(ids)
    _, fell = sim.flags()
    rec(4)
    t.finish(sim.root_states, sim.dof_state, actions, tau, fell=fell)
    rec(5)


def tick_torch(task, actions, ev=None):
    sim = task.sim
    tau = task.bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, task.commands)
    sim.step(tau)
    if ev is not None:
        ev[0].record()
    torch_half(task, actions, tau)
    if ev is not None:
        ev[1].record()


class Bare:
    """tools/closed_loop_rate.py's loop: controller + plant, no task (and so no device reset: on the ticks on which no robot is due for its MPC
    update the controller is one kernel)"""

    def __init__(self, n, dev):
        from rl_mpc_locomotion_amd.locomotion import BatchedLocomotion
        from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
        self.n = n
        self.sim = BatchedToySim([0] * n, yaw0=np.random.default_rng(0).uniform(-np.pi, np.pi, n), device=dev)
        self.ctl = BatchedLocomotion([0] * n, [TROT] * n, horizon=10, flat_ground=True, device=dev)
        self.cmd = torch.tensor([0.5, 0.0, 0.0, 5, 5, 5, 50, 50, 50, 1, 1, 1, 1, 1, 1, 0], dtype=torch.float32, device=dev).repeat(n, 1).contiguous()

    def tick(self):
        self.sim.step(self.ctl.run(self.sim.dof_state.view(self.n, 12, 2), self.sim.root_states, self.cmd))


def med(x):
    return float(np.median(x))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=100, help="ticks per block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--quick", action="store_true", help="one block of BatchedRLTask.step only (for a kernel trace)")
    ap.add_argument("--out")
    args = ap.parse_args()
    dev, n = "cuda:0", args.robots
    actions = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    if args.quick:
        task = make(n, dev)
        for _ in range(args.ticks):
            task.step(actions)
        torch.cuda.synchronize()
        sys.exit(0)
    from bench import device_state  # noqa: E402
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks,
           "device_state": {"before": device_state(0)}}
    loops = {"step": (make(n, dev), lambda t: t.step(actions)), "torch_half": (make(n, dev), lambda t: tick_torch(t, actions)),
             "controller_and_plant": (Bare(n, dev), lambda t: t.tick())}
    for task, fn in loops.values():       # warm-up: cold solves, code objects, torch's kernels
        for _ in range(20):
            fn(task)
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(args.blocks):          # the three loops alternate, block by block
        for name, (task, fn) in loops.items():
            t0 = time.perf_counter()
            for _ in range(args.ticks):
                fn(task)
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    for name, w in wall.items():
        res[name] = {"ms_per_tick_median": med(w) / args.ticks * 1e3, "ms_per_tick_min": min(w) / args.ticks * 1e3, "ms_per_tick_max": max(w) / args.ticks * 1e3,
                     "robot_ticks_per_s": n * args.ticks / med(w)}
    # the parts, from events inside the running loops
    E = lambda k: [[torch.cuda.Event(enable_timing=True) for _ in range(k)] for _ in range(args.ticks * 2)]
    ev = E(6)
    for e in ev:
        tick_fused(loops["step"][0], actions, e)
    torch.cuda.synchronize()
    parts = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(5)] for e in ev])
    ev2 = E(2)
    for e in ev2:
        tick_torch(loops["torch_half"][0], actions, e)
    torch.cuda.synchronize()
    th = np.array([e[0].elapsed_time(e[1]) for e in ev2])
    names = ("controller_ms", "plant_ms", "begin_kernel_ms", "device_resets_ms", "finish_kernel_ms")
    res["parts_median_of_ticks"] = {nm: med(parts[:, i]) for i, nm in enumerate(names)}
    fused = parts[:, 2:].sum(1)
    res["parts_median_of_ticks"].update({"fused_half_ms": med(fused), "torch_half_ms": med(th), "events": len(ev)})
    res["added_per_tick_share_of_controller_step"] = med(fused) / med(parts[:, 0])
    res["fused_half_over_torch_half"] = med(fused) / med(th)
    res["step_over_controller_and_plant_rate"] = res["step"]["robot_ticks_per_s"] / res["controller_and_plant"]["robot_ticks_per_s"]
    res["step_over_torch_half_rate"] = res["step"]["robot_ticks_per_s"] / res["torch_half"]["robot_ticks_per_s"]
    res["fallen_fraction"] = {k: float(t.sim.flags()[1].float().mean().item()) for k, (t, _) in loops.items()}
    res["device_state"]["after"] = device_state(0, smi=False)
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
