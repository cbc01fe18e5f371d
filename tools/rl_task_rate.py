"""What the RL task's post-physics half costs: BatchedRLTask.step for 4096 Aliengo robots trotting, h = 10, against the loop of
tools/closed_loop_rate.py (controller + toy plant alone) and against the same half written as the plain torch composition with its
`reset_buf.nonzero()`.  Per tick, from HIP events inside the running loop (median over the ticks): the controller step, the toy plant's step, the
`begin` kernel, the device resets, the `finish` kernel; and the torch composition of begin + resets + finish.  Per loop, from the host clock around
blocks of ticks that end in a synchronise (median of the blocks, the three loops alternating): robot-ticks / s.  The shader clock is recorded as
bench.py --full records it (device_state).
    python tools/rl_task_rate.py [--ticks 100] [--blocks 7] [--out profiles/r08_rl_task.json]
--curriculum times the terrain curriculum instead (rl_mpc_locomotion_amd.curriculum) on legged_gym's 10 x 20 grid of 8 m tiles, in one process: the
`update` kernel alone and the `begin` kernel alone from HIP events inside the running loop (median, p10, p90 over the ticks), and BatchedRLTask.step
with the curriculum against the same task on the same field and origins without one, in alternating blocks; with --learn K also what K iterations of
PPO from level 0 do to the levels, and PPOTrainer.evaluate's falls per terrain type before and after.
    python tools/rl_task_rate.py --curriculum [--learn 30] [--out profiles/r14_curriculum.json]
--heights times the terrain height scan (rl_mpc_locomotion_amd.height_scan) on the same grid, with or without --curriculum: the scan kernel against
the `finish` kernel from HIP events inside the running loop (p10, median, p90 and the ratio), the bytes the kernel moves per second against what the
wide rows' writes alone come to, BatchedRLTask.step with and without the scan in alternating blocks, one PPOTrainer.learn iteration at 240 columns
against 48 for both update backends, and with --curriculum --learn K what K iterations do to the levels with and without the scan.
    python tools/rl_task_rate.py --heights [--curriculum --learn 30] [--out profiles/r15_height_scan.json]
--domain-rand times the opt-in domain randomisation (rl_mpc_locomotion_amd.domain_rand) at its widest, 240 columns with the height scan on the same grid:
the three launches alone from HIP events inside the running loop (the action-noise kernel, the push kernel -- launched on every tick for the timing --
and the observation-noise kernel, beside the `finish` kernel and the scan; p10, median, p90), the bytes the observation kernel moves, and
BatchedRLTask.step with the option (legged_gym's observation noise, gaussian action noise, a push every 1500 ticks) against the same task without it in
alternating blocks, with their p10 - p90 and the share of the tick the option adds.
    python tools/rl_task_rate.py --domain-rand [--out profiles/r16_domain_rand.json]
--terms times the per-term episode sums (rl_mpc_locomotion_amd.episode_terms), with --command-curriculum also the command curriculum they drive, on
the flat plane: the unit's two calls alone from HIP events inside the running loop (close_and_resample: two launches, three with the curriculum;
accumulate: one; beside the `begin` and `finish` kernels; p10, median, p90), and BatchedRLTask.step with the unit against the same task without it --
the step as it is without the option -- in alternating blocks, with the share of the tick the unit adds; with --learn K also what K PPO iterations
do with the curriculum and with the fixed default range (one seed: a finding, not a claim).
    python tools/rl_task_rate.py --terms [--command-curriculum] [--learn 20] [--out profiles/episode_terms_rate.json]
--privileged times the critic's privileged observation row (rl_mpc_locomotion_amd.privileged_obs), on the flat plane (48 actor columns, 64 privileged)
or with --heights on the terrain grid (240 and 240): the assembly kernel alone from HIP events inside the running loop, beside the `finish` kernel and
the scan (p10, median, p90), the bytes it moves, and BatchedRLTask.step with the option against the same task without it in alternating blocks, with
the share of the tick the launch adds.  --baseline times only the task without the option (it runs on a tree that has no such unit, for a
measurement of the parent commit in the same session).
    python tools/rl_task_rate.py --privileged [--heights] [--baseline] [--out results/privileged_step.json]
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


def spread(x):
    return {"median_ms": med(x), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def tick_curriculum(task, actions, ev):
    """BatchedRLTask.step's statements with a curriculum, with events around `update` and around `begin`"""
    sim, t = task.sim, task.task
    tau = task.bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, task.commands)
    sim.step(tau)
    ev[0].record()
    task.curriculum.update(task.reset_buf, sim.root_states, task.commands)
    ev[1].record()
    ids = t.begin()
    ev[2].record()
    task.bridge.ctl.reset(ids)
    sim.reset_idx(ids)
    _, fell = sim.flags()
    t.finish(sim.root_states, sim.dof_state, actions, tau, fell=fell)


def curriculum_report(args, dev, n, actions):
    from bench import device_state
    from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
    from rl_mpc_locomotion_amd.terrain import TerrainGrid
    grid = TerrainGrid(num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, seed=0)
    cfg = TaskConfig(**CFG)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks,
           "grid": {"levels": grid.num_levels, "types": grid.num_types, "tile_m": grid.tile_length, "nodes": [grid.terrain.rows, grid.terrain.cols]},
           "max_init_level": args.max_init_level, "device_state": {"before": device_state(0)}}

    def make_pair():
        cur = TerrainCurriculum(grid, n, max_init_level=args.max_init_level, seed=0, device=dev, episode_length_s=cfg.episode_length_s)
        with_c = BatchedRLTask([0] * n, [TROT] * n, cfg=cfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev, curriculum=cur)
        without = BatchedRLTask([0] * n, [TROT] * n, cfg=cfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev, terrain=grid.terrain, origin=cur.origins0)
        return cur, with_c, without
    cur, with_c, without = make_pair()
    loops = {"step_with_curriculum": with_c, "step_without": without}
    for task in loops.values():
        task.reset()
        for _ in range(20):
            task.step(actions)
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(args.blocks):          # the two loops alternate, block by block
        for name, task in loops.items():
            t0 = time.perf_counter()
            for _ in range(args.ticks):
                task.step(actions)
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    for name, w in wall.items():
        res[name] = {"ms_per_tick_median": med(w) / args.ticks * 1e3, "ms_per_tick_min": min(w) / args.ticks * 1e3, "ms_per_tick_max": max(w) / args.ticks * 1e3,
                     "robot_ticks_per_s": n * args.ticks / med(w)}
    res["with_over_without_ms_per_tick"] = res["step_with_curriculum"]["ms_per_tick_median"] / res["step_without"]["ms_per_tick_median"]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.ticks * 2)]
    for e in ev:
        tick_curriculum(with_c, actions, e)
    torch.cuda.synchronize()
    upd, beg = np.array([e[0].elapsed_time(e[1]) for e in ev]), np.array([e[1].elapsed_time(e[2]) for e in ev])
    res["update_kernel"], res["begin_kernel"], res["events"] = spread(upd), spread(beg), len(ev)
    res["update_over_begin_median"] = med(upd) / med(beg)
    res["condition_update_at_most_twice_begin"] = bool(med(upd) <= 2.0 * med(beg))
    s = cur.summary().tolist()
    res["after_timing"] = {"fallen_fraction": {k: float(t.sim.flags()[1].float().mean().item()) for k, t in loops.items()},
                           "resets_seen_per_env_mean": float(cur.counts.float().mean().item()), **TerrainCurriculum.record(s, grid.num_types)}
    res["device_state"]["mid"] = device_state(0, smi=False)
    if args.learn > 0:                    # a finding, not a condition: does the toy's policy climb?
        from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer
        res["learn"] = {}
        for normalize in (False, True):
            cur = TerrainCurriculum(grid, n, max_init_level=0, seed=0, device=dev, episode_length_s=TaskConfig().episode_length_s)
            task = BatchedRLTask([0] * n, [TROT] * n, cfg=TaskConfig(), horizon=10, yaw0=yaw, flat_ground=True, device=dev, curriculum=cur)
            trainer = PPOTrainer(task, PPOConfig(), seed=1, update="hip", normalize_obs=normalize)
            keys = ("episodes", "time_outs", "terminations", "mean_length")
            ev0 = trainer.evaluate(args.eval_ticks, groups=cur.types, num_groups=grid.num_types)
            lv0 = TerrainCurriculum.record(cur.summary().tolist(), grid.num_types)
            infos = trainer.learn(args.learn, init_at_random_ep_len=True)[-args.learn:]
            ev1 = trainer.evaluate(args.eval_ticks, groups=cur.types, num_groups=grid.num_types)
            lv1 = TerrainCurriculum.record(cur.summary().tolist(), grid.num_types)
            brief = lambda e: {"overall": {k: e[k] for k in keys}, "terminations_by_type": [g["terminations"] for g in e["groups"]],
                               "episodes_by_type": [g["episodes"] for g in e["groups"]]}
            res["learn"]["normalize_obs_" + str(normalize).lower()] = {
                "iterations": args.learn, "eval_ticks": args.eval_ticks, "tile_kind_of_type": list(grid.kind),
                "mean_terrain_level_per_iteration": [i["mean_terrain_level"] for i in infos], "mean_reward_per_iteration": [i["mean_reward"] for i in infos],
                "mean_episode_length_per_iteration": [i["mean_episode_length"] for i in infos],
                "terrain_level_by_type_last": infos[-1]["terrain_level_by_type"], "levels_after_first_evaluate": lv0, "levels_after_last_evaluate": lv1,
                "evaluate_before": brief(ev0), "evaluate_after": brief(ev1)}
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def tick_heights(task, actions, ev):
    """BatchedRLTask.step's statements with a height scan, with events around `finish` and around the scan"""
    sim, t = task.sim, task.task
    tau = task.bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, task.commands)
    sim.step(tau)
    if task.curriculum is not None:
        task.curriculum.update(task.reset_buf, sim.root_states, task.commands)
    ids = t.begin()
    task.bridge.ctl.reset(ids)
    sim.reset_idx(ids)
    _, fell = sim.flags()
    ev[0].record()
    t.finish(sim.root_states, sim.dof_state, actions, tau, fell=fell)
    ev[1].record()
    task.height_scan.measure(sim.root_states, t.obs_buf, out=task.obs_buf, heights=task.measured_heights)
    ev[2].record()


HBM_PEAK_BYTES_PER_S = 8.0e12           # MI355X, HBM3E spec


def heights_report(args, dev, n, actions):
    from bench import device_state
    from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
    from rl_mpc_locomotion_amd.height_scan import HeightScan
    from rl_mpc_locomotion_amd.terrain import TerrainGrid
    grid = TerrainGrid(num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, seed=0)
    cfg = TaskConfig(**CFG)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks,
           "grid": {"levels": grid.num_levels, "types": grid.num_types, "tile_m": grid.tile_length, "nodes": [grid.terrain.rows, grid.terrain.cols]},
           "curriculum": bool(args.curriculum), "max_init_level": args.max_init_level, "device_state": {"before": device_state(0)}}

    def make_task(with_scan, task_cfg=cfg, max_init_level=args.max_init_level):
        cur = TerrainCurriculum(grid, n, max_init_level=max_init_level, seed=0, device=dev, episode_length_s=task_cfg.episode_length_s)
        where = dict(curriculum=cur) if args.curriculum else dict(terrain=grid.terrain, origin=cur.origins0)
        return BatchedRLTask([0] * n, [TROT] * n, cfg=task_cfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev,
                             height_scan=HeightScan(n, device=dev) if with_scan else None, **where)
    loops = {"step_with_scan": make_task(True), "step_without": make_task(False)}
    for task in loops.values():
        task.reset()
        for _ in range(20):
            task.step(actions)
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(args.blocks):          # the two loops alternate, block by block
        for name, task in loops.items():
            t0 = time.perf_counter()
            for _ in range(args.ticks):
                task.step(actions)
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    for name, w in wall.items():
        res[name] = {"ms_per_tick_median": med(w) / args.ticks * 1e3, "ms_per_tick_min": min(w) / args.ticks * 1e3, "ms_per_tick_max": max(w) / args.ticks * 1e3,
                     "robot_ticks_per_s": n * args.ticks / med(w)}
    res["with_over_without_ms_per_tick"] = res["step_with_scan"]["ms_per_tick_median"] / res["step_without"]["ms_per_tick_median"]
    task = loops["step_with_scan"]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.ticks * 2)]
    for e in ev:
        tick_heights(task, actions, e)
    torch.cuda.synchronize()
    fin, scn = np.array([e[0].elapsed_time(e[1]) for e in ev]), np.array([e[1].elapsed_time(e[2]) for e in ev])
    res["finish_kernel"], res["scan_kernel"], res["events"] = spread(fin), spread(scn), len(ev)
    res["scan_over_finish_median"] = med(scn) / med(fin)
    # the bytes the algorithm needs, from the shapes: what it reads (root states, origins, the narrow rows, the points once, three int16 per point) and
    # what it writes (the wide rows, the heights)
    P, w = task.height_scan.num_points, task.num_obs
    rows = n * w * 4
    moved = rows + n * P * 4 + n * 48 * 4 + n * 13 * 4 + n * 2 * 8 + P * 2 * 4 + n * P * 3 * 2
    t_s = med(scn) * 1e-3
    res["scan_bytes"] = {"wide_row_writes": rows, "all_reads_and_writes": moved, "achieved_bytes_per_s": moved / t_s, "row_writes_bytes_per_s": rows / t_s,
                         "row_writes_alone_at_hbm_peak_ms": rows / HBM_PEAK_BYTES_PER_S * 1e3, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
                         "share_of_hbm_peak": moved / t_s / HBM_PEAK_BYTES_PER_S}
    cols = task.obs_buf[:, 48:48 + P]
    res["after_timing"] = {"fallen_fraction": {k: float(t.sim.flags()[1].float().mean().item()) for k, t in loops.items()},
                           "scan_columns": {"min": float(cols.min().item()), "max": float(cols.max().item()), "distinct": int(len(torch.unique(cols)))}}
    res["device_state"]["mid"] = device_state(0, smi=False)
    del loops, task
    # one learn iteration, 240 columns against 48, both update backends: alternating, after a warm-up iteration each
    from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer
    res["learn_iteration"] = {}
    for backend in ("torch", "hip"):
        trainers = {"columns_240": PPOTrainer(make_task(True), PPOConfig(), seed=1, update=backend),
                    "columns_48": PPOTrainer(make_task(False), PPOConfig(), seed=1, update=backend)}
        for tr in trainers.values():
            tr.learn(1)
        torch.cuda.synchronize()
        wall = {k: [] for k in trainers}
        for _ in range(args.learn_blocks):
            for name, tr in trainers.items():
                t0 = time.perf_counter()
                tr.learn(1)
                torch.cuda.synchronize()
                wall[name].append(time.perf_counter() - t0)
        out = {k: {"s_median": med(w), "s_min": min(w), "s_max": max(w)} for k, w in wall.items()}
        out["wide_over_narrow_median"] = out["columns_240"]["s_median"] / out["columns_48"]["s_median"]
        res["learn_iteration"][backend] = out
        del trainers
    if args.learn > 0 and args.curriculum:      # a finding, not a condition: does sight make the toy's policy climb?
        res["learn"] = {}
        for with_scan in (False, True):
            task = make_task(with_scan, task_cfg=TaskConfig(), max_init_level=0)
            trainer = PPOTrainer(task, PPOConfig(), seed=1, update="hip")
            infos = trainer.learn(args.learn, init_at_random_ep_len=True)[-args.learn:]
            res["learn"]["with_scan" if with_scan else "without_scan"] = {
                "iterations": args.learn, "num_obs": task.num_obs, "mean_terrain_level_per_iteration": [i["mean_terrain_level"] for i in infos],
                "mean_reward_per_iteration": [i["mean_reward"] for i in infos], "mean_episode_length_per_iteration": [i["mean_episode_length"] for i in infos],
                "terrain_level_by_type_last": infos[-1]["terrain_level_by_type"]}
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def tick_domain_rand(task, raw_actions, ev):
    """BatchedRLTask.step's statements with the domain randomisation, with events around its three launches, `finish` and the scan (the push is
    launched on every tick here, for the timing; max_vel 0 would freeze the robots, so it pushes as configured)"""
    sim, t, dr = task.sim, task.task, task.domain_rand
    dr.begin_step()
    ev[0].record()
    dr.noise("actions", raw_actions, out=task.actions, clip=task.cfg.clip_actions, tick=dr.tick)
    ev[1].record()
    tau = task.bridge.pre_physics_step(task.actions, sim.dof_state, sim.root_states, task.commands)
    sim.step(tau)
    dr.common_step_counter += 1
    ev[2].record()
    dr.push_robots(sim.root_states, dr.common_step_counter)
    ev[3].record()
    ids = t.begin()
    task.bridge.ctl.reset(ids)
    sim.reset_idx(ids)
    _, fell = sim.flags()
    ev[4].record()
    t.finish(sim.root_states, sim.dof_state, task.actions, tau, fell=fell)
    ev[5].record()
    task.height_scan.measure(sim.root_states, t.obs_buf, out=task.obs_buf, heights=task.measured_heights)
    ev[6].record()
    dr.noise("observations", task.obs_buf, active=task.num_active_obs, clip=task.cfg.clip_observations, tick=dr.tick)
    ev[7].record()


def domain_rand_report(args, dev, n, actions):
    from bench import device_state
    from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
    from rl_mpc_locomotion_amd.domain_rand import DomainRand, NoiseSpec, PushSpec
    from rl_mpc_locomotion_amd.height_scan import HeightScan
    from rl_mpc_locomotion_amd.terrain import TerrainGrid
    grid = TerrainGrid(num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, seed=0)
    cfg = TaskConfig(**CFG)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    origins = TerrainCurriculum(grid, n, max_init_level=args.max_init_level, seed=0, device=dev, episode_length_s=cfg.episode_length_s).origins0
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks,
           "grid": {"levels": grid.num_levels, "types": grid.num_types, "tile_m": grid.tile_length, "nodes": [grid.terrain.rows, grid.terrain.cols]},
           "device_state": {"before": device_state(0)}}

    def make_task(with_dr):
        scan = HeightScan(n, device=dev)
        dr = DomainRand(n, observations=NoiseSpec.legged_gym(cfg, height_scan=scan), actions=NoiseSpec("gaussian", "additive", (0.0, 0.02)),
                        push=PushSpec(), seed=1, device=dev) if with_dr else None
        return BatchedRLTask([0] * n, [TROT] * n, cfg=cfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev, terrain=grid.terrain, origin=origins,
                             height_scan=scan, domain_rand=dr)
    loops = {"step_with_domain_rand": make_task(True), "step_without": make_task(False)}
    for task in loops.values():
        task.reset()
        for _ in range(20):
            task.step(actions)
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(args.blocks):          # the two loops alternate, block by block
        for name, task in loops.items():
            t0 = time.perf_counter()
            for _ in range(args.ticks):
                task.step(actions)
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    for name, w in wall.items():
        per = np.array(w) / args.ticks * 1e3
        res[name] = {"ms_per_tick_median": med(per), "ms_per_tick_p10": float(np.percentile(per, 10)), "ms_per_tick_p90": float(np.percentile(per, 90)),
                     "ms_per_tick_min": float(per.min()), "ms_per_tick_max": float(per.max()), "robot_ticks_per_s": n * args.ticks / med(w)}
    res["with_over_without_ms_per_tick"] = res["step_with_domain_rand"]["ms_per_tick_median"] / res["step_without"]["ms_per_tick_median"]
    task = loops["step_with_domain_rand"]
    res["launches_in_the_timed_blocks"] = dict(task.domain_rand.launches)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(8)] for _ in range(args.ticks * 2)]
    for e in ev:
        tick_domain_rand(task, actions, e)
    torch.cuda.synchronize()
    span = lambda i: np.array([e[i].elapsed_time(e[i + 1]) for e in ev])
    parts = {"action_noise_kernel": span(0), "push_kernel": span(2), "finish_kernel": span(4), "scan_kernel": span(5), "observation_noise_kernel": span(6)}
    for k, v in parts.items():
        res[k] = spread(v)
    res["events"] = len(ev)
    three = med(parts["action_noise_kernel"]) + med(parts["observation_noise_kernel"])
    tick_ms = res["step_without"]["ms_per_tick_median"]
    res["share_of_the_tick"] = {"two_noise_launches_medians_ms": three, "push_launch_median_ms": med(parts["push_kernel"]),
                                "noise_launches_over_step_without": three / tick_ms,
                                "all_three_over_step_without": (three + med(parts["push_kernel"])) / tick_ms,
                                "measured_step_difference_over_step_without": res["with_over_without_ms_per_tick"] - 1.0}
    w = task.num_obs
    rows = 2 * n * w * 4 + w * 4          # the rows read and written, the column scales
    t_s = med(parts["observation_noise_kernel"]) * 1e-3
    res["observation_noise_bytes"] = {"rows_read_and_written": rows, "achieved_bytes_per_s": rows / t_s, "at_hbm_peak_ms": rows / HBM_PEAK_BYTES_PER_S * 1e3,
                                      "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "share_of_hbm_peak": rows / t_s / HBM_PEAK_BYTES_PER_S}
    res["observation_noise_over_scan_median"] = med(parts["observation_noise_kernel"]) / med(parts["scan_kernel"])
    res["after_timing"] = {"fallen_fraction": {k: float(t.sim.flags()[1].float().mean().item()) for k, t in loops.items()}}
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def tick_terms(task, actions, ev):
    """BatchedRLTask.step's statements with the episode terms, with events around `begin`, the unit's two calls and `finish`"""
    sim, t, et = task.sim, task.task, task.episode_terms
    tau = task.bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, task.commands)
    sim.step(tau)
    ev[0].record()
    ids = t.begin()
    ev[1].record()
    task.common_step_counter += 1
    et.close_and_resample(ids, task.commands, task.common_step_counter)
    ev[2].record()
    task.bridge.ctl.reset(ids)
    sim.reset_idx(ids)
    _, fell = sim.flags()
    ev[3].record()
    t.finish(sim.root_states, sim.dof_state, actions, tau, fell=fell)
    ev[4].record()
    et.accumulate(sim.root_states, task.commands, tau, fell)
    ev[5].record()


def terms_report(args, dev, n, actions):
    from bench import device_state
    from rl_mpc_locomotion_amd.episode_terms import CommandCurriculumSpec, EpisodeTerms
    cfg = TaskConfig(episode_length_s=args.episode_s)                          # the default command ranges: the curriculum starts inside them
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    spec = CommandCurriculumSpec(max_curriculum=2.5, x_range0=(-1.0, 1.0)) if args.command_curriculum else None
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks,
           "command_curriculum": bool(args.command_curriculum), "episode_length_s": cfg.episode_length_s,
           "launches_per_tick": {"close_and_resample": 3 if spec is not None else 2, "accumulate": 1}, "device_state": {"before": device_state(0)}}

    def make_task(with_terms, task_cfg=cfg, task_spec=spec):
        et = EpisodeTerms(n, task_cfg, command_curriculum=task_spec, device=dev) if with_terms else None
        return BatchedRLTask([0] * n, [TROT] * n, cfg=task_cfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev, episode_terms=et)
    loops = {"step_with_terms": make_task(True), "step_without": make_task(False)}
    for task in loops.values():
        task.reset()
        for _ in range(20):
            task.step(actions)
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(args.blocks):          # the two loops alternate, block by block
        for name, task in loops.items():
            t0 = time.perf_counter()
            for _ in range(args.ticks):
                task.step(actions)
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    for name, w in wall.items():
        per = np.array(w) / args.ticks * 1e3
        res[name] = {"ms_per_tick_median": med(per), "ms_per_tick_p10": float(np.percentile(per, 10)), "ms_per_tick_p90": float(np.percentile(per, 90)),
                     "ms_per_tick_min": float(per.min()), "ms_per_tick_max": float(per.max()), "robot_ticks_per_s": n * args.ticks / med(w)}
    res["with_over_without_ms_per_tick"] = res["step_with_terms"]["ms_per_tick_median"] / res["step_without"]["ms_per_tick_median"]
    task = loops["step_with_terms"]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(args.ticks * 2)]
    for e in ev:
        tick_terms(task, actions, e)
    torch.cuda.synchronize()
    span = lambda i: np.array([e[i].elapsed_time(e[i + 1]) for e in ev])
    parts = {"begin_kernel": span(0), "close_and_resample": span(1), "finish_kernel": span(3), "accumulate_kernel": span(4)}
    for k, v in parts.items():
        res[k] = spread(v)
    res["events"] = len(ev)
    unit = med(parts["close_and_resample"]) + med(parts["accumulate_kernel"])
    tick_ms = res["step_without"]["ms_per_tick_median"]
    res["share_of_the_tick"] = {"unit_launches_medians_us": unit * 1e3, "unit_over_step_without": unit / tick_ms,
                                "unit_over_begin_plus_finish": unit / (med(parts["begin_kernel"]) + med(parts["finish_kernel"])),
                                "measured_step_difference_over_step_without": res["with_over_without_ms_per_tick"] - 1.0}
    et = task.episode_terms
    res["after_timing"] = {"fallen_fraction": {k: float(t.sim.flags()[1].float().mean().item()) for k, t in loops.items()},
                           "resamples_seen_per_env_mean": float(et.counts.float().mean().item()), "record": EpisodeTerms.record(et.summary().tolist())}
    res["device_state"]["mid"] = device_state(0, smi=False)
    del loops, task
    if args.learn > 0:                    # a finding, not a condition, and one seed: what the curriculum does to a short training run
        from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer
        res["learn"] = {"seeds": 1, "iterations": args.learn}
        learn_cfg = TaskConfig()
        for name, learn_spec in (("command_curriculum", CommandCurriculumSpec(max_curriculum=2.5, x_range0=(-1.0, 1.0))), ("fixed_default_range", None)):
            trainer = PPOTrainer(make_task(True, learn_cfg, learn_spec), PPOConfig(), seed=1, update="hip")
            infos = trainer.learn(args.learn, init_at_random_ep_len=True)[-args.learn:]
            res["learn"][name] = {"mean_reward_per_iteration": [i["mean_reward"] for i in infos],
                                  "mean_episode_length_per_iteration": [i["mean_episode_length"] for i in infos],
                                  "rew_lin_vel_xy_per_iteration": [i["episode_terms"]["rew_lin_vel_xy"] for i in infos],
                                  "max_command_x_per_iteration": [i["episode_terms"]["max_command_x"] for i in infos], "last_record": infos[-1]["episode_terms"]}
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def tick_privileged(task, actions, ev):
    """BatchedRLTask.step's statements with the privileged row, with events around `finish`, the scan (when there is one) and the assembly kernel"""
    sim, t = task.sim, task.task
    tau = task.bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, task.commands)
    sim.step(tau)
    ids = t.begin()
    task.bridge.ctl.reset(ids)
    sim.reset_idx(ids)
    _, fell = sim.flags()
    ev[0].record()
    t.finish(sim.root_states, sim.dof_state, actions, tau, fell=fell)
    ev[1].record()
    if task.height_scan is not None:
        task.height_scan.measure(sim.root_states, t.obs_buf, out=task.obs_buf, heights=task.measured_heights)
    ev[2].record()
    task.privileged_obs.assemble(task.obs_buf, task.progress_buf, task._inv_len, num_scan=task._num_scan, out=task.privileged_obs_buf)
    ev[3].record()


def privileged_report(args, dev, n, actions):
    from bench import device_state
    cfg = TaskConfig(**CFG)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks,
           "heights": bool(args.heights), "baseline_only": bool(args.baseline), "device_state": {"before": device_state(0)}}
    where = {}
    if args.heights:
        from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
        from rl_mpc_locomotion_amd.height_scan import HeightScan
        from rl_mpc_locomotion_amd.terrain import TerrainGrid
        grid = TerrainGrid(num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, seed=0)
        origins = TerrainCurriculum(grid, n, max_init_level=args.max_init_level, seed=0, device=dev, episode_length_s=cfg.episode_length_s).origins0
        where = dict(terrain=grid.terrain, origin=origins)

    def make_task(with_privileged):
        opts = dict(where)
        if args.heights:
            opts["height_scan"] = HeightScan(n, device=dev)
        if with_privileged:
            from rl_mpc_locomotion_amd.privileged_obs import PrivilegedObs
            opts["privileged_obs"] = PrivilegedObs(n, device=dev)
        return BatchedRLTask([0] * n, [TROT] * n, cfg=cfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev, **opts)
    loops = {"step_without": make_task(False)} if args.baseline else {"step_with_privileged": make_task(True), "step_without": make_task(False)}
    for task in loops.values():
        task.reset()
        for _ in range(20):
            task.step(actions)
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(args.blocks):          # the loops alternate, block by block
        for name, task in loops.items():
            t0 = time.perf_counter()
            for _ in range(args.ticks):
                task.step(actions)
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    for name, w in wall.items():
        per = np.array(w) / args.ticks * 1e3
        res[name] = {"ms_per_tick_median": med(per), "ms_per_tick_p10": float(np.percentile(per, 10)), "ms_per_tick_p90": float(np.percentile(per, 90)),
                     "ms_per_tick_min": float(per.min()), "ms_per_tick_max": float(per.max()), "robot_ticks_per_s": n * args.ticks / med(w)}
    res["after_timing"] = {"fallen_fraction": {k: float(t.sim.flags()[1].float().mean().item()) for k, t in loops.items()}}
    if not args.baseline:
        res["with_over_without_ms_per_tick"] = res["step_with_privileged"]["ms_per_tick_median"] / res["step_without"]["ms_per_tick_median"]
        task = loops["step_with_privileged"]
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.ticks * 2)]
        for e in ev:
            tick_privileged(task, actions, e)
        torch.cuda.synchronize()
        span = lambda i: np.array([e[i].elapsed_time(e[i + 1]) for e in ev])
        parts = {"finish_kernel": span(0), "assembly_kernel": span(2)}
        if args.heights:
            parts["scan_kernel"] = span(1)
        for k, v in parts.items():
            res[k] = spread(v)
        res["events"] = len(ev)
        tick_ms = res["step_without"]["ms_per_tick_median"]
        res["share_of_the_tick"] = {"assembly_kernel_median_us": med(parts["assembly_kernel"]) * 1e3, "assembly_over_step_without": med(parts["assembly_kernel"]) / tick_ms,
                                    "assembly_over_finish_median": med(parts["assembly_kernel"]) / med(parts["finish_kernel"]),
                                    "measured_step_difference_over_step_without": res["with_over_without_ms_per_tick"] - 1.0}
        # the bytes the algorithm needs, from the shapes: the live columns read, four contact words and one counter per environment, the whole row written
        wp, live = task.num_privileged_obs, 48 + task._num_scan
        moved = n * live * 4 + n * 4 * 4 + n * 8 + n * wp * 4
        t_s = med(parts["assembly_kernel"]) * 1e-3
        res["assembly_bytes"] = {"actor_columns": task.num_obs, "privileged_columns": wp, "row_writes": n * wp * 4, "all_reads_and_writes": moved,
                                 "achieved_bytes_per_s": moved / t_s, "at_hbm_peak_ms": moved / HBM_PEAK_BYTES_PER_S * 1e3,
                                 "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "share_of_hbm_peak": moved / t_s / HBM_PEAK_BYTES_PER_S}
        rows = task.privileged_obs_buf
        res["after_timing"]["privileged_row"] = {"contact_mean": float(rows[:, live:live + 4].mean().item()), "phase_max": float(rows[:, live + 4].max().item()),
                                                  "equals_the_actor_row_in_the_live_columns": bool(torch.equal(rows[:, :live], task.obs_buf[:, :live]))}
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=100, help="ticks per block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--quick", action="store_true", help="one block of BatchedRLTask.step only (for a kernel trace)")
    ap.add_argument("--curriculum", action="store_true", help="time the terrain curriculum (see the head of this file)")
    ap.add_argument("--max-init-level", type=int, default=9, help="--curriculum: initial levels uniform in 0 .. this")
    ap.add_argument("--learn", type=int, default=0, help="--curriculum: also K PPO iterations from level 0, with evaluate() before and after; --terms: K iterations with and without the command curriculum")
    ap.add_argument("--eval-ticks", type=int, default=500)
    ap.add_argument("--heights", action="store_true", help="time the terrain height scan (see the head of this file); with or without --curriculum")
    ap.add_argument("--learn-blocks", type=int, default=3, help="--heights: timed learn iterations per trainer")
    ap.add_argument("--domain-rand", action="store_true", help="time the domain randomisation's three launches and the step with and without it")
    ap.add_argument("--terms", action="store_true", help="time the per-term episode sums' launches and the step with and without them")
    ap.add_argument("--command-curriculum", action="store_true", help="--terms: with the command curriculum (one more launch per tick)")
    ap.add_argument("--episode-s", type=float, default=20.0, help="--terms: the episode length of the timed tasks, in seconds")
    ap.add_argument("--privileged", action="store_true", help="time the privileged row's assembly kernel and the step with and without it; with or without --heights")
    ap.add_argument("--baseline", action="store_true", help="--privileged: only the task without the option (runs on a tree without the unit)")
    ap.add_argument("--out")
    args = ap.parse_args()
    dev, n = "cuda:0", args.robots
    actions = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    if args.privileged or args.terms or args.domain_rand or args.heights or args.curriculum:
        res = (privileged_report if args.privileged else terms_report if args.terms else domain_rand_report if args.domain_rand else heights_report if args.heights else curriculum_report)(args, dev, n, actions)
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        sys.exit(0)
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
