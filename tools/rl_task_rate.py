"""What BatchedRLTask.step costs, whole and by its parts, for 4096 Aliengo robots trotting, h = 10.  Every mode times the product's own tick:
whole ticks from the host clock around blocks of ticks that end in a synchronise (median, p10, p90, min, max of the blocks, the loops alternating
block by block; robot-ticks / s), and the tick's parts from HIP events recorded in the `mark` that `step` calls after each of its stages
(rl_task.STAGES; tools/_rate.py: stage_times) -- a part's time is the span from the event before it to its own, p10 / median / p90 over the ticks.
The shader clock is recorded as bench.py --full records it (device_state).
The default mode sets the step against the loop of tools/closed_loop_rate.py (controller + toy plant alone) and against its post-physics half
written as the plain torch composition with its `reset_buf.nonzero()` (torch_half):
    python tools/rl_task_rate.py [--ticks 100] [--blocks 7] [--out profiles/r08_rl_task.json]
--curriculum: the terrain curriculum (rl_mpc_locomotion_amd.curriculum) on legged_gym's 10 x 20 grid of 8 m tiles: the `update` kernel beside the
`begin` kernel, and the step with the curriculum against the same task on the same field and origins without one; with --learn K also what K
iterations of PPO from level 0 do to the levels, and PPOTrainer.evaluate's falls per terrain type before and after.
    python tools/rl_task_rate.py --curriculum [--learn 30] [--out profiles/r14_curriculum.json]
--heights: the terrain height scan (rl_mpc_locomotion_amd.height_scan) on the same grid, with or without --curriculum: the scan kernel beside the
`finish` kernel, the bytes the kernel moves per second against what the wide rows' writes alone come to, the step with and without the scan, one
PPOTrainer.learn iteration at 240 columns against 48 for both update backends, and with --curriculum --learn K what K iterations do to the levels
with and without the scan.
    python tools/rl_task_rate.py --heights [--curriculum --learn 30] [--out profiles/r15_height_scan.json]
--domain-rand: the opt-in domain randomisation (rl_mpc_locomotion_amd.domain_rand) at its widest, 240 columns with the height scan on the same
grid: its three launches (action noise, push, observation noise) beside the `finish` kernel and the scan, the bytes the observation kernel moves,
and the step with the option (legged_gym's observation noise, gaussian action noise, a push every 1500 ticks) against the same task without it.
For the event pass the DomainRand's public `push_interval` is set to 1, so that the product's own `after_physics` pushes on every tick: the tool
never launches a push itself.
    python tools/rl_task_rate.py --domain-rand [--out profiles/r16_domain_rand.json]
--terms: the per-term episode sums (rl_mpc_locomotion_amd.episode_terms), with --command-curriculum also the command curriculum they drive, on
the flat plane: the unit's two calls (close_and_resample: two launches, three with the curriculum; accumulate: one) beside the `begin` and `finish`
kernels, and the step with the unit against the same task without it; with --learn K also what K PPO iterations do with the curriculum and with
the fixed default range (one seed: a finding, not a claim).
    python tools/rl_task_rate.py --terms [--command-curriculum] [--learn 20] [--out profiles/episode_terms_rate.json]
--privileged: the critic's privileged observation row (rl_mpc_locomotion_amd.privileged_obs), on the flat plane (48 actor columns, 64 privileged)
or with --heights on the terrain grid (240 and 240): the assembly kernel beside the `finish` kernel and the scan, the bytes it moves, and the step
with the option against the same task without it.  --baseline times only the task without the option and passes no `mark` (it runs on a tree that
has neither, for a measurement of a parent commit in the same session).
    python tools/rl_task_rate.py --privileged [--heights] [--baseline] [--out results/privileged_step.json]
--plant-rand: the per-robot plant record (rl_mpc_locomotion_amd.plant_rand) with ranges on all three axes, on the flat plane: the step with the
option against the same task without it, and the `controller`, `plant` (the parametrised step kernel against the plain one) and `resets` (which
holds the draw) stages of both, from events, the tasks alternating; a third task carries a record that stays neutral, which separates the kernel's
cost from that of robots that differ.  With --privileged all of them assemble the critic's row, with the plant columns where there is a record.
    python tools/rl_task_rate.py --plant-rand [--privileged] [--out profiles/plant_rand_rate.json]
--shaping: the opt-in reward shaping terms (rl_mpc_locomotion_amd.reward_shaping) with every scale non-zero; with --heights on the terrain grid with
the scan (base_height over the measured heights), with --terms beside the per-term episode sums: the step with the option against the same task
without it, block by block, and the added time per tick from the blocks' differences; the stages that hold the unit's launches (`resets`: close,
`height_scan` or `finish`: run) of both tasks, and the episode sums' own two stages of the same run as the yardstick.
    python tools/rl_task_rate.py --shaping --heights --terms [--out profiles/reward_shaping_rate.json]
--contact: the opt-in contact terms (rl_mpc_locomotion_amd.contact_terms) with every scale non-zero on a plant with a friction record drawn below and
above the controller's mu, with --privileged the critic's sixteen columns as well; --shaping, --heights and --terms as above, for all three tasks:
the step with the option against the same task without it, block by block, and the added time per tick; the stages that hold the unit's launches
(`resets`: close, `height_scan` or `finish`: run, `privileged_obs`: extend) of both tasks; and with --shaping a third task without the shaping terms
either, whose difference to the second is the yardstick of the same run: reward_shaping's three launches.
    python tools/rl_task_rate.py --contact --shaping --heights --terms --privileged [--out profiles/contact_terms_rate.json]
The kernel-trace stats of the same step: rocprofv3 --kernel-trace --stats ... -- python tools/rl_task_rate.py --ticks 50 --quick"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_mpc_locomotion_amd  # noqa: E402,F401
from _rate import HBM_PEAK_BYTES_PER_S, clock, emit, ev, header, med, spread, stage_times, terrain_grid, wall_blocks  # noqa: E402
from rl_mpc_locomotion_amd.rl_task import REWARD_TERMS, BatchedRLTask, TaskConfig  # noqa: E402

TROT = 0
# the closed-loop golden's trot command (0.5 m/s ahead) as a one-point command range; zero actions are its MPC weights (5 5 5 50 50 50 1 ...)
CFG = dict(command_x_range=(0.5, 0.5), command_y_range=(0.0, 0.0), command_yaw_range=(0.0, 0.0))
# --plant-rand: legged_gym's added_mass_range and the usual motor-strength and gravity ranges, all three axes
PLANT_RANGES = dict(payload=(-1.0, 3.0), strength=(0.9, 1.1), gravity=(-1.0, 1.0))


def make(n, dev, cfg=None, **options):
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    return BatchedRLTask([0] * n, [TROT] * n, cfg=cfg if cfg is not None else TaskConfig(**CFG), horizon=10, yaw0=yaw, flat_ground=True, device=dev, **options)


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


def blocks(res, args, actions, loops, per_block=False):
    """The whole ticks of the tasks ``loops`` names, reset first: their records into ``res``, and the first over ``step_without`` where there are two."""
    for task in loops.values():
        task.reset()
    res.update(wall_blocks({k: (lambda t=t: t.step(actions)) for k, t in loops.items()}, args.ticks, args.blocks, args.robots, per_block=per_block))
    if len(loops) == 2:
        res["with_over_without_ms_per_tick"] = res[next(iter(loops))]["ms_per_tick_median"] / res["step_without"]["ms_per_tick_median"]


def stages(res, args, actions, task, keys):
    """The parts of ``task``'s own tick that ``keys`` {record key: stage} names: their spreads into ``res``, their medians back."""
    parts = stage_times(task, actions, args.ticks)
    for key, stage in keys.items():
        res[key] = spread(parts[stage])
    res["events"] = 2 * args.ticks
    return {key: med(parts[stage]) for key, stage in keys.items()}


def fallen(loops):
    return {k: float(t.sim.flags()[1].float().mean().item()) for k, t in loops.items()}


def hbm(moved, ms):
    t_s = ms * 1e-3
    return {"achieved_bytes_per_s": moved / t_s, "at_hbm_peak_ms": moved / HBM_PEAK_BYTES_PER_S * 1e3, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
            "share_of_hbm_peak": moved / t_s / HBM_PEAK_BYTES_PER_S}


def curriculum_report(args, dev, n, actions):
    cfg = TaskConfig(**CFG)
    grid, curriculum, grid_rec = terrain_grid(n, args.max_init_level, dev, cfg.episode_length_s)
    res = header(args, n, grid=grid_rec, max_init_level=args.max_init_level)
    cur = curriculum()
    loops = {"step_with_curriculum": make(n, dev, cfg, curriculum=cur), "step_without": make(n, dev, cfg, terrain=grid.terrain, origin=cur.origins0)}
    blocks(res, args, actions, loops)
    p = stages(res, args, actions, loops["step_with_curriculum"], {"update_kernel": "terrain_curriculum", "begin_kernel": "begin"})
    res["update_over_begin_median"] = p["update_kernel"] / p["begin_kernel"]
    res["condition_update_at_most_twice_begin"] = bool(p["update_kernel"] <= 2.0 * p["begin_kernel"])
    res["after_timing"] = {"fallen_fraction": fallen(loops), "resets_seen_per_env_mean": float(cur.counts.float().mean().item()),
                           **cur.record(cur.summary().tolist(), grid.num_types)}
    clock(res, "mid")
    if args.learn > 0:                    # a finding, not a condition: does the toy's policy climb?
        from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer
        res["learn"] = {}
        for normalize in (False, True):
            cur = curriculum(0, TaskConfig().episode_length_s)
            trainer = PPOTrainer(make(n, dev, TaskConfig(), curriculum=cur), PPOConfig(), seed=1, update="hip", normalize_obs=normalize)
            keys = ("episodes", "time_outs", "terminations", "mean_length")
            ev0 = trainer.evaluate(args.eval_ticks, groups=cur.types, num_groups=grid.num_types)
            lv0 = cur.record(cur.summary().tolist(), grid.num_types)
            infos = trainer.learn(args.learn, init_at_random_ep_len=True)[-args.learn:]
            ev1 = trainer.evaluate(args.eval_ticks, groups=cur.types, num_groups=grid.num_types)
            lv1 = cur.record(cur.summary().tolist(), grid.num_types)
            brief = lambda e: {"overall": {k: e[k] for k in keys}, "terminations_by_type": [g["terminations"] for g in e["groups"]],
                               "episodes_by_type": [g["episodes"] for g in e["groups"]]}
            res["learn"]["normalize_obs_" + str(normalize).lower()] = {
                "iterations": args.learn, "eval_ticks": args.eval_ticks, "tile_kind_of_type": list(grid.kind),
                "mean_terrain_level_per_iteration": [i["mean_terrain_level"] for i in infos], "mean_reward_per_iteration": [i["mean_reward"] for i in infos],
                "mean_episode_length_per_iteration": [i["mean_episode_length"] for i in infos],
                "terrain_level_by_type_last": infos[-1]["terrain_level_by_type"], "levels_after_first_evaluate": lv0, "levels_after_last_evaluate": lv1,
                "evaluate_before": brief(ev0), "evaluate_after": brief(ev1)}
    clock(res, "after")
    return res


def heights_report(args, dev, n, actions):
    from rl_mpc_locomotion_amd.height_scan import HeightScan
    cfg = TaskConfig(**CFG)
    grid, curriculum, grid_rec = terrain_grid(n, args.max_init_level, dev, cfg.episode_length_s)
    res = header(args, n, grid=grid_rec, curriculum=bool(args.curriculum), max_init_level=args.max_init_level)

    def make_task(with_scan, task_cfg=cfg, max_init_level=args.max_init_level):
        cur = curriculum(max_init_level, task_cfg.episode_length_s)
        where = dict(curriculum=cur) if args.curriculum else dict(terrain=grid.terrain, origin=cur.origins0)
        return make(n, dev, task_cfg, height_scan=HeightScan(n, device=dev) if with_scan else None, **where)
    loops = {"step_with_scan": make_task(True), "step_without": make_task(False)}
    blocks(res, args, actions, loops)
    task = loops["step_with_scan"]
    p = stages(res, args, actions, task, {"finish_kernel": "finish", "scan_kernel": "height_scan"})
    res["scan_over_finish_median"] = p["scan_kernel"] / p["finish_kernel"]
    # the bytes the algorithm needs, from the shapes: what it reads (root states, origins, the narrow rows, the points once, three int16 per point) and
    # what it writes (the wide rows, the heights)
    P, w = task.height_scan.num_points, task.num_obs
    rows = n * w * 4
    moved = rows + n * P * 4 + n * 48 * 4 + n * 13 * 4 + n * 2 * 8 + P * 2 * 4 + n * P * 3 * 2
    t_s = p["scan_kernel"] * 1e-3
    res["scan_bytes"] = {"wide_row_writes": rows, "all_reads_and_writes": moved, "achieved_bytes_per_s": moved / t_s, "row_writes_bytes_per_s": rows / t_s,
                         "row_writes_alone_at_hbm_peak_ms": rows / HBM_PEAK_BYTES_PER_S * 1e3, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
                         "share_of_hbm_peak": moved / t_s / HBM_PEAK_BYTES_PER_S}
    cols = task.obs_buf[:, 48:48 + P]
    res["after_timing"] = {"fallen_fraction": fallen(loops),
                           "scan_columns": {"min": float(cols.min().item()), "max": float(cols.max().item()), "distinct": int(len(torch.unique(cols)))}}
    clock(res, "mid")
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
    clock(res, "after")
    return res


def domain_rand_report(args, dev, n, actions):
    from rl_mpc_locomotion_amd.domain_rand import DomainRand, NoiseSpec, PushSpec
    from rl_mpc_locomotion_amd.height_scan import HeightScan
    cfg = TaskConfig(**CFG)
    grid, curriculum, grid_rec = terrain_grid(n, args.max_init_level, dev, cfg.episode_length_s)
    origins = curriculum().origins0
    res = header(args, n, grid=grid_rec)

    def make_task(with_dr):
        scan = HeightScan(n, device=dev)
        dr = DomainRand(n, observations=NoiseSpec.legged_gym(cfg, height_scan=scan), actions=NoiseSpec("gaussian", "additive", (0.0, 0.02)),
                        push=PushSpec(), seed=1, device=dev) if with_dr else None
        return make(n, dev, cfg, terrain=grid.terrain, origin=origins, height_scan=scan, domain_rand=dr)
    loops = {"step_with_domain_rand": make_task(True), "step_without": make_task(False)}
    blocks(res, args, actions, loops)
    task = loops["step_with_domain_rand"]
    res["launches_in_the_timed_blocks"] = dict(task.domain_rand.launches)
    task.domain_rand.push_interval = 1     # from here on the product's after_physics pushes on every tick (max_vel 0 would freeze the robots: it pushes as configured)
    p = stages(res, args, actions, task, {"action_noise_kernel": "actions", "push_kernel": "push", "finish_kernel": "finish", "scan_kernel": "height_scan",
                                          "observation_noise_kernel": "observation_noise"})
    two = p["action_noise_kernel"] + p["observation_noise_kernel"]
    tick_ms = res["step_without"]["ms_per_tick_median"]
    res["share_of_the_tick"] = {"two_noise_launches_medians_ms": two, "push_launch_median_ms": p["push_kernel"], "noise_launches_over_step_without": two / tick_ms,
                                "all_three_over_step_without": (two + p["push_kernel"]) / tick_ms,
                                "measured_step_difference_over_step_without": res["with_over_without_ms_per_tick"] - 1.0}
    w = task.num_obs
    rows = 2 * n * w * 4 + w * 4          # the rows read and written, the column scales
    res["observation_noise_bytes"] = {"rows_read_and_written": rows, **hbm(rows, p["observation_noise_kernel"])}
    res["observation_noise_over_scan_median"] = p["observation_noise_kernel"] / p["scan_kernel"]
    res["after_timing"] = {"fallen_fraction": fallen(loops)}
    clock(res, "after")
    return res


def terms_report(args, dev, n, actions):
    from rl_mpc_locomotion_amd.episode_terms import CommandCurriculumSpec, EpisodeTerms
    cfg = TaskConfig(episode_length_s=args.episode_s)                          # the default command ranges: the curriculum starts inside them
    spec = CommandCurriculumSpec(max_curriculum=2.5, x_range0=(-1.0, 1.0)) if args.command_curriculum else None
    res = header(args, n, command_curriculum=bool(args.command_curriculum), episode_length_s=cfg.episode_length_s,
                 launches_per_tick={"close_and_resample": 3 if spec is not None else 2, "accumulate": 1})

    def make_task(with_terms, task_cfg=cfg, task_spec=spec):
        return make(n, dev, task_cfg, episode_terms=EpisodeTerms(n, task_cfg, command_curriculum=task_spec, device=dev) if with_terms else None)
    loops = {"step_with_terms": make_task(True), "step_without": make_task(False)}
    blocks(res, args, actions, loops)
    task = loops["step_with_terms"]
    p = stages(res, args, actions, task, {"begin_kernel": "begin", "close_and_resample": "episode_close", "finish_kernel": "finish",
                                          "accumulate_kernel": "episode_accumulate"})
    unit = p["close_and_resample"] + p["accumulate_kernel"]
    res["share_of_the_tick"] = {"unit_launches_medians_us": unit * 1e3, "unit_over_step_without": unit / res["step_without"]["ms_per_tick_median"],
                                "unit_over_begin_plus_finish": unit / (p["begin_kernel"] + p["finish_kernel"]),
                                "measured_step_difference_over_step_without": res["with_over_without_ms_per_tick"] - 1.0}
    et = task.episode_terms
    res["after_timing"] = {"fallen_fraction": fallen(loops), "resamples_seen_per_env_mean": float(et.counts.float().mean().item()),
                           "record": EpisodeTerms.record(et.summary().tolist())}
    clock(res, "mid")
    del loops, task
    if args.learn > 0:                    # a finding, not a condition, and one seed: what the curriculum does to a short training run
        from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer
        res["learn"] = {"seeds": 1, "iterations": args.learn}
        for name, learn_spec in (("command_curriculum", CommandCurriculumSpec(max_curriculum=2.5, x_range0=(-1.0, 1.0))), ("fixed_default_range", None)):
            trainer = PPOTrainer(make_task(True, TaskConfig(), learn_spec), PPOConfig(), seed=1, update="hip")
            infos = trainer.learn(args.learn, init_at_random_ep_len=True)[-args.learn:]
            res["learn"][name] = {"mean_reward_per_iteration": [i["mean_reward"] for i in infos],
                                  "mean_episode_length_per_iteration": [i["mean_episode_length"] for i in infos],
                                  "rew_lin_vel_xy_per_iteration": [i["episode_terms"]["rew_lin_vel_xy"] for i in infos],
                                  "max_command_x_per_iteration": [i["episode_terms"]["max_command_x"] for i in infos], "last_record": infos[-1]["episode_terms"]}
    clock(res, "after")
    return res


def privileged_report(args, dev, n, actions):
    cfg = TaskConfig(**CFG)
    res = header(args, n, heights=bool(args.heights), baseline_only=bool(args.baseline))
    where = {}
    if args.heights:
        grid, curriculum, _ = terrain_grid(n, args.max_init_level, dev, cfg.episode_length_s)
        where = dict(terrain=grid.terrain, origin=curriculum().origins0)

    def make_task(with_privileged):
        opts = dict(where)
        if args.heights:
            from rl_mpc_locomotion_amd.height_scan import HeightScan
            opts["height_scan"] = HeightScan(n, device=dev)
        if with_privileged:
            from rl_mpc_locomotion_amd.privileged_obs import PrivilegedObs
            opts["privileged_obs"] = PrivilegedObs(n, device=dev)
        return make(n, dev, cfg, **opts)
    loops = {"step_without": make_task(False)} if args.baseline else {"step_with_privileged": make_task(True), "step_without": make_task(False)}
    blocks(res, args, actions, loops)
    res["after_timing"] = {"fallen_fraction": fallen(loops)}
    if not args.baseline:
        task = loops["step_with_privileged"]
        keys = {"finish_kernel": "finish", "assembly_kernel": "privileged_obs"}
        if args.heights:
            keys["scan_kernel"] = "height_scan"
        p = stages(res, args, actions, task, keys)
        res["share_of_the_tick"] = {"assembly_kernel_median_us": p["assembly_kernel"] * 1e3,
                                    "assembly_over_step_without": p["assembly_kernel"] / res["step_without"]["ms_per_tick_median"],
                                    "assembly_over_finish_median": p["assembly_kernel"] / p["finish_kernel"],
                                    "measured_step_difference_over_step_without": res["with_over_without_ms_per_tick"] - 1.0}
        # the bytes the algorithm needs, from the shapes: the live columns read, four contact words and one counter per environment, the whole row written
        wp, live = task.num_privileged_obs, 48 + (task.height_scan.num_points if args.heights else 0)
        moved = n * live * 4 + n * 4 * 4 + n * 8 + n * wp * 4
        res["assembly_bytes"] = {"actor_columns": task.num_obs, "privileged_columns": wp, "row_writes": n * wp * 4, "all_reads_and_writes": moved,
                                 **hbm(moved, p["assembly_kernel"])}
        rows = task.privileged_obs_buf
        res["after_timing"]["privileged_row"] = {"contact_mean": float(rows[:, live:live + 4].mean().item()), "phase_max": float(rows[:, live + 4].max().item()),
                                                  "equals_the_actor_row_in_the_live_columns": bool(torch.equal(rows[:, :live], task.obs_buf[:, :live]))}
    clock(res, "after")
    return res


def plant_rand_report(args, dev, n, actions):
    """The step, and its controller, plant and resets stages, with and without the per-robot plant record: whole ticks in alternating blocks, then the
    stages from events, the tasks alternating round by round.  A third task carries the record and never randomises it (no ranges: every draw writes
    the neutral values): it runs the parametrised kernel and the draw on robots that stay alike, which separates what the kernel costs from what
    robots that differ cost (lanes of a wave that disagree on a foot's contact run both branches, and the solver's iteration counts differ).
    --privileged: all three assemble the critic's row, the first two with the plant columns."""
    from rl_mpc_locomotion_amd.plant_rand import PlantRand, PlantSpec
    cfg = TaskConfig(**CFG)
    res = header(args, n, privileged=bool(args.privileged), ranges=PLANT_RANGES)

    def make_task(spec):
        opts = {}
        if spec is not None:
            opts["plant_rand"] = PlantRand(n, spec, seed=0, device=dev)
        if args.privileged:
            from rl_mpc_locomotion_amd.privileged_obs import PrivilegedObs
            opts["privileged_obs"] = PrivilegedObs(n, device=dev, plant=spec is not None)
        return make(n, dev, cfg, **opts)
    loops = {"step_with_plant_rand": make_task(PlantSpec(**PLANT_RANGES)), "step_with_neutral_record": make_task(PlantSpec()), "step_without": make_task(None)}
    blocks(res, args, actions, loops)
    without = res["step_without"]["ms_per_tick_median"]
    res["over_step_without_ms_per_tick"] = {k: res[k]["ms_per_tick_median"] / without for k in loops}
    names = ("controller", "plant", "resets") + (("privileged_obs",) if args.privileged else ())
    parts = {k: {s: [] for s in names} for k in loops}
    for _ in range(args.blocks):
        for k, task in loops.items():
            got = stage_times(task, actions, max(args.ticks // 2, 1))
            for s in names:
                parts[k][s] += list(got[s])
    res["stages"] = {k: {s: {**spread(v), "events": len(v)} for s, v in d.items()} for k, d in parts.items()}
    res["over_without_stage_median"] = {k: {s: med(parts[k][s]) / med(parts["step_without"][s]) for s in names} for k in loops}
    task = loops["step_with_plant_rand"]
    rec = task.plant_rand.get_params()
    res["after_timing"] = {"fallen_fraction": fallen(loops), "draw_launches": task.plant_rand.launches,
                           "draws_per_environment_mean": float(task.plant_rand.get_counters().mean()), "record_min": rec.min(0).tolist(), "record_max": rec.max(0).tolist(),
                           "neutral_record_stayed_neutral": bool((loops["step_with_neutral_record"].plant_rand.get_params() == np.array([0.0, 1.0, -9.81])).all())}
    clock(res, "after")
    return res


# --shaping: every term live (the values are of legged_gym's order of magnitude; none is a preset)
SHAPING_SCALES = dict(orientation=-0.2, base_height=-1.0, dof_vel=-1e-4, dof_acc=-2.5e-7, action_rate=-0.01, feet_air_time=1.0, stand_still=-0.1, termination=-2.0,
                      base_height_target=0.3)


def shaping_task(args, dev, n, cfg, with_shaping=True):
    """The task --shaping times: on the terrain grid with the scan with --heights, beside the episode sums with --terms."""
    from rl_mpc_locomotion_amd.reward_shaping import RewardShaping, ShapingSpec
    opts = {}
    if args.heights:
        from rl_mpc_locomotion_amd.height_scan import HeightScan
        grid, curriculum, _ = terrain_grid(n, args.max_init_level, dev, cfg.episode_length_s)
        opts.update(terrain=grid.terrain, origin=curriculum().origins0, height_scan=HeightScan(n, device=dev))
    if args.terms:
        from rl_mpc_locomotion_amd.episode_terms import EpisodeTerms
        opts["episode_terms"] = EpisodeTerms(n, cfg, device=dev)
    if with_shaping:
        opts["reward_shaping"] = RewardShaping(n, ShapingSpec(**SHAPING_SCALES), device=dev, cfg=cfg)
    return make(n, dev, cfg, **opts)


def shaping_report(args, dev, n, actions):
    from rl_mpc_locomotion_amd.reward_shaping import RewardShaping
    cfg = TaskConfig(**CFG, episode_length_s=args.episode_s)
    res = header(args, n, heights=bool(args.heights), terms=bool(args.terms), episode_length_s=cfg.episode_length_s, scales=SHAPING_SCALES,
                 launches_per_tick={"close": 2, "run": 1})
    loops = {"step_with_shaping": shaping_task(args, dev, n, cfg), "step_without": shaping_task(args, dev, n, cfg, with_shaping=False)}
    blocks(res, args, actions, loops, per_block=True)
    added = (np.array(res["step_with_shaping"]["ms_per_tick_blocks"]) - np.array(res["step_without"]["ms_per_tick_blocks"])) * 1e3
    res["added_us_per_tick"] = {"p10": float(np.percentile(added, 10)), "median": med(added), "p90": float(np.percentile(added, 90)), "blocks": added.tolist()}
    run_stage = "height_scan" if args.heights else "finish"
    names = ("resets", run_stage) + (("episode_close", "episode_accumulate") if args.terms else ())
    parts = {k: {s: [] for s in names} for k in loops}
    for _ in range(args.blocks):              # the stages from events, the tasks alternating round by round
        for k, task in loops.items():
            got = stage_times(task, actions, max(args.ticks // 2, 1))
            for s in names:
                parts[k][s] += list(got[s])
    res["stages"] = {k: {s: {**spread(v), "events": len(v)} for s, v in d.items()} for k, d in parts.items()}
    m = {k: {s: med(v) for s, v in d.items()} for k, d in parts.items()}
    unit = sum(m["step_with_shaping"][s] - m["step_without"][s] for s in ("resets", run_stage))
    res["unit_from_stage_medians_us"] = {"close_in_resets": (m["step_with_shaping"]["resets"] - m["step_without"]["resets"]) * 1e3,
                                         "run_in_" + run_stage: (m["step_with_shaping"][run_stage] - m["step_without"][run_stage]) * 1e3, "both": unit * 1e3}
    if args.terms:
        both = np.array(parts["step_with_shaping"]["episode_close"]) + np.array(parts["step_with_shaping"]["episode_accumulate"])
        res["episode_terms_yardstick_us"] = {"p10": float(np.percentile(both, 10)) * 1e3, "median": med(both) * 1e3, "p90": float(np.percentile(both, 90)) * 1e3}
        y = res["episode_terms_yardstick_us"]
        res["unit_exceeds_yardstick_by_more_than_its_spread"] = bool(res["added_us_per_tick"]["median"] - y["median"] > y["p90"] - y["p10"])
    rs = loops["step_with_shaping"].reward_shaping
    res["after_timing"] = {"fallen_fraction": fallen(loops), "record": RewardShaping.record(rs.summary().tolist())}
    clock(res, "after")
    return res


# --contact: every term live (the values are of legged_gym's order of magnitude; none is a preset), and the friction range of the timed plants
CONTACT_SCALES = dict(feet_slip=-0.1, feet_contact_forces=-0.01, feet_stumble=-0.5, max_contact_force=100.0)
CONTACT_FRICTION = dict(range=(0.2, 1.25), buckets=64, resample="reset")


def contact_task(args, dev, n, cfg, with_contact=True, with_shaping=True):
    """The task --contact times: a plant with friction drawn at resets; --shaping, --heights, --terms and --privileged as they are given."""
    from rl_mpc_locomotion_amd.contact_terms import ContactSpec, ContactTerms
    from rl_mpc_locomotion_amd.friction import Friction, FrictionSpec
    opts = dict(friction=Friction(n, FrictionSpec(**CONTACT_FRICTION), seed=3, device=dev))
    if args.heights:
        from rl_mpc_locomotion_amd.height_scan import HeightScan
        grid, curriculum, _ = terrain_grid(n, args.max_init_level, dev, cfg.episode_length_s)
        opts.update(terrain=grid.terrain, origin=curriculum().origins0, height_scan=HeightScan(n, device=dev))
    if args.terms:
        from rl_mpc_locomotion_amd.episode_terms import EpisodeTerms
        opts["episode_terms"] = EpisodeTerms(n, cfg, device=dev)
    if args.shaping and with_shaping:
        from rl_mpc_locomotion_amd.reward_shaping import RewardShaping, ShapingSpec
        opts["reward_shaping"] = RewardShaping(n, ShapingSpec(**SHAPING_SCALES), device=dev, cfg=cfg)
    if args.privileged:
        from rl_mpc_locomotion_amd.privileged_obs import PrivilegedObs
        opts["privileged_obs"] = PrivilegedObs(n, device=dev)
    if with_contact:
        opts["contact_terms"] = ContactTerms(n, ContactSpec(**CONTACT_SCALES), device=dev, cfg=cfg, privileged=bool(args.privileged))
    return make(n, dev, cfg, **opts)


def contact_report(args, dev, n, actions):
    from rl_mpc_locomotion_amd.contact_terms import ContactTerms
    cfg = TaskConfig(**CFG, episode_length_s=args.episode_s)
    res = header(args, n, heights=bool(args.heights), terms=bool(args.terms), shaping=bool(args.shaping), privileged=bool(args.privileged),
                 episode_length_s=cfg.episode_length_s, scales=CONTACT_SCALES, friction=CONTACT_FRICTION,
                 launches_per_tick={"close": 2, "run": 1, "extend": 1 if args.privileged else 0})
    loops = {"step_with_contact": contact_task(args, dev, n, cfg), "step_without": contact_task(args, dev, n, cfg, with_contact=False)}
    if args.shaping:                          # the yardstick's baseline: neither unit
        loops["step_without_shaping"] = contact_task(args, dev, n, cfg, with_contact=False, with_shaping=False)
    blocks(res, args, actions, loops, per_block=True)
    per = {k: np.array(res[k]["ms_per_tick_blocks"]) * 1e3 for k in loops}
    pct = lambda v: {"p10": float(np.percentile(v, 10)), "median": med(v), "p90": float(np.percentile(v, 90)), "blocks": v.tolist()}
    res["added_us_per_tick"] = pct(per["step_with_contact"] - per["step_without"])
    run_stage = "height_scan" if args.heights and args.shaping else "finish"
    names = ("resets", run_stage) + (("privileged_obs",) if args.privileged else ())
    parts = {k: {s: [] for s in names} for k in loops}
    for _ in range(args.blocks):              # the stages from events, the tasks alternating round by round
        for k, task in loops.items():
            got = stage_times(task, actions, max(args.ticks // 2, 1))
            for s in names:
                parts[k][s] += list(got[s])
    res["stages"] = {k: {s: {**spread(v), "events": len(v)} for s, v in d.items()} for k, d in parts.items()}
    m = {k: {s: med(v) for s, v in d.items()} for k, d in parts.items()}
    diff = lambda a, b, s: (m[a][s] - m[b][s]) * 1e3
    unit = {"close_in_resets": diff("step_with_contact", "step_without", "resets"), "run_in_" + run_stage: diff("step_with_contact", "step_without", run_stage)}
    unit["close_and_run"] = unit["close_in_resets"] + unit["run_in_" + run_stage]
    if args.privileged:
        unit["extend_in_privileged_obs"] = diff("step_with_contact", "step_without", "privileged_obs")
    res["unit_from_stage_medians_us"] = unit
    if args.shaping:                          # reward_shaping's three launches, in the same run: from the blocks and from the two stages that hold them
        y = pct(per["step_without"] - per["step_without_shaping"])
        y["from_stage_medians"] = diff("step_without", "step_without_shaping", "resets") + diff("step_without", "step_without_shaping", run_stage)
        res["reward_shaping_yardstick_us"] = y
        res["close_and_run_exceed_yardstick_by_more_than_its_spread"] = bool(unit["close_and_run"] - y["from_stage_medians"] > y["p90"] - y["p10"])
    ct = loops["step_with_contact"].contact_terms
    res["after_timing"] = {"fallen_fraction": fallen(loops), "record": ContactTerms.record(ct.summary().tolist())}
    clock(res, "after")
    return res


def default_report(args, dev, n, actions):
    res = header(args, n)
    step, half, bare = make(n, dev), make(n, dev), Bare(n, dev)
    for task in (step, half):
        task.reset()
    res.update(wall_blocks({"step": lambda: step.step(actions), "torch_half": lambda: tick_torch(half, actions), "controller_and_plant": bare.tick},
                           args.ticks, args.blocks, n))
    # the parts, from events inside the running loops
    names = {"controller_ms": "controller", "plant_ms": "plant", "begin_kernel_ms": "begin", "device_resets_ms": "resets", "finish_kernel_ms": "finish"}
    parts = stage_times(step, actions, args.ticks)
    pairs = [(ev(), ev()) for _ in range(args.ticks * 2)]
    for e in pairs:
        tick_torch(half, actions, e)
    torch.cuda.synchronize()
    th = np.array([a.elapsed_time(b) for a, b in pairs])
    fused = parts["begin"] + parts["resets"] + parts["finish"]
    res["parts_median_of_ticks"] = {**{nm: med(parts[stage]) for nm, stage in names.items()}, "fused_half_ms": med(fused), "torch_half_ms": med(th),
                                    "events": len(pairs)}
    res["added_per_tick_share_of_controller_step"] = med(fused) / med(parts["controller"])
    res["fused_half_over_torch_half"] = med(fused) / med(th)
    res["step_over_controller_and_plant_rate"] = res["step"]["robot_ticks_per_s"] / res["controller_and_plant"]["robot_ticks_per_s"]
    res["step_over_torch_half_rate"] = res["step"]["robot_ticks_per_s"] / res["torch_half"]["robot_ticks_per_s"]
    res["fallen_fraction"] = fallen({"step": step, "torch_half": half, "controller_and_plant": bare})
    clock(res, "after")
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
    ap.add_argument("--plant-rand", action="store_true", help="time the step and its plant and resets stages with and without the per-robot plant record; with --privileged both tasks assemble the critic's row, one with the plant columns")
    ap.add_argument("--shaping", action="store_true", help="time the step with and without the reward shaping terms; with --heights on the terrain with the scan, with --terms beside the episode sums")
    ap.add_argument("--contact", action="store_true", help="time the step with and without the contact terms on a plant with friction; --shaping, --heights, --terms and --privileged are honoured")
    ap.add_argument("--out")
    args = ap.parse_args()
    dev, n = "cuda:0", args.robots
    actions = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    if args.quick and args.contact:        # one block of the step with the option (for a kernel trace)
        task = contact_task(args, dev, n, TaskConfig(**CFG, episode_length_s=args.episode_s))
        task.reset()
        for _ in range(args.ticks):
            task.step(actions)
        torch.cuda.synchronize()
        sys.exit(0)
    if args.quick and args.shaping:        # one block of the step with the option, --heights and --terms honoured (for a kernel trace)
        task = shaping_task(args, dev, n, TaskConfig(**CFG, episode_length_s=args.episode_s))
        task.reset()
        for _ in range(args.ticks):
            task.step(actions)
        torch.cuda.synchronize()
        sys.exit(0)
    if args.quick and not (args.plant_rand or args.privileged or args.terms or args.domain_rand or args.heights or args.curriculum):
        task = make(n, dev)
        task.reset()
        for _ in range(args.ticks):
            task.step(actions)
        torch.cuda.synchronize()
        sys.exit(0)
    report = (contact_report if args.contact else shaping_report if args.shaping else plant_rand_report if args.plant_rand else privileged_report if args.privileged else terms_report if args.terms else domain_rand_report if args.domain_rand else heights_report if args.heights
              else curriculum_report if args.curriculum else default_report)
    emit(report(args, dev, n, actions), args.out)
