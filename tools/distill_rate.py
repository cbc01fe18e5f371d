"""What policy distillation costs at the training shape: 4096 Aliengo robots trotting on the terrain grid, h = 10, T = 24, the reference's nets, the
task with the default height scan and privileged rows (240 columns each).  Two measurements by the host clock, each over loops that alternate block
by block in one process (_rate.wall_blocks):

* one ``Distillation.update`` (5 epochs x 4 mini-batches of 24 576 rows) with each backend -- torch autograd + Adam on the device, and the device update
  of include/mpc_ppo_update.h (``backend="hip"``) -- on two students with the same initial weights and ONE storage, filled by a real collection;
* one collection launch: ``mpc_ac_act_distill`` (the student samples, the teacher labels) against ``mpc_ac_act_asymmetric`` on the same student (the
  student samples, its critic values the privileged rows), both into the same slot.

    python tools/distill_rate.py [--ticks 4] [--blocks 7] [--out profiles/distill_rate.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_mpc_locomotion_amd  # noqa: E402,F401
from _rate import clock, emit, header, terrain_grid, wall_blocks  # noqa: E402
from rl_mpc_locomotion_amd.distill import DistillConfig, Distillation, Distiller, act_distill  # noqa: E402
from rl_mpc_locomotion_amd.height_scan import HeightScan  # noqa: E402
from rl_mpc_locomotion_amd.ppo import ActorCritic, PPOConfig  # noqa: E402
from rl_mpc_locomotion_amd.privileged_obs import PrivilegedObs  # noqa: E402
from rl_mpc_locomotion_amd.rl_task import BatchedRLTask, TaskConfig  # noqa: E402

TROT = 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=4, help="updates per block (the act loops run 50 x as many launches)")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, n = torch.device("cuda:0"), args.robots
    cfg, tcfg = DistillConfig(), TaskConfig()
    grid, curriculum, grid_record = terrain_grid(n, 9, dev, tcfg.episode_length_s)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    env = BatchedRLTask([0] * n, [TROT] * n, cfg=tcfg, horizon=10, yaw0=yaw, flat_ground=True, device=dev, terrain=grid.terrain, origin=curriculum().origins0,
                        height_scan=HeightScan(n, device=dev), privileged_obs=PrivilegedObs(n, device=dev))
    torch.manual_seed(1)
    ref = PPOConfig()
    teacher = ActorCritic(env.num_privileged_obs, 12, ref.actor_hidden_dims, ref.critic_hidden_dims)
    runner = Distiller(env, teacher, cfg, seed=1, update="hip")
    runner.collect()                                                             # a real storage: rows, the student's actions, the teacher's labels
    st = runner.storage
    twin = ActorCritic(env.num_obs, 12, cfg.actor_hidden_dims, cfg.critic_hidden_dims, init_noise_std=cfg.student_noise_std,
                       num_critic_obs=env.num_privileged_obs).to(dev)
    twin.load_state_dict(runner.actor_critic.state_dict())
    students = {"hip": runner.actor_critic, "torch": twin}
    algs = {"hip": runner.alg, "torch": Distillation(students["torch"], cfg, backend="torch")}
    res = header(args, n, num_steps_per_env=st.T, mini_batches_per_update=cfg.num_learning_epochs * cfg.num_mini_batches,
                 rows_per_mini_batch=st.n * st.T // cfg.num_mini_batches, loss_type=cfg.loss_type, terrain=grid_record,
                 columns={"student": env.num_obs, "teacher": env.num_privileged_obs}, actor_hidden_dims=list(cfg.actor_hidden_dims))
    up = wall_blocks({name: (lambda a=alg: a.update(st)) for name, alg in algs.items()}, args.ticks, args.blocks, n, warmup=2, per_block=True)
    for name in up:
        up[name]["ms_per_update_median"] = up[name].pop("ms_per_tick_median")
        up[name].pop("robot_ticks_per_s")
    res["update"] = up
    res["update"]["torch_over_hip"] = up["torch"]["ms_per_update_median"] / up["hip"]["ms_per_update_median"]
    # the collection launch, into slot 0 of the storage and of a twin for the asymmetric launch's outputs
    student, obs, priv = students["hip"], st.observations[1].contiguous(), env.privileged_obs_buf
    slot = st.slot(0)
    plain = dict(actions=st.actions[0], mu=st.mu[0], sigma=st.sigma[0], actions_log_prob=torch.empty((n, 1), device=dev), values=torch.empty((n, 1), device=dev))
    act = wall_blocks({"act_distill": lambda: act_distill(student, runner.teacher, obs, priv, 1, 0, out=slot),
                       "act_asymmetric": lambda: student.act(obs, 1, 0, out=plain, critic_obs=priv)}, 50 * args.ticks, args.blocks, n, warmup=20, per_block=True)
    res["act"] = act
    res["act"]["distill_over_asymmetric"] = act["act_distill"]["ms_per_tick_median"] / act["act_asymmetric"]["ms_per_tick_median"]
    clock(res, "after")
    emit(res, args.out)


if __name__ == "__main__":
    main()
