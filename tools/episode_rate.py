"""What the device-side episode statistics cost, and what an evaluation run shows.

Timing (the default): 4096 Aliengo robots trotting, h = 10.  One 24-tick collection's (rew, reset, time_outs) are recorded, then per repeat and
alternating in one process, each tick timed with HIP events: `EpisodeStats.add` (three launches) and rsl_rl's
torch composition on the same buffers (the two `+=`, `nonzero`, the `.cpu().numpy().tolist()` extends of two deque(maxlen=100), the two zeroings --
with the host round trip it needs).  Medians with p10 .. p90 over ticks x repeats; 24 `add` beside the measured collection; the shader clock before
and after, as bench.py --full records it.
    python tools/episode_rate.py [--repeats 7]          (writes profiles/r12_episode_stats.json unless --out names another file)
Evaluation: `--terrain reference|mild|none --iterations K` trains K iterations (`learn(K, init_at_random_ep_len=True)`, the device update) on three
robot types with `PPOTrainer.evaluate` before and after, and reports per robot type the terminations, their fraction of the finished episodes and the
mean episode length.  `--merge` adds the result to an existing --out file instead of replacing it."""
import argparse
import json
import os
import sys
from collections import deque

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_mpc_locomotion_amd  # noqa: E402,F401
from _rate import ev, stats  # noqa: E402
from rl_mpc_locomotion_amd import _lib, episode as E  # noqa: E402
from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer  # noqa: E402
from rl_mpc_locomotion_amd.rl_task import BatchedRLTask, TaskConfig  # noqa: E402
from rl_mpc_locomotion_amd.terrain import Terrain, spread_origins  # noqa: E402

TROT = 0
ACT_PLUS_ADD_US = 69.3                 # DESIGN 8.3 (profiles/r09_ppo.json): `act` + `RolloutStorage.add` per tick


class TorchRunner:
    """rsl_rl's lines of OnPolicyRunner.learn."""

    def __init__(self, n, dev):
        self.rewbuffer, self.lenbuffer = deque(maxlen=100), deque(maxlen=100)
        self.cur_reward_sum = torch.zeros(n, dtype=torch.float, device=dev)
        self.cur_episode_length = torch.zeros(n, dtype=torch.float, device=dev)

    def add(self, rewards, dones):
        self.cur_reward_sum += rewards
        self.cur_episode_length += 1
        new_ids = (dones > 0).nonzero(as_tuple=False)
        self.rewbuffer.extend(self.cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
        self.lenbuffer.extend(self.cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
        self.cur_reward_sum[new_ids] = 0
        self.cur_episode_length[new_ids] = 0


def timing(args, dev):
    from bench import device_state
    n = args.robots
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    env = BatchedRLTask([0] * n, [TROT] * n, cfg=TaskConfig(), horizon=10, yaw0=yaw, flat_ground=True, device=dev)
    cfg = PPOConfig()
    T = cfg.num_steps_per_env
    trainer = PPOTrainer(env, cfg, seed=1, update="hip")
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats, "window": 100,
           "device_state": {"before": device_state(0, smi=False)}}
    trainer.learn(2, init_at_random_ep_len=True)                                 # warm-up: cold solves, code objects
    # one collection's ticks as the task wrote them
    ticks = []
    with torch.no_grad():
        for t in range(T):
            trainer.obs, rew, reset, extras = env.step(trainer.actor_critic.act(trainer.obs, 1, 10 ** 6 + t)["actions"])
            ticks.append((rew.clone(), reset.clone(), extras["time_outs"].clone()))
    finished = torch.stack([(r > 0).sum() for _, r, _ in ticks]).tolist()
    res["finished_per_recorded_tick"] = finished
    sides = {"device": E.EpisodeStats(n, device=dev), "torch": TorchRunner(n, dev)}
    for s in sides.values():                                                     # warm-up of each side
        for rew, reset, to in ticks:
            s.add(rew, reset) if isinstance(s, TorchRunner) else s.add(rew, reset, to)
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    order = list(sides)
    for rep in range(args.repeats):
        for name in order[rep % 2:] + order[:rep % 2]:                           # which side goes first alternates
            s = sides[name]
            e = [[ev(), ev()] for _ in range(T)]
            for t, (rew, reset, to) in enumerate(ticks):
                e[t][0].record()
                s.add(rew, reset) if name == "torch" else s.add(rew, reset, to)
                e[t][1].record()
            torch.cuda.synchronize()
            times[name].extend(a.elapsed_time(b) for a, b in e)
    res["add_per_tick"] = {k: stats(v) for k, v in times.items()}
    t_collect = []
    for rep in range(args.repeats):
        x, y = ev(), ev()
        x.record()
        trainer.collect()
        y.record()
        torch.cuda.synchronize()
        t_collect.append(x.elapsed_time(y))
    res["collection_24_ticks"] = stats(t_collect)
    m = lambda k: res["add_per_tick"][k]["median_ms"]
    d, t = res["add_per_tick"]["device"], res["add_per_tick"]["torch"]
    res["device_over_torch"] = d["median_ms"] / t["median_ms"]
    res["device_p90_below_torch_p10"] = d["p90_ms"] < t["p10_ms"]
    res["share_of_act_plus_add_tick"] = m("device") * 1e3 / ACT_PLUS_ADD_US
    res["adds_per_iteration_ms"] = T * m("device")
    res["share_of_collection"] = T * m("device") / res["collection_24_ticks"]["median_ms"]
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def evaluation(args, dev):
    n = args.robots
    robot_type = [i % 3 for i in range(n)]
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    ground = {}
    if args.terrain != "none":
        t = Terrain.reference(0) if args.terrain == "reference" else Terrain.mild(0)
        ground = dict(terrain=t, origin=spread_origins(n, t, margin=3.0))
    env = BatchedRLTask(robot_type, [TROT] * n, cfg=TaskConfig(), horizon=10, yaw0=yaw, flat_ground=args.terrain == "none", device=dev, **ground)
    trainer = PPOTrainer(env, PPOConfig(), seed=1, update="hip")

    def evaluate():
        out = trainer.evaluate(args.eval_ticks, groups=robot_type, num_groups=3)
        per = lambda g, robots: dict(g, termination_fraction_of_episodes=g["terminations"] / g["episodes"] if g["episodes"] else None,
                                     terminations_per_robot=g["terminations"] / robots)
        return dict(per({k: v for k, v in out.items() if k != "groups"}, n),
                    per_robot_type={str(k): per(g, robot_type.count(k)) for k, g in enumerate(out["groups"])})
    res = {"terrain": args.terrain, "robots": n, "iterations": args.iterations, "eval_ticks": args.eval_ticks, "max_episode_length": env.cfg.max_episode_length,
           "before": evaluate()}
    infos = trainer.learn(args.iterations, init_at_random_ep_len=True)
    res["training"] = [{k: i[k] for k in ("iter", "mean_reward", "mean_episode_return", "mean_episode_length", "episodes_finished", "timeouts_in_window")}
                       for i in infos[::max(1, len(infos) // 10)]]
    res["after"] = evaluate()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--terrain", choices=("reference", "mild", "none"))
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--eval-ticks", type=int, default=500)
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_episode_stats.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("episode_rate.py measures on the GPU; none is visible")
    if args.terrain:
        res = {"evaluation_" + args.terrain: evaluation(args, "cuda:0")}
    else:
        res = timing(args, "cuda:0")
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if args.merge and os.path.exists(args.out):
            with open(args.out) as fh:
                res = dict(json.load(fh), **res)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
