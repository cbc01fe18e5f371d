"""What running observation normalisation costs per tick, and what it does to training on terrain.

Timing (the default): 4096 Aliengo robots trotting, h = 10.  The observations of one 24-tick collection are recorded, then per repeat and alternating in
one process, each tick timed with HIP events: `ObsNormalizer.__call__` (update, then normalise: three launches, into a second buffer as the trainer writes a
storage slot) and the torch composition of the same formulas (rsl_rl 2.x's EmpiricalNormalization.update and forward on float32 device tensors: count,
rate, mean, var(unbiased=False), the two in-place updates, sqrt, and (x - mean) / (std + eps)).  Medians with p10 .. p90 over ticks x repeats, the
normalise-only call (update=False) beside them, 24 calls beside a measured collection with and without normalisation; the shader clock before and after, as
bench.py --full records it.
    python tools/obs_norm_rate.py [--repeats 7]          (writes profiles/r13_obs_norm.json unless --out names another file)
Evaluation: `--terrain reference|mild|none --iterations K` runs DESIGN 8.3.1's terrain evaluation twice from the same seed, without and with
`normalize_obs=True`: `evaluate(500)` before and after `learn(K, init_at_random_ep_len=True)` with the device update on three robot types, and reports per
robot type the terminations per robot and the mean episode length.  `--merge` adds the result to an existing --out file instead of replacing it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_mpc_locomotion_amd  # noqa: E402,F401
from _rate import ev, stats  # noqa: E402
from rl_mpc_locomotion_amd import _lib  # noqa: E402
from rl_mpc_locomotion_amd.obs_norm import ObsNormalizer  # noqa: E402
from rl_mpc_locomotion_amd.ppo import PPOConfig, PPOTrainer  # noqa: E402
from rl_mpc_locomotion_amd.rl_task import BatchedRLTask, TaskConfig  # noqa: E402
from rl_mpc_locomotion_amd.terrain import Terrain, spread_origins  # noqa: E402

TROT = 0
ACT_PLUS_ADD_US = 69.3                 # DESIGN 8.3 (profiles/r09_ppo.json): `act` + `RolloutStorage.add` per tick


class TorchNormalizer:
    """rsl_rl 2.x's EmpiricalNormalization, training mode, by its published formulas."""

    def __init__(self, D, dev, eps=1e-2):
        self.eps = eps
        self._mean, self._var, self._std = torch.zeros((1, D), device=dev), torch.ones((1, D), device=dev), torch.ones((1, D), device=dev)
        self.count = torch.tensor(0, dtype=torch.long, device=dev)

    def __call__(self, x, out=None):
        count_x = x.shape[0]
        self.count += count_x
        rate = count_x / self.count
        var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(x, dim=0, keepdim=True)
        delta_mean = mean_x - self._mean
        self._mean += rate * delta_mean
        self._var += rate * (var_x - self._var + delta_mean * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)
        return torch.div(x - self._mean, self._std + self.eps, out=out)


def make_env(n, robot_type, terrain, dev):
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    ground = {}
    if terrain != "none":
        t = Terrain.reference(0) if terrain == "reference" else Terrain.mild(0)
        ground = dict(terrain=t, origin=spread_origins(n, t, margin=3.0))
    return BatchedRLTask(robot_type, [TROT] * n, cfg=TaskConfig(), horizon=10, yaw0=yaw, flat_ground=terrain == "none", device=dev, **ground)


def timing(args, dev):
    from bench import device_state
    n = args.robots
    cfg = PPOConfig()
    T = cfg.num_steps_per_env
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats, "eps": 1e-2,
           "device_state": {"before": device_state(0, smi=False)}}
    collections = {}
    ticks = None
    for on in (False, True):
        trainer = PPOTrainer(make_env(n, [0] * n, "none", dev), cfg, seed=1, update="hip", normalize_obs=on)
        trainer.learn(2, init_at_random_ep_len=True)                             # warm-up: cold solves, code objects
        t_collect = []
        for rep in range(args.repeats):
            x, y = ev(), ev()
            x.record()
            trainer.collect()
            y.record()
            torch.cuda.synchronize()
            t_collect.append(x.elapsed_time(y))
        collections["normalize_obs" if on else "plain"] = stats(t_collect)
        if not on:                                                               # one collection's raw observations as the task wrote them
            ticks = []
            with torch.no_grad():
                for t in range(T):
                    trainer.obs = trainer.env.step(trainer.actor_critic.act(trainer.obs, 1, 10 ** 6 + t)["actions"])[0]
                    ticks.append(trainer.obs.clone())
        del trainer
    res["collection_24_ticks"] = collections
    D = ticks[0].shape[1]
    res["num_obs"] = D
    res["recorded_abs_max_per_tick"] = torch.stack([x.abs().max() for x in ticks]).tolist()
    out = torch.empty_like(ticks[0])
    sides = {"device": ObsNormalizer(D, device=dev), "torch": TorchNormalizer(D, dev)}
    for s in sides.values():                                                     # warm-up of each side
        for x in ticks:
            s(x, out=out)
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    times["device_normalize_only"] = []
    order = list(sides)
    for rep in range(args.repeats):
        for name in order[rep % 2:] + order[:rep % 2]:                           # which side goes first alternates
            s = sides[name]
            e = [[ev(), ev()] for _ in range(T)]
            for t, x in enumerate(ticks):
                e[t][0].record()
                s(x, out=out)
                e[t][1].record()
            torch.cuda.synchronize()
            times[name].extend(a.elapsed_time(b) for a, b in e)
        e = [[ev(), ev()] for _ in range(T)]
        for t, x in enumerate(ticks):
            e[t][0].record()
            sides["device"](x, out=out, update=False)
            e[t][1].record()
        torch.cuda.synchronize()
        times["device_normalize_only"].extend(a.elapsed_time(b) for a, b in e)
    res["per_tick"] = {k: stats(v) for k, v in times.items()}
    d, t = res["per_tick"]["device"], res["per_tick"]["torch"]
    res["agreement_with_torch_float32"] = {
        "mean_max_abs_diff": float((sides["device"]._mean - sides["torch"]._mean).abs().max()),
        "std_max_rel_diff": float(((sides["device"]._std - sides["torch"]._std).abs() / (sides["torch"]._std + 1e-2)).max())}
    res["device_over_torch"] = d["median_ms"] / t["median_ms"]
    res["device_p90_below_torch_p10"] = d["p90_ms"] < t["p10_ms"]
    res["share_of_act_plus_add_tick"] = d["median_ms"] * 1e3 / ACT_PLUS_ADD_US
    res["calls_per_iteration_ms"] = (T + 1) * d["median_ms"]
    res["share_of_collection"] = (T + 1) * d["median_ms"] / collections["normalize_obs"]["median_ms"]
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def evaluation(args, dev):
    n = args.robots
    robot_type = [i % 3 for i in range(n)]
    res = {"terrain": args.terrain, "robots": n, "iterations": args.iterations, "eval_ticks": args.eval_ticks}
    for on in (False, True):
        env = make_env(n, robot_type, args.terrain, dev)
        trainer = PPOTrainer(env, PPOConfig(), seed=1, update="hip", normalize_obs=on)

        def evaluate():
            out = trainer.evaluate(args.eval_ticks, groups=robot_type, num_groups=3)
            per = lambda g, robots: dict(g, termination_fraction_of_episodes=g["terminations"] / g["episodes"] if g["episodes"] else None,
                                         terminations_per_robot=g["terminations"] / robots)
            return dict(per({k: v for k, v in out.items() if k != "groups"}, n),
                        per_robot_type={str(k): per(g, robot_type.count(k)) for k, g in enumerate(out["groups"])})
        run = {"max_episode_length": env.cfg.max_episode_length, "before": evaluate()}
        infos = trainer.learn(args.iterations, init_at_random_ep_len=True)
        run["training"] = [{k: i[k] for k in ("iter", "mean_reward", "mean_episode_return", "mean_episode_length", "episodes_finished", "timeouts_in_window")}
                           for i in infos[::max(1, len(infos) // 10)]]
        run["after"] = evaluate()
        if on:
            run["obs_norm"] = {"count": int(trainer.obs_norm.count), "mean": trainer.obs_norm._mean[0].tolist(), "std": trainer.obs_norm._std[0].tolist()}
        res["normalize_obs" if on else "plain"] = run
        del trainer, env
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--terrain", choices=("reference", "mild", "none"))
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--eval-ticks", type=int, default=500)
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_obs_norm.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("obs_norm_rate.py measures on the GPU; none is visible")
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
