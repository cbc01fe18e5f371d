"""What a PPO iteration costs: 4096 Aliengo robots trotting, h = 10, T = 24, the reference's nets (48-512-256-128-12 / -1).
Per tick, from HIP events (median over ticks x repeats): `ActorCritic.act` (one launch), `RolloutStorage.add` (the observation copy + one kernel); per
iteration: `evaluate` + `compute_returns`, the whole 24-tick collection with `BatchedRLTask.step` inside, 24 bare `step`s, the update with each
backend (torch autograd + Adam, and the device update of include/mpc_ppo_update.h: `PPO(backend="hip")`) and one full iteration with each, the two
backends alternating repeat by repeat on the same actor-critic and storage.  In the same call, alternating repeat by repeat, the TORCH COMPOSITION of the collection half on the same buffers: the two
nn.Sequential, Normal(...).sample / log_prob, the storage copies, the time-out bootstrap and rsl_rl's GAE loop.  The shader clock is recorded as
bench.py --full records it (device_state).
    python tools/ppo_rate.py [--repeats 7] [--out profiles/r10_ppo_update.json]
--privileged times one iteration (collection, update, both) of the asymmetric actor-critic on a task with privileged observations against the symmetric
one on the same task without them, the two trainers alternating repeat by repeat in one process, with the device update: on the flat plane (48 actor
columns; 48 against 64 critic columns) or with --heights on the terrain grid (240 columns everywhere: the asymmetric path at equal widths).
--baseline times the symmetric trainer alone (it runs on a tree without the option, for a measurement of the parent commit in the same session).
    python tools/ppo_rate.py --privileged [--heights] [--baseline] [--out results/privileged_iteration.json]
--recurrent times the recurrent actor-critic (recurrent.py, an LSTM of --hidden state elements in front of each MLP) against the feed-forward one, the
two alternating block by block in one process: the cell launch alone, a recurrent `act` (cell launch + act launch) against the feed-forward `act`, and a
whole iteration (collection + torch update) of each trainer; the cell launch is reported as a share of the 0.82 ms control step and against the weight
bytes it streams.  --baseline times the feed-forward trainer alone.
    python tools/ppo_rate.py --recurrent [--hidden 256] [--baseline] [--out profiles/recurrent_rate.json]
--recurrent --through-time hip times the recurrent trainer with the memories' update through time on the device (RecurrentConfig(update_through_time="hip"),
csrc/recurrent_bptt.h) against the recurrent trainer with the torch update, the two alternating block by block in one process -- the "torch" trainer makes
the launches it made before the option existed -- : collection, update and whole iteration of each, and on one mini-batch of the "hip" trainer's storage
the forward launch, the whole backward call and the weight-gradient GEMMs with their reduction alone (the launch through time is the difference).
    python tools/ppo_rate.py --recurrent --through-time hip [--hidden 256] [--out profiles/recurrent_bptt_rate.json]
--recurrent --through-time hip --heads hip times the recurrent trainer with the whole update on the device (RecurrentConfig(update_through_time="hip",
update_heads="hip"): the MLPs, the loss head, the clip and Adam of include/mpc_ppo_update.h around the memories' roll) against the recurrent trainer with
update_heads="torch", which makes the launches it made before the option existed; the two alternate block by block in one process (_rate.wall_blocks,
one iteration per block): update and iteration from HIP events, the iteration also by the host clock, and the device memory behind the update.
    python tools/ppo_rate.py --recurrent --through-time hip --heads hip [--hidden 256] [--out profiles/recurrent_update_rate.json]
The kernel-trace stats: rocprofv3 --kernel-trace --stats ... -- python tools/ppo_rate.py --quick   (3 collections and one update per backend)"""
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
from rl_mpc_locomotion_amd.ppo import PPO, PPOConfig, PPOTrainer, RolloutStorage  # noqa: E402
from rl_mpc_locomotion_amd.rl_task import BatchedRLTask, TaskConfig  # noqa: E402

TROT = 0


def make_env(n, dev):
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    return BatchedRLTask([0] * n, [TROT] * n, cfg=TaskConfig(), horizon=10, yaw0=yaw, flat_ground=True, device=dev)


def torch_act(ac, st, t, obs):
    """rsl_rl's PPO.act: ActorCritic.act / evaluate and the copies of RolloutStorage.add_transitions"""
    with torch.no_grad():
        mean = ac.actor(obs)
        dist = torch.distributions.Normal(mean, mean * 0. + ac.std)
        actions = dist.sample()
        st.actions[t].copy_(actions)
        st.values[t].copy_(ac.critic(obs))
        st.actions_log_prob[t].copy_(dist.log_prob(actions).sum(dim=-1).view(-1, 1))
        st.mu[t].copy_(mean)
        st.sigma[t].copy_(dist.stddev)
        st.observations[t].copy_(obs)


def torch_add(st, t, rew, reset, time_outs, gamma):
    """rsl_rl's PPO.process_env_step: the time-out bootstrap and the two copies"""
    rewards = rew.clone()
    rewards += gamma * torch.squeeze(st.values[t] * time_outs.unsqueeze(1), 1)
    st.rewards[t].copy_(rewards.view(-1, 1))
    st.dones[t].copy_(reset.view(-1, 1))


def torch_returns(ac, st, obs, gamma, lam):
    """rsl_rl's evaluate + RolloutStorage.compute_returns"""
    with torch.no_grad():
        last_values = ac.critic(obs)
        advantage = 0
        for step in reversed(range(st.T)):
            next_values = last_values if step == st.T - 1 else st.values[step + 1]
            next_is_not_terminal = 1.0 - st.dones[step].float()
            delta = st.rewards[step] + next_is_not_terminal * gamma * next_values - st.values[step]
            advantage = delta + next_is_not_terminal * gamma * lam * advantage
            st.returns[step] = advantage + st.values[step]
        adv = st.returns - st.values
        st.advantages = (adv - adv.mean()) / (adv.std() + 1e-8)


def privileged_report(args, dev, n):
    from bench import device_state
    cfg = PPOConfig()
    T = cfg.num_steps_per_env
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    where = {}
    if args.heights:
        from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
        from rl_mpc_locomotion_amd.height_scan import HeightScan
        from rl_mpc_locomotion_amd.terrain import TerrainGrid
        grid = TerrainGrid(num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, seed=0)
        origins = TerrainCurriculum(grid, n, max_init_level=9, seed=0, device=dev, episode_length_s=TaskConfig().episode_length_s).origins0
        where = dict(terrain=grid.terrain, origin=origins)

    def make_task(with_privileged):
        opts = dict(where)
        if args.heights:
            opts["height_scan"] = HeightScan(n, device=dev)
        if with_privileged:
            from rl_mpc_locomotion_amd.privileged_obs import PrivilegedObs
            opts["privileged_obs"] = PrivilegedObs(n, device=dev)
        return BatchedRLTask([0] * n, [TROT] * n, cfg=TaskConfig(), horizon=10, yaw0=yaw, flat_ground=True, device=dev, **opts)
    trainers = {"symmetric": PPOTrainer(make_task(False), cfg, seed=1, update="hip")}
    if not args.baseline:
        trainers["asymmetric"] = PPOTrainer(make_task(True), cfg, seed=1, update="hip")
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats, "update": "hip",
           "heights": bool(args.heights), "baseline_only": bool(args.baseline), "mini_batches_per_update": cfg.num_learning_epochs * cfg.num_mini_batches,
           "columns": {k: {"actor": tr.actor_critic.actor[0].in_features, "critic": tr.actor_critic.critic[0].in_features} for k, tr in trainers.items()},
           "device_state": {"before": device_state(0)}}
    for tr in trainers.values():          # warm-up: cold solves, code objects, Adam's state, the update's workspace
        tr.learn(2)
    torch.cuda.synchronize()
    times = {k: {"collect": [], "update": [], "full": []} for k in trainers}
    names = list(trainers)
    for rep in range(args.repeats):       # which one goes first alternates
        for name in (names if rep % 2 == 0 else names[::-1]):
            tr = trainers[name]
            a, b, c = ev(), ev(), ev()
            a.record()
            tr.collect()
            b.record()
            tr.alg.update(tr.storage)
            c.record()
            torch.cuda.synchronize()
            tb = times[name]
            tb["collect"].append(a.elapsed_time(b)); tb["update"].append(b.elapsed_time(c)); tb["full"].append(a.elapsed_time(c))
    for name, tb in times.items():
        res[name] = {k: stats(v) for k, v in tb.items()}
        res[name]["robot_ticks_per_s_training"] = n * T / (float(np.median(tb["full"])) * 1e-3)
    if not args.baseline:
        res["asymmetric_over_symmetric_median"] = {k: res["asymmetric"][k]["median_ms"] / res["symmetric"][k]["median_ms"] for k in ("collect", "update", "full")}
        res["asymmetric_inside_symmetric_p10_p90"] = {k: bool(res["symmetric"][k]["p10_ms"] <= res["asymmetric"][k]["median_ms"] <= res["symmetric"][k]["p90_ms"])
                                                      for k in ("collect", "update", "full")}
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def recurrent_report(args, dev, n):
    """The recurrent actor-critic (recurrent.py) against the feed-forward one, in one process and alternating block by block: the cell launch alone, a
    recurrent ``act`` (cell launch + act launch) against the feed-forward ``act`` launch, and a whole iteration (collection + torch update) of each
    trainer.  The feed-forward trainer makes the launches it made before the option existed; --baseline times it alone."""
    from bench import device_state
    from rl_mpc_locomotion_amd.recurrent import ACTOR, CRITIC, RecurrentConfig
    cfg = PPOConfig()
    T, H = cfg.num_steps_per_env, args.hidden
    trainers = {"feed_forward": PPOTrainer(make_env(n, dev), cfg, seed=1)}
    if not args.baseline:
        trainers["recurrent"] = PPOTrainer(make_env(n, dev), cfg, seed=1, recurrent=RecurrentConfig(hidden_size=H))
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats, "update": "torch",
           "hidden_size": H, "baseline_only": bool(args.baseline), "mini_batches_per_update": cfg.num_learning_epochs * cfg.num_mini_batches,
           "device_state": {"before": device_state(0)}}
    for tr in trainers.values():          # warm-up: cold solves, code objects, torch's kernels, Adam's state
        tr.learn(2)
    torch.cuda.synchronize()
    # the launches on fixed inputs: 24 of each per block, one event pair around each
    obs = {k: tr.obs for k, tr in trainers.items()}
    launches = {"feed_forward_act": lambda t: trainers["feed_forward"].actor_critic.act(obs["feed_forward"], 1, t, out=trainers["feed_forward"].storage.slot(t))}
    if not args.baseline:
        rac, rst = trainers["recurrent"].actor_critic, trainers["recurrent"].storage
        launches["cell"] = lambda t: rac.cell_step({ACTOR: obs["recurrent"], CRITIC: obs["recurrent"]}, None, rst.hidden_slot(t))
        launches["recurrent_act"] = lambda t: rac.act(obs["recurrent"], 1, t, out=rst.slot(t), saved=rst.hidden_slot(t))
    spans = {k: [] for k in launches}
    names = list(launches)
    for rep in range(args.repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):
            e = [(ev(), ev()) for _ in range(T)]
            for t in range(T):
                e[t][0].record()
                launches[name](t)
                e[t][1].record()
            torch.cuda.synchronize()
            spans[name].extend(a.elapsed_time(b) for a, b in e)
    res["launches"] = {k: stats(v) for k, v in spans.items()}
    if not args.baseline:
        trainers["recurrent"].actor_critic.reset_memory()
        nets = lambda seq: sum(m.weight.numel() for m in seq if hasattr(m, "weight"))
        ff = trainers["feed_forward"].actor_critic
        mlp_bytes, cell_bytes = 4 * (nets(ff.actor) + nets(ff.critic)), 4 * 2 * 4 * H * (ff.num_obs + H)
        med = lambda k: res["launches"][k]["median_ms"]
        res["cell_share_of_0p82_ms_control_step"] = med("cell") / 0.82
        res["cell_over_feed_forward_act"] = med("cell") / med("feed_forward_act")
        res["weight_bytes"] = {"cell_both_memories": cell_bytes, "feed_forward_act_both_mlps": mlp_bytes, "ratio": cell_bytes / mlp_bytes}
        res["recurrent_act_over_feed_forward_act"] = med("recurrent_act") / med("feed_forward_act")
    # a whole iteration of each trainer
    times = {k: {"collect": [], "update": [], "full": []} for k in trainers}
    names = list(trainers)
    for rep in range(args.repeats):       # which one goes first alternates
        for name in (names if rep % 2 == 0 else names[::-1]):
            tr = trainers[name]
            a, b, c = ev(), ev(), ev()
            a.record()
            tr.collect()
            b.record()
            tr.alg.update(tr.storage)
            c.record()
            torch.cuda.synchronize()
            tb = times[name]
            tb["collect"].append(a.elapsed_time(b)); tb["update"].append(b.elapsed_time(c)); tb["full"].append(a.elapsed_time(c))
    for name, tb in times.items():
        res[name] = {k: stats(v) for k, v in tb.items()}
        res[name]["robot_ticks_per_s_training"] = n * T / (float(np.median(tb["full"])) * 1e-3)
    if not args.baseline:
        res["recurrent_over_feed_forward_median"] = {k: res["recurrent"][k]["median_ms"] / res["feed_forward"][k]["median_ms"] for k in ("collect", "update", "full")}
        res["collection_added_per_tick_ms"] = (res["recurrent"]["collect"]["median_ms"] - res["feed_forward"]["collect"]["median_ms"]) / T
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def through_time_report(args, dev, n):
    """The recurrent trainer with ``update_through_time="hip"`` against the one with the torch update: see the head of this file."""
    from bench import device_state
    from rl_mpc_locomotion_amd.recurrent import ACTOR, CRITIC, RecurrentConfig
    cfg = PPOConfig()
    T, H = cfg.num_steps_per_env, args.hidden
    trainers = {k: PPOTrainer(make_env(n, dev), cfg, seed=1, recurrent=RecurrentConfig(hidden_size=H, update_through_time=k)) for k in ("torch", "hip")}
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats, "hidden_size": H,
           "mini_batches_per_update": cfg.num_learning_epochs * cfg.num_mini_batches, "block_of_environments": n // cfg.num_mini_batches,
           "device_state": {"before": device_state(0)}}
    for tr in trainers.values():          # warm-up: cold solves, code objects, torch's kernels, Adam's state, the handle's workspace
        tr.learn(2)
    torch.cuda.synchronize()
    times = {k: {"collect": [], "update": [], "full": []} for k in trainers}
    names = list(trainers)
    for rep in range(args.repeats):       # which one goes first alternates
        for name in (names if rep % 2 == 0 else names[::-1]):
            tr = trainers[name]
            a, b, c = ev(), ev(), ev()
            a.record()
            tr.collect()
            b.record()
            tr.alg.update(tr.storage)
            c.record()
            torch.cuda.synchronize()
            tb = times[name]
            tb["collect"].append(a.elapsed_time(b)); tb["update"].append(b.elapsed_time(c)); tb["full"].append(a.elapsed_time(c))
    for name, tb in times.items():
        res[name] = {k: stats(v) for k, v in tb.items()}
        res[name]["robot_ticks_per_s_training"] = n * T / (float(np.median(tb["full"])) * 1e-3)
    res["hip_over_torch_median"] = {k: res["hip"][k]["median_ms"] / res["torch"][k]["median_ms"] for k in ("collect", "update", "full")}
    res["hip_p90_below_torch_p10"] = {k: bool(res["hip"][k]["p90_ms"] < res["torch"][k]["p10_ms"]) for k in ("update", "full")}
    # the device calls on their own, on the first mini-batch of the "hip" trainer's storage: both memories in every call
    tr = trainers["hip"]
    tr.collect()
    kernel = tr.actor_critic._seq
    b = next(tr.storage.recurrent_sequence_generator(cfg.num_mini_batches, 1))
    B = b.obs.shape[1]
    rows = (b.obs, b.obs if b.critic_obs is None else b.critic_obs)
    h0s, c0s = (b.hidden_a[0], b.hidden_c[0]), (b.hidden_a[1], b.hidden_c[1])
    dys = [torch.randn(T, B, H, device=dev) * 1e-3 for _ in range(2)]
    calls = {"forward": lambda: kernel.forward((ACTOR, CRITIC), rows, h0s, c0s, b.reset),
             "backward": lambda: kernel.backward((ACTOR, CRITIC), T, B, dys),
             "weight_gradients": lambda: kernel.backward((ACTOR, CRITIC), T, B, dys, entry="mpc_recurrent_bptt_weight_gradients")}
    spans = {k: [] for k in calls}
    for k in calls:                       # (forward first: the others go back through it)
        calls[k]()
    for rep in range(max(args.repeats, 3) * 3):
        for k in calls:
            a, c = ev(), ev()
            a.record()
            calls[k]()
            c.record()
            torch.cuda.synchronize()
            spans[k].append(a.elapsed_time(c))
    res["calls_on_one_mini_batch"] = {k: stats(v) for k, v in spans.items()}
    med = lambda k: res["calls_on_one_mini_batch"][k]["median_ms"]
    res["calls_on_one_mini_batch"]["through_time_launch_and_transposition_ms"] = med("backward") - med("weight_gradients")
    res["device_calls_per_update_ms"] = res["mini_batches_per_update"] * (med("forward") + med("backward"))
    res["workspace_bytes"] = kernel.workspace_bytes()
    res["workgroups_per_sequence_launch"] = 2 * ((B + 15) // 16)
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


def heads_report(args, dev, n):
    """The recurrent trainer with ``update_heads="hip"`` against the one with ``update_heads="torch"`` (both with the device roll): see the head of this file."""
    from _rate import wall_blocks
    from bench import device_state
    from rl_mpc_locomotion_amd.recurrent import RecurrentConfig
    cfg = PPOConfig()
    T, H = cfg.num_steps_per_env, args.hidden
    trainers = {k: PPOTrainer(make_env(n, dev), cfg, seed=1, recurrent=RecurrentConfig(hidden_size=H, update_through_time="hip", update_heads=k))
                for k in ("torch", "hip")}
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats, "hidden_size": H,
           "mini_batches_per_update": cfg.num_learning_epochs * cfg.num_mini_batches, "block_of_environments": n // cfg.num_mini_batches,
           "rows_per_mini_batch": T * (n // cfg.num_mini_batches), "device_state": {"before": device_state(0)}}
    events = {k: [] for k in trainers}
    warmup = 2                            # cold solves, code objects, torch's kernels, Adam's state, the handles' workspaces

    def iteration(name):
        tr = trainers[name]

        def run():
            a, b, c = ev(), ev(), ev()
            a.record()
            tr.collect()
            b.record()
            tr.alg.update(tr.storage)
            c.record()
            events[name].append((a, b, c))
        return run
    wall = wall_blocks({k: iteration(k) for k in trainers}, 1, args.repeats, n * T, warmup=warmup)
    for name, spans in events.items():
        spans = spans[warmup:]
        res[name] = {"collect": stats([a.elapsed_time(b) for a, b, _ in spans]), "update": stats([b.elapsed_time(c) for _, b, c in spans]),
                     "full": stats([a.elapsed_time(c) for a, _, c in spans])}
        res[name]["robot_ticks_per_s_training"] = n * T / (res[name]["full"]["median_ms"] * 1e-3)
        res[name]["host_clock_iteration"] = wall[name]
    res["hip_over_torch_median"] = {k: res["hip"][k]["median_ms"] / res["torch"][k]["median_ms"] for k in ("collect", "update", "full")}
    res["hip_p90_below_torch_p10"] = {k: bool(res["hip"][k]["p90_ms"] < res["torch"][k]["p10_ms"]) for k in ("update", "full")}
    res["update_per_mini_batch_ms"] = {k: res[k]["update"]["median_ms"] / res["mini_batches_per_update"] for k in trainers}
    hip = trainers["hip"]
    res["workspace_bytes"] = {"update_handle_and_dense_rows": hip.alg.workspace_bytes(), "memories_handle": hip.actor_critic._seq.workspace_bytes(),
                              "memories_handle_torch_heads": trainers["torch"].actor_critic._seq.workspace_bytes()}
    res["tensors_in_the_clip_and_adam"] = len(list(hip.actor_critic.parameters()))
    res["device_state"]["after"] = device_state(0, smi=False)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="3 collections and one update only (for a kernel trace)")
    ap.add_argument("--privileged", action="store_true", help="one iteration of the asymmetric actor-critic against the symmetric one (see the head of this file)")
    ap.add_argument("--heights", action="store_true", help="--privileged: on the terrain grid with the height scan (240 columns)")
    ap.add_argument("--baseline", action="store_true", help="--privileged / --recurrent: the symmetric / feed-forward trainer alone (runs on a tree without the option)")
    ap.add_argument("--recurrent", action="store_true", help="the recurrent actor-critic against the feed-forward one (see the head of this file)")
    ap.add_argument("--hidden", type=int, default=256, help="--recurrent: the memories' hidden size")
    ap.add_argument("--through-time", choices=("hip",), help="--recurrent: the update through time on the device against the torch update (see the head of this file)")
    ap.add_argument("--heads", choices=("hip",), help="--recurrent --through-time hip: the whole update on the device against torch's MLPs, loss and Adam")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.through_time and not args.recurrent:
        ap.error("--through-time goes with --recurrent")
    if args.heads and not args.through_time:
        ap.error("--heads goes with --recurrent --through-time hip")
    if not torch.cuda.is_available():
        sys.exit("ppo_rate.py measures on the GPU; none is visible")
    dev, n = "cuda:0", args.robots
    if args.privileged or args.recurrent:
        if args.recurrent:
            res = (heads_report if args.heads else through_time_report)(args, dev, n) if args.through_time else recurrent_report(args, dev, n)
        else:
            res = privileged_report(args, dev, n)
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        sys.exit(0)
    cfg = PPOConfig()
    T = cfg.num_steps_per_env
    env = make_env(n, dev)
    trainer = PPOTrainer(env, cfg, seed=1)
    ac, st = trainer.actor_critic, trainer.storage
    # the device update on the same actor-critic, with an optimiser of its own
    algs = {"torch": trainer.alg, "hip": PPO(ac, cfg, backend="hip")}
    if args.quick:
        for _ in range(3):
            trainer.collect()
        for alg in algs.values():
            st.step = st.T
            alg.update(st)
        torch.cuda.synchronize()
        sys.exit(0)
    from bench import device_state  # noqa: E402
    res = {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": n, "horizon": 10, "num_steps_per_env": T, "repeats": args.repeats,
           "nets": {"actor": [48, *cfg.actor_hidden_dims, 12], "critic": [48, *cfg.critic_hidden_dims, 1]}, "mini_batches_per_update": cfg.num_learning_epochs * cfg.num_mini_batches,
           "device_state": {"before": device_state(0)}}
    st_torch = RolloutStorage(n, T, dev)
    # warm-up: cold solves, code objects, torch's kernels and its GEMM choices, Adam's state
    trainer.learn(2)
    for _ in range(2):
        st.step = st.T
        algs["hip"].update(st)
    obs = trainer.obs
    _, rew, reset, extras = env.step(st.actions[0])
    time_outs = extras["time_outs"]
    for t in range(T):
        torch_act(ac, st_torch, t, obs); torch_add(st_torch, t, rew, reset, time_outs, cfg.gamma)
    torch_returns(ac, st_torch, obs, cfg.gamma, cfg.lam)
    torch.cuda.synchronize()

    t_act, t_add, t_ret, t_tact, t_tadd, t_tret, t_collect, t_steps, t_update, t_iter = ([] for _ in range(10))
    t_backend = {k: {"collect": [], "update": [], "full": []} for k in algs}
    for rep in range(args.repeats):
        # the pieces on fixed inputs (the environment's current buffers), fused and torch alternating
        for fused in (True, False):
            e = [[ev() for _ in range(3)] for _ in range(T)]
            s = st if fused else st_torch
            st.clear()
            for t in range(T):
                e[t][0].record()
                if fused:
                    ac.act(obs, trainer.seed, trainer.tick + t, out=s.slot(t))
                else:
                    torch_act(ac, s, t, obs)
                e[t][1].record()
                if fused:
                    s.add(rew, reset, time_outs, cfg.gamma, obs=obs)
                else:
                    torch_add(s, t, rew, reset, time_outs, cfg.gamma)
                e[t][2].record()
            r0, r1 = ev(), ev()
            r0.record()
            if fused:
                s.compute_returns(ac.evaluate(obs), cfg.gamma, cfg.lam)
            else:
                torch_returns(ac, s, obs, cfg.gamma, cfg.lam)
            r1.record()
            torch.cuda.synchronize()
            (t_act if fused else t_tact).extend(x[0].elapsed_time(x[1]) for x in e)
            (t_add if fused else t_tadd).extend(x[1].elapsed_time(x[2]) for x in e)
            (t_ret if fused else t_tret).append(r0.elapsed_time(r1))
        st.clear()
        # the whole iteration with each backend (which one goes first alternates), and T bare steps of the environment
        for name in (("torch", "hip") if rep % 2 == 0 else ("hip", "torch")):
            a, b, c = ev(), ev(), ev()
            a.record()
            trainer.collect()
            b.record()
            algs[name].update(st)
            c.record()
            torch.cuda.synchronize()
            tb = t_backend[name]
            tb["collect"].append(a.elapsed_time(b)); tb["update"].append(b.elapsed_time(c)); tb["full"].append(a.elapsed_time(c))
        t_collect.append(t_backend["torch"]["collect"][-1]); t_update.append(t_backend["torch"]["update"][-1]); t_iter.append(t_backend["torch"]["full"][-1])
        d, f = ev(), ev()
        d.record()
        for t in range(T):
            env.step(st.actions[t])
        f.record()
        torch.cuda.synchronize()
        trainer.obs = env.obs_buf
        t_steps.append(d.elapsed_time(f))
    res["fused"] = {"act": stats(t_act), "add_with_observation_copy": stats(t_add), "evaluate_and_compute_returns": stats(t_ret)}
    res["torch_composition"] = {"act": stats(t_tact), "add": stats(t_tadd), "evaluate_and_compute_returns": stats(t_tret)}
    res["iteration"] = {"collection_24_ticks": stats(t_collect), "bare_24_steps": stats(t_steps), "update": stats(t_update), "full": stats(t_iter)}
    m = lambda x: float(np.median(x))
    ut, uh = stats(t_backend["torch"]["update"]), stats(t_backend["hip"]["update"])
    res["update"] = {"torch": ut, "hip": uh, "hip_over_torch": uh["median_ms"] / ut["median_ms"], "hip_p90_below_torch_p10": uh["p90_ms"] < ut["p10_ms"],
                     "per_mini_batch_ms": {"torch": ut["median_ms"] / res["mini_batches_per_update"], "hip": uh["median_ms"] / res["mini_batches_per_update"]}}
    res["iteration_hip"] = {k: stats(v) for k, v in t_backend["hip"].items()}
    res["update_share_of_iteration_hip"] = m(t_backend["hip"]["update"]) / m(t_backend["hip"]["full"])
    res["robot_ticks_per_s_training_hip"] = n * T / (m(t_backend["hip"]["full"]) * 1e-3)
    tick_fused = np.array(t_act) + np.array(t_add)
    tick_torch = np.array(t_tact) + np.array(t_tadd)
    res["act_plus_add_per_tick"] = {"fused": stats(tick_fused), "torch": stats(tick_torch), "fused_over_torch": m(tick_fused) / m(tick_torch)}
    res["compute_returns_fused_over_torch"] = m(t_ret) / m(t_tret)
    res["collection_added_per_tick_ms"] = (m(t_collect) - m(t_steps)) / T
    res["collection_added_share_of_a_step_tick"] = (m(t_collect) - m(t_steps)) / m(t_steps)
    res["update_share_of_iteration"] = m(t_update) / m(t_iter)
    res["robot_ticks_per_s_training"] = n * T / (m(t_iter) * 1e-3)
    res["device_state"]["after"] = device_state(0, smi=False)
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
