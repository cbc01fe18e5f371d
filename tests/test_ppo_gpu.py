"""PPO's collection half on the MI355X (include/mpc_ppo.h, rl_mpc_locomotion_amd.ppo): the act kernel against torch's nn.Sequential and against
WeightPolicy, the parameters read in place, add + compute_returns against tests/ppo_ref.py (the rules of tests/test_ppo.py), the sampler, a
collection with BatchedRLTask that never waits for the device, a learning sanity run and the checkpoint round trip."""
import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import ppo as P, rl_task as R
from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
from tests import ppo_ref
from tests.test_policy import ACT_ATOL, ACT_RTOL
from tests.test_ppo import GAMMA, LAM, check_log_prob, check_returns, check_sampler_moments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
NETS = {"reference": ((512, 256, 128), (512, 256, 128)), "uneven": ((32, 16), (64,))}


def _pair(nets, seed):
    """The same random actor-critic on the CPU (torch's reference) and on the device, std in [0.05, 2]."""
    torch.manual_seed(seed)
    cpu = P.ActorCritic(48, 12, *NETS[nets])
    with torch.no_grad():
        cpu.std.copy_(torch.rand(12) * 1.95 + 0.05)
        for p in cpu.parameters():
            if p.dim() == 1 and p is not cpu.std:
                p.copy_(torch.randn_like(p) * 0.1)                               # (torch's default biases are small)
    dev = P.ActorCritic(48, 12, *NETS[nets])
    dev.load_state_dict(cpu.state_dict())
    return cpu, dev.to(DEV)


def _obs(n, seed):
    return (torch.randn((n, 48), generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


def _check_act(cpu, out, obs, what, rows):
    """One act's outputs against torch on the CPU with the kernel's own noise: mean, values, sigma, and actions == mean + std * eps bit for bit.
    The rows go to `rows` for _check_log_prob."""
    host = {k: v.cpu() for k, v in out.items()}
    _, _, values, mean, sigma = ppo_ref.act(cpu.actor, cpu.critic, cpu.std.detach(), obs.cpu(), host["eps"])
    np.testing.assert_allclose(host["mu"].numpy(), mean.numpy(), rtol=ACT_RTOL, atol=ACT_ATOL, err_msg=what)
    np.testing.assert_allclose(host["values"].numpy(), values.numpy(), rtol=ACT_RTOL, atol=ACT_ATOL, err_msg=what)
    assert torch.equal(host["sigma"], sigma), what
    assert torch.equal(host["actions"], host["mu"] + sigma * host["eps"]), f"{what}: actions differ from mean + std * eps in float32"
    rows.append(host)


def _check_log_prob(cpu, rows, what):
    """The rule of the CPU test (4 x torch's own float32-vs-float64 gap on the same rows) over all the rows of a test together, at least the CPU
    test's 64: the gap of a single row is one draw of a rounding error and may be nothing at all, which would turn the rule into bit-identity with
    torch's log and reduction order."""
    cat = lambda k: torch.cat([r[k] for r in rows]).numpy()
    assert len(cat("mu")) >= 64
    check_log_prob(cat("actions"), cat("actions_log_prob")[:, 0], cat("mu"), cpu.std.detach().numpy(), cat("eps"), what)


@pytest.mark.parametrize("nets", sorted(NETS))
def test_act_matches_torch(nets):
    cpu, dev = _pair(nets, seed=1)
    rows = []
    for n in (1, 15, 16, 17, 80):
        obs = _obs(n, seed=n)
        out = dev.act(obs, seed=3, step=n, return_eps=True)
        assert out["actions"].shape == (n, 12) and out["values"].shape == (n, 1) and out["actions_log_prob"].shape == (n, 1)
        _check_act(cpu, out, obs, f"{nets} n = {n}", rows)
        assert torch.equal(dev.evaluate(obs), out["values"]) and torch.equal(dev.act_inference(obs), out["mu"])
    _check_log_prob(cpu, rows, f"{nets}, n = 1, 15, 16, 17, 80 together")


@pytest.mark.parametrize("n", (17, 80))
def test_mean_is_bit_identical_to_weight_policy(n):
    cpu, dev = _pair("reference", seed=2)
    obs = _obs(n, seed=20 + n)
    raw = WeightPolicy.from_state_dict(cpu.state_dict(), device=DEV).step(obs, return_actions=True)[1]
    out = dev.act(obs, seed=1, step=0)
    assert torch.equal(out["mu"], raw) and torch.equal(dev.act_inference(obs), raw)


def test_parameters_are_read_in_place():
    cpu, dev = _pair("uneven", seed=3)
    obs = _obs(81, seed=5)
    before = dev.act(obs, seed=1, step=0, return_eps=True)
    ptrs = dev._bound_ptrs
    opt = torch.optim.SGD(dev.parameters(), lr=0.05)
    g = torch.Generator().manual_seed(9)
    for p in dev.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV) * (0.2 if p is dev.std else 1.0)
    opt.step()                                                                   # in place: same addresses, new values
    after = dev.act(obs, seed=1, step=0, return_eps=True)
    assert dev._bound_ptrs == ptrs                                               # no re-bind
    cpu.load_state_dict({k: v.cpu() for k, v in dev.state_dict().items()})
    rows = []
    _check_act(cpu, after, obs, "after an optimiser step", rows)
    _check_log_prob(cpu, rows, "after an optimiser step")
    assert torch.equal(after["eps"], before["eps"])
    assert (after["mu"] - before["mu"]).abs().max() > 100 * ACT_ATOL and (after["values"] - before["values"]).abs().max() > 100 * ACT_ATOL
    assert not torch.equal(after["sigma"], before["sigma"])


def _add_and_compute_returns(n, T):
    """T adds and compute_returns on a storage of n environments against the torch loop (check_returns), and a rerun.  Returns what the device read and
    wrote as [T, n] numpy arrays: (returns - values, normalised advantages)."""
    rew, reset, time_outs, values, last = ppo_ref.rollout(T, n, seed=30 + n)
    st = P.RolloutStorage(n, T, DEV)
    st.values.copy_(values)
    st.rewards.fill_(-7.0); st.dones.fill_(-7.0)
    d_rew, d_reset, d_to = rew.to(DEV), reset.to(DEV), time_outs.to(DEV)
    for t in range(T):
        st.add(d_rew[t], d_reset[t], d_to[t], GAMMA)
        if t == 2:                                                               # slots 0 .. 2 written, 3 and 4 untouched
            assert (st.rewards[3:] == -7.0).all() and (st.dones[3:] == -7.0).all() and (st.rewards[:3] != -7.0).all() and (st.dones[:3] >= 0).all()
    assert st.step == T and torch.equal(st.dones[..., 0].cpu(), reset.float()) and torch.equal(st.values.cpu(), values)
    with pytest.raises(RuntimeError):
        st.add(d_rew[0], d_reset[0], d_to[0], GAMMA)
    st.compute_returns(last.to(DEV), GAMMA, LAM)
    h = lambda x: x[..., 0].cpu().numpy()
    raw = h(st.returns) - h(st.values)
    check_returns(h(st.rewards), h(st.returns), raw, h(st.advantages), rew, reset, time_outs, values, last, f"device n = {n}, T = {T}")
    first = st.advantages.clone()
    st.compute_returns(last.to(DEV), GAMMA, LAM)                                 # fixed-order float64 sums: a rerun is bit-identical
    assert torch.equal(first, st.advantages)
    return raw, h(first)


@pytest.mark.parametrize("n", (1, 63, 65))
def test_add_and_compute_returns_match_the_torch_loop(n):
    _add_and_compute_returns(n, 5)


# normalise_kernel is one workgroup of 1024 lanes, each walking i += 1024: m = n T around one trip (1023, 1024, 1025), two trips and one element
# (2049), and PPOConfig's own 4096 x 24 = 98 304 (96 trips, every lane of the tree loaded)
@pytest.mark.parametrize("n, T", ((341, 3), (1024, 1), (205, 5), (683, 3), (4096, 24)))
def test_compute_returns_normalises_beyond_one_trip(n, T):
    """On top of check_returns: the kernel's moments are float64 and differ from the sequential ones in summation order only, so the float32 rounding
    of (a - mean) / (std + 1e-8) may flip against that of ppo_ref.normalise in float64 but cannot move further: one float32 ulp, everywhere."""
    from tests.helpers import ulp32
    assert n * T in (1023, 1024, 1025, 2049, 98304)
    raw, adv = _add_and_compute_returns(n, T)
    want = ppo_ref.normalise(torch.from_numpy(raw).double()).float().numpy()
    assert np.isfinite(adv).all() and adv.shape == want.shape == (T, n)
    off = np.abs(adv.astype(np.float64) - want.astype(np.float64)) / ulp32(want)
    print(f"device n = {n}, T = {T}: normalised advantages within {off.max():.2f} ulp of the rounded float64 evaluation, {int((off > 0).sum())} of {off.size} differ")
    assert (off <= 1.0).all(), f"n = {n}, T = {T}: {int((off > 1.0).sum())} normalised advantages more than one ulp off, worst {off.max():.2f}"


def test_sampler_on_the_device():
    """The moment bounds of the CPU test on the device's own draws; reruns; and environment 5's three-step rollout inside a batch of 80 against the
    smallest batch that holds it (6), whose other environments see other observations: a draw depends on (seed, environment, step) alone."""
    _, dev = _pair("uneven", seed=4)
    obs = _obs(4096, seed=1)
    draws = [dev.act(obs, seed=1, step=s, return_eps=True) for s in range(16)]
    eps = torch.stack([d["eps"] for d in draws], dim=1)                         # [4096, 16, 12]
    check_sampler_moments(eps.cpu().numpy())
    again = dev.act(obs, seed=1, step=7, return_eps=True)
    for k in ("eps", "actions", "actions_log_prob", "values", "mu"):
        assert torch.equal(again[k], draws[7][k]), k
    assert not torch.equal(dev.act(obs, seed=2, step=7, return_eps=True)["eps"], again["eps"])
    small = obs[:6].clone()
    small[:5] = _obs(5, seed=2)
    for s in range(3):
        a, b = dev.act(obs[:80].contiguous(), seed=1, step=s, return_eps=True), dev.act(small, seed=1, step=s, return_eps=True)
        for k in ("eps", "actions", "actions_log_prob", "values", "mu"):
            assert torch.equal(a[k][5], b[k][5]) and torch.equal(a[k][5], draws[s][k][5]), (s, k)
        assert not torch.equal(a["mu"][4], b["mu"][4]) and not torch.equal(a["values"][4], b["values"][4])       # (the neighbours did differ)


class _Recorder:
    """An environment that keeps what BatchedRLTask.step returned on each tick (device copies: its buffers are rewritten by the next step)."""

    def __init__(self, env, ticks):
        self.env, self.k = env, 0
        self.num_envs, self.num_obs, self.num_actions, self.device = env.num_envs, env.num_obs, env.num_actions, env.device
        self.rew = torch.zeros((ticks, env.num_envs), dtype=torch.float32, device=env.device)
        self.reset_rec = torch.zeros((ticks, env.num_envs), dtype=torch.long, device=env.device)
        self.time_outs = torch.zeros((ticks, env.num_envs), dtype=torch.long, device=env.device)

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        out = self.env.step(actions)
        self.rew[self.k].copy_(out[1]); self.reset_rec[self.k].copy_(out[2]); self.time_outs[self.k].copy_(out[3]["time_outs"])
        self.k += 1
        return out


def test_collection_with_the_batched_task_never_waits_for_the_device():
    n, T = 64, 4
    task = R.BatchedRLTask([i % 3 for i in range(n)], [TROT] * n, cfg=R.TaskConfig(episode_length_s=0.03, seed=5), device=DEV)      # 3-tick episodes
    env = _Recorder(task, T)
    cfg = P.PPOConfig(num_steps_per_env=T, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,), init_noise_std=0.5)
    trainer = P.PPOTrainer(env, cfg, seed=11)
    trainer.obs = env.reset()
    eps = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # a torch call that waits for the device or copies to the host raises from here on
    try:
        trainer.collect(record_eps=eps)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = trainer.storage
    assert trainer.tick == T and st.step == T and env.k == T
    rew, reset, time_outs = env.rew.cpu(), env.reset_rec.cpu(), env.time_outs.cpu()
    assert reset.any() and time_outs.any() and not reset.all()
    cpu = P.ActorCritic(48, 12, cfg.actor_hidden_dims, cfg.critic_hidden_dims)
    cpu.load_state_dict({k: v.cpu() for k, v in trainer.actor_critic.state_dict().items()})
    rows = []
    for t in range(T):
        out = dict(st.slot(t), eps=eps[t])
        _check_act(cpu, out, st.observations[t], f"tick {t}", rows)
        if t:
            assert not torch.equal(st.observations[t], st.observations[t - 1])
    _check_log_prob(cpu, rows, "collection, all ticks")
    assert torch.equal(st.observations[T - 1], st.observations[T - 1].clamp(-5, 5)) and torch.equal(trainer.obs, task.obs_buf)
    np.testing.assert_allclose(trainer.last_values.cpu().numpy(), cpu.critic(trainer.obs.cpu()).detach().numpy(), rtol=ACT_RTOL, atol=ACT_ATOL)
    h = lambda x: x[..., 0].cpu().numpy()
    check_returns(h(st.rewards), h(st.returns), h(st.returns) - h(st.values), h(st.advantages), rew, reset, time_outs, st.values.cpu(),
                  trainer.last_values.cpu(), "collection")


class _Standin:
    """Fresh standard normal observations; reward -mean((clamp(a, -1, 1) - c)^2) with c = linspace(-0.6, 0.6, 12); a time-out every 40 steps."""

    def __init__(self, n, seed):
        self.num_envs, self.num_obs, self.num_actions, self.device = n, 48, 12, torch.device(DEV)
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.c = torch.linspace(-0.6, 0.6, 12, device=DEV)
        self.k = 0
        self.flags = (torch.zeros(n, dtype=torch.long, device=DEV), torch.ones(n, dtype=torch.long, device=DEV))

    def observe(self, n=None):
        return torch.randn((n or self.num_envs, 48), generator=self.gen, device=DEV)

    def reset(self):
        return self.observe()

    def step(self, actions):
        rew = -((actions.clamp(-1, 1) - self.c) ** 2).mean(-1)
        self.k += 1
        time_outs = self.flags[self.k % 40 == 0]
        return self.observe(), rew, time_outs, {"time_outs": time_outs}

    def rms(self, policy):
        return float(((policy(self.observe(1024)).clamp(-1, 1) - self.c) ** 2).mean().sqrt())


def test_learning_sanity():
    env = _Standin(256, seed=0)
    cfg = P.PPOConfig(num_steps_per_env=24, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    trainer = P.PPOTrainer(env, cfg, seed=0)
    policy = trainer.get_inference_policy()
    before = env.rms(policy)
    infos = trainer.learn(30)
    after = env.rms(policy)
    print(f"rms of clamp(mean) - c: {before:.3f} -> {after:.3f} (ratio {after / before:.2f}); mean reward {infos[0]['mean_reward']:.3f} -> {infos[-1]['mean_reward']:.3f}")
    assert len(infos) == 30 and infos[-1]["iter"] == 30 and all(np.isfinite(list(i.values())).all() for i in infos)
    assert after <= 0.6 * before


def test_checkpoint_round_trip(tmp_path):
    cfg = P.PPOConfig(num_steps_per_env=4, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,))
    trainer = P.PPOTrainer(_Standin(32, seed=1), cfg, seed=3)
    trainer.learn(2)
    path = str(tmp_path / "model.pt")
    trainer.save(path)
    ck = torch.load(path)
    assert sorted(ck) == ["infos", "iter", "model_state_dict", "optimizer_state_dict"] and ck["iter"] == 2 and len(ck["infos"]) == 2
    fresh = P.PPOTrainer(_Standin(32, seed=2), cfg, seed=4)
    obs = _obs(50, seed=8)
    want = trainer.get_inference_policy()(obs)
    assert not torch.equal(fresh.get_inference_policy()(obs), want)
    fresh.load(path)
    assert fresh.iteration == 2 and torch.equal(fresh.get_inference_policy()(obs), want)
    assert fresh.alg.optimizer.state_dict()["state"].keys() == trainer.alg.optimizer.state_dict()["state"].keys()
    raw = WeightPolicy.from_state_dict(torch.load(path)["model_state_dict"], device=DEV).step(obs, return_actions=True)[1]
    assert torch.equal(raw, want)
    fresh.learn(1)                                                               # and training goes on from it
    assert fresh.iteration == 3


# every option at once: the riders of learn's one read in their full order, every checkpoint part, both kinds of actor-critic
RECORD_KEYS = ["iter", "mean_reward", "done_rate", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate", "mean_episode_return", "mean_episode_length",
               "episodes_in_window", "episodes_finished", "timeouts_in_window", "mean_terrain_level", "terrain_level_by_type", "episode_terms"]
CHECKPOINT_KEYS = ["critic_obs_norm_state_dict", "episode_terms_state_dict", "infos", "iter", "model_state_dict", "obs_norm_state_dict", "optimizer_state_dict",
                   "plant_rand_state_dict"]


def _all_options_task(n=64):
    """64 environments of the three robot types on test_curriculum_gpu's 3 x 2 grid with episodes of 3 ticks, so that resets, episode closes, terrain
    and command curriculum moves, pushes and plant draws all happen inside a collection of 4 ticks."""
    from rl_mpc_locomotion_amd import curriculum as K, domain_rand as DR, episode_terms as E, height_scan as HS, plant_rand as PR, privileged_obs as V
    from tests.test_curriculum_gpu import grid
    cfg = R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), episode_length_s=0.03, seed=4)
    scan = HS.HeightScan(n, device=DEV)
    return R.BatchedRLTask(
        [i % 3 for i in range(n)], [TROT] * n, cfg=cfg, horizon=10, device=DEV, yaw0=np.random.default_rng(6).uniform(-np.pi, np.pi, n), height_scan=scan,
        curriculum=K.TerrainCurriculum(grid(), n, max_init_level=1, seed=2, device=DEV, env_length=0.0002, episode_length_s=cfg.episode_length_s),
        episode_terms=E.EpisodeTerms(n, cfg, command_curriculum=E.CommandCurriculumSpec(1.5, x_range0=(-0.5, 0.5), step=0.5, threshold=0.0, update_every=1),
                                     device=DEV),
        domain_rand=DR.DomainRand(n, observations=DR.NoiseSpec.legged_gym(cfg, height_scan=scan), actions=DR.NoiseSpec("gaussian", "additive", (0.0, 0.05)),
                                  push=DR.PushSpec(interval_s=0.02, max_vel_xy=0.5), seed=9, device=DEV),
        plant_rand=PR.PlantRand(n, PR.PlantSpec(payload=(-1.0, 3.0), strength=(0.9, 1.1), gravity=(-1.0, 1.0), resample="reset"), seed=21, device=DEV),
        privileged_obs=V.PrivilegedObs(n, device=DEV, plant=True))


@pytest.mark.parametrize("kind", ["feed_forward_hip_update", "recurrent_through_time_on_the_device"])
def test_all_options_at_once(kind, tmp_path):
    from rl_mpc_locomotion_amd.episode_terms import EpisodeTerms
    from rl_mpc_locomotion_amd.recurrent import RecurrentConfig
    recurrent = kind.startswith("recurrent")
    cfg = P.PPOConfig(num_steps_per_env=4, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,))
    how = dict(update="torch", recurrent=RecurrentConfig(hidden_size=32, update_through_time="hip")) if recurrent else dict(update="hip")
    task = _all_options_task()
    cur, et = task.curriculum, task.episode_terms
    trainer = P.PPOTrainer(task, cfg, seed=3, normalize_obs=True, **how)
    held, asked, summary, zero = [], [], et.summary, et.new_window

    def new_window():                                                            # what the window held when the trainer read it
        held.append(summary().tolist())
        zero()
    et.summary = lambda: (asked.append(1), summary())[1]
    et.new_window = new_window
    infos = trainer.learn(2)
    assert len(infos) == 2 and all(list(i) == RECORD_KEYS for i in infos) and [i["iter"] for i in infos] == [1, 2]
    if not recurrent:
        assert infos[-1]["learning_rate"] == trainer.alg.lr_device.item() == trainer.alg.learning_rate
    levels = cur.record(cur.summary().tolist(), cur.num_types)
    assert {k: infos[-1][k] for k in levels} == levels and len(levels["terrain_level_by_type"]) == cur.num_types == 2
    assert len(asked) == len(held) == 2 and [i["episode_terms"] for i in infos] == [EpisodeTerms.record(h) for h in held]      # one summary read per iteration
    # the options did their work inside the collections (the first tick's resets close empty episodes, which are not counted: the second window has the closes)
    assert held[0][0] == 0 and held[1][0] >= 64 and infos[1]["episode_terms"]["command_widenings"] >= 1 and task.plant_rand.get_counters().min() >= 2
    assert infos[1]["mean_terrain_level"] != infos[0]["mean_terrain_level"]
    path = str(tmp_path / "all.pt")
    trainer.save(path)
    assert sorted(torch.load(path)) == CHECKPOINT_KEYS
    fresh = P.PPOTrainer(_all_options_task(), cfg, seed=4, normalize_obs=True, **how)
    obs = torch.randn((64, task.num_obs), generator=torch.Generator().manual_seed(8)).to(DEV)
    start = dict(reset=torch.ones(64, dtype=torch.long, device=DEV)) if recurrent else {}      # (the actor's memory starts from zero state on either side)
    want = trainer.get_inference_policy()(obs, **start)
    assert not torch.equal(fresh.get_inference_policy()(obs, **start), want)
    fresh.load(path)
    assert fresh.iteration == 2 and fresh._prev_reset is None and fresh.obs is None
    assert torch.equal(fresh.get_inference_policy()(obs, **start), want)
    assert len(fresh.learn(1)) == 3 and fresh.iteration == 3 and list(fresh.infos[-1]) == RECORD_KEYS
