"""The running observation normaliser on the MI355X (include/mpc_obs_norm.h, rl_mpc_locomotion_amd.obs_norm, PPOTrainer(normalize_obs=True)): the device
kernels tick by tick against the model of tests/obs_norm_ref.py (the rules of tests/test_obs_norm.py), reruns, in-place and storage-slot outputs behind
sentinels, a run that never waits for the device, the state dict, the trainer, fold_normalizer through WeightPolicy, and a learning run on badly scaled
observations."""
import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, obs_norm as O, ppo as P
from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
from tests import obs_norm_ref as ref
from tests.test_policy import ACT_ATOL, ACT_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -777.0


def _guarded(D, **kw):
    """An ObsNormalizer whose every buffer lies between two runs of sentinels."""
    norm = O.ObsNormalizer(D, device=DEV, guard=GUARD, **kw)
    for raw in norm._raw.values():
        raw.fill_(SENTINEL)
    norm.clear()
    return norm


def _guards_intact(norm):
    for name, raw in norm._raw.items():
        assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), name


def _state(norm):
    return [t.detach().cpu().numpy().copy() for t in (norm.state64[0], norm.state64[1], norm.count, norm._mean, norm._var, norm._std)]


def _same(a, b):
    return all(ref.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("D", ref.DS_GPU)
@pytest.mark.parametrize("n", ref.NS_GPU)
def test_device_matches_the_model_tick_by_tick(n, D):
    ticks, snaps = ref.reference(n, D, 100 * n + D)
    dev = [torch.tensor(x, device=DEV) for x in ticks]
    norm = _guarded(D)
    slots = torch.full((3, n, D), SENTINEL, device=DEV)                    # a rollout storage: the middle slot is written, its neighbours are not
    worst, outs, states = [0.0, 0.0], [], []
    for t, (x, xd, model) in enumerate(zip(ticks, dev, snaps)):
        what = f"n {n} D {D} tick {t}"
        before = _state(norm)
        y = norm(xd)
        st = _state(norm)
        r = ref.check_state(model, st[0], st[1], st[2], st[3], st[4], st[5], what)
        worst = [max(a, b) for a, b in zip(worst, r)]
        ref.check_output(x, y.cpu().numpy(), st[3], st[5], what, updated=model.count > 0)
        if t == ref.ALL_BAD_TICK:
            assert _same(before, st), what + ": a tick without a finite row changed the state"
        same = xd.clone()
        assert norm(same, out=same, update=False) is same and ref.same_bits(same.cpu().numpy(), y.cpu().numpy()), what + ": in place"
        rows = x.shape[0]
        slots[1].fill_(SENTINEL)
        norm(xd, out=slots[1, :rows], update=False)
        assert ref.same_bits(slots[1, :rows].cpu().numpy(), y.cpu().numpy()), what + ": storage slot"
        assert (slots[0] == SENTINEL).all() and (slots[2] == SENTINEL).all() and (slots[1, rows:] == SENTINEL).all(), what + ": wrote outside the slot"
        assert _same(st, _state(norm)), what + ": update=False changed the state"
        outs.append(y)
        states.append(st)
    _guards_intact(norm)
    print(f"n {n} D {D}: largest error / bound on the device, mean {worst[0]:.3f} var {worst[1]:.3f}")
    # again, from fresh, without ever waiting for the device: bit-identical
    again = _guarded(D)
    ys = [torch.empty_like(xd) for xd in dev]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for xd, y in zip(dev, ys):
            again(xd, out=y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same(states[-1], _state(again))
    for t, (a, b) in enumerate(zip(outs, ys)):
        assert ref.same_bits(a.cpu().numpy(), b.cpu().numpy()), f"n {n} D {D} tick {t}: a rerun differs"
    _guards_intact(again)


@pytest.mark.parametrize("n,D", [(65, 48), (1025, 80)])
def test_until_is_decided_on_the_device(n, D):
    until = 3 * n
    ticks, snaps = ref.reference(n, D, 9, until)
    norm = O.ObsNormalizer(D, until=until, device=DEV)
    torch.cuda.synchronize()
    dev = [torch.tensor(x, device=DEV) for x in ticks]
    states = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for xd in dev:
            norm(xd, out=xd)
            states.append([t.clone() for t in (norm.state64, norm.count, norm._mean, norm._var, norm._std)])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    frozen = [t for t in range(1, len(ticks)) if snaps[t - 1].count >= until]
    assert 3 <= frozen[0] <= 9
    for t, (model, st) in enumerate(zip(snaps, states)):
        assert int(st[1]) == model.count, t
        ref.check_state(model, st[0][0].cpu().numpy(), st[0][1].cpu().numpy(), int(st[1]), *(s.cpu().numpy() for s in st[2:]), f"until, tick {t}")
        if t in frozen:
            assert all(torch.equal(a, b) for a, b in zip(st, states[t - 1])), t


def test_wide_and_narrow_observations():
    """The widths at either end (one column; 256, the widest a staged block holds) and an odd one, against the model."""
    for D, n in ((1, 65), (33, 70), (256, 65)):
        ticks, snaps = ref.reference(n, D, 77)
        norm = _guarded(D)
        for t, (x, model) in enumerate(zip(ticks, snaps)):
            y = norm(torch.tensor(x, device=DEV))
            st = _state(norm)
            ref.check_state(model, *st, f"D {D} tick {t}")
            ref.check_output(x, y.cpu().numpy(), st[3], st[5], f"D {D} tick {t}", updated=model.count > 0)
        _guards_intact(norm)
    with pytest.raises(_lib.MpcLibraryError):
        O.ObsNormalizer(257, device=DEV)
    norm = O.ObsNormalizer(48, device=DEV)
    for bad in (torch.zeros((4, 47), device=DEV), torch.zeros((4, 48), device=DEV, dtype=torch.float64), torch.zeros((4, 96), device=DEV)[:, :48],
                torch.zeros((0, 48), device=DEV)):
        with pytest.raises(ValueError):
            norm(bad)
    with pytest.raises(ValueError):
        norm(torch.zeros((4, 48), device=DEV), out=torch.zeros((5, 48), device=DEV))


def test_the_workspace_grows_with_the_batch():
    """64 rows, then 5 x 64, then 64 and 5 x 64 again on one normaliser: the second call needs 10 blocks of partials where the first left room for 2, so the
    workspace is replaced by a larger one, which the later calls keep.  State and output against the model after every call."""
    D = 48
    small, large = ref.make_case(64, D, 6448), ref.make_case(5 * 64, D, 32048)
    model = ref.Model(D)
    norm = _guarded(D)
    for t, x in enumerate((small[0], large[1], small[2], large[3])):
        model.update(x)
        y = norm(torch.tensor(x, device=DEV))
        st = _state(norm)
        ref.check_state(model.snapshot(), *st, f"call {t}, {x.shape[0]} rows")
        ref.check_output(x, y.cpu().numpy(), st[3], st[5], f"call {t}, {x.shape[0]} rows", updated=model.count > 0)
    _guards_intact(norm)


def test_state_dict_round_trips():
    n, D = 65, 48
    ticks, _ = ref.reference(n, D, 100 * n + D)
    dev = [torch.tensor(x, device=DEV) for x in ticks]
    a = O.ObsNormalizer(D, device=DEV)
    for xd in dev[:6]:
        a(xd)
    sd = a.state_dict()
    assert sorted(sd) == ["_mean", "_std", "_var", "count", "state64"]
    assert sd["_mean"].shape == sd["_var"].shape == sd["_std"].shape == (1, D) and sd["_mean"].dtype == torch.float32
    assert sd["count"].dtype == torch.long and sd["state64"].dtype == torch.float64 and sd["state64"].shape == (2, D)
    b = O.ObsNormalizer(D, device=DEV)
    b.load_state_dict({k: v.cpu() for k, v in sd.items()})              # (as torch.load(map_location="cpu") gives it)
    assert _same(_state(a), _state(b))
    for xd in dev[6:9]:                                                    # the next three ticks: bit for bit the uninterrupted run
        assert torch.equal(a(xd).view(torch.int32), b(xd).view(torch.int32))
        assert _same(_state(a), _state(b))
    assert not torch.equal(sd["state64"], a.state64)                       # (the dict is a copy)
    # rsl_rl's own four keys: the float32 values, widened
    c = O.ObsNormalizer(D, device=DEV)
    c.load_state_dict({k: v for k, v in sd.items() if k != "state64"})
    for k in ("_mean", "_var", "_std", "count"):
        assert torch.equal(getattr(c, k), sd[k]), k
    assert torch.equal(c.state64[0], sd["_mean"][0].double()) and torch.equal(c.state64[1], sd["_var"][0].double())
    c(dev[6])                                                              # and it goes on from there
    assert int(c.count) == int(a.count) - int(np.isfinite(ticks[7]).all(1).sum()) - int(np.isfinite(ticks[8]).all(1).sum())
    with pytest.raises(ValueError):
        O.ObsNormalizer(32, device=DEV).load_state_dict(sd)
    a.clear()
    fresh = O.ObsNormalizer(D, device=DEV)
    assert _same(_state(a), _state(fresh)) and int(a.count) == 0 and (a._std == 1).all() and (a._mean == 0).all()


class _Standin:
    """tests/test_ppo_gpu.py's stand-in with observations offset_c + scale_c z: reward -mean((clamp(a, -1, 1) - c)^2), a time-out every 40 steps."""

    def __init__(self, n, seed, offset=None, scale=None):
        self.num_envs, self.num_obs, self.num_actions, self.device = n, 48, 12, torch.device(DEV)
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.c = torch.linspace(-0.6, 0.6, 12, device=DEV)
        self.offset = torch.zeros(48, device=DEV) if offset is None else offset.to(DEV)
        self.scale = torch.ones(48, device=DEV) if scale is None else scale.to(DEV)
        self.k = 0
        self.flags = (torch.zeros(n, dtype=torch.long, device=DEV), torch.ones(n, dtype=torch.long, device=DEV))

    def observe(self, n=None):
        return self.offset + self.scale * torch.randn((n or self.num_envs, 48), generator=self.gen, device=DEV)

    def reset(self):
        return self.observe()

    def step(self, actions):
        rew = -((actions.clamp(-1, 1) - self.c) ** 2).mean(-1)
        self.k += 1
        time_outs = self.flags[self.k % 40 == 0]
        return self.observe(), rew, time_outs, {"time_outs": time_outs}

    def rms(self, policy):
        return float(((policy(self.observe(1024)).clamp(-1, 1) - self.c) ** 2).mean().sqrt())


class _Recorder:
    """An environment that keeps a copy of every raw observation it hands out, in order."""

    def __init__(self, env):
        self.env, self.raw = env, []
        self.num_envs, self.num_obs, self.num_actions, self.device = env.num_envs, env.num_obs, env.num_actions, env.device

    def reset(self):
        obs = self.env.reset()
        self.raw.append(obs.clone())
        return obs

    def step(self, actions):
        out = self.env.step(actions)
        self.raw.append(out[0].clone())
        return out


N, T = 64, 4
CFG = dict(num_steps_per_env=T, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,), init_noise_std=0.5)


def _spread(seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(48, generator=g) * 4 - 2, torch.rand(48, generator=g) * 1.8 + 0.2


@pytest.mark.parametrize("update", ["torch", "hip"])
def test_trainer_normalises_every_observation_once(update):
    offset, scale = _spread()
    env = _Recorder(_Standin(N, seed=1, offset=offset, scale=scale))
    trainer = P.PPOTrainer(env, P.PPOConfig(**CFG), seed=3, update=update, normalize_obs=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                # the collection half still never waits for the device
    try:
        trainer.collect()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    trainer.alg.update(trainer.storage)
    trainer.learn(1)
    assert len(env.raw) == 1 + 2 * T and trainer.tick == 2 * T
    replay, model = O.ObsNormalizer(48, device=DEV), ref.Model(48)
    outs = []
    for raw in env.raw:                                                    # reset's observation, then every step's: update, then normalise
        outs.append(replay(raw))
        model.update(raw.cpu().numpy())
    assert int(trainer.obs_norm.count) == N * (1 + 2 * T) == model.count
    assert _same(_state(trainer.obs_norm), _state(replay))
    st = _state(replay)
    ref.check_state(model, *st, "trainer", const=())
    for t in range(T):                                                     # the storage of the second iteration: what the policy was given
        assert torch.equal(trainer.storage.observations[t], outs[T + t]), t
        ref.check_output(env.raw[T + t].cpu().numpy(), outs[T + t].cpu().numpy(), *[s.cpu().numpy() for s in _pub_after(env.raw, T + t)], f"slot {t}", const=())
    assert torch.equal(trainer.obs, outs[2 * T])
    assert abs(float(trainer.storage.observations.mean())) < 0.2 and abs(float(trainer.storage.observations.std()) - 1) < 0.2
    before = _state(trainer.obs_norm)
    result = trainer.evaluate(5)                                           # evaluation normalises with the statistics as they are
    assert _same(before, _state(trainer.obs_norm)) and len(env.raw) == 1 + 2 * T + 5 and result["episodes"] >= 0
    assert torch.equal(trainer.obs, replay(env.raw[-1], update=False))
    policy = trainer.get_inference_policy()
    assert torch.equal(policy(env.raw[3]), trainer.actor_critic.act_inference(replay(env.raw[3], update=False))) and _same(before, _state(trainer.obs_norm))


def _pub_after(raws, k):
    """(_mean, _std) of a fresh normaliser after raws[0 .. k]."""
    norm = O.ObsNormalizer(48, device=DEV)
    for raw in raws[:k + 1]:
        norm(raw)
    return norm._mean, norm._std


def test_normalisation_off_is_the_trainer_as_it_was(tmp_path):
    runs = []
    for kw in ({}, dict(normalize_obs=False)):
        trainer = P.PPOTrainer(_Standin(N, seed=1), P.PPOConfig(**CFG), seed=3, **kw)
        infos = trainer.learn(2)
        path = str(tmp_path / f"model{len(runs)}.pt")
        trainer.save(path)
        runs.append((infos, [p.detach().clone() for p in trainer.actor_critic.parameters()], torch.load(path), trainer))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert sorted(runs[0][2]) == sorted(runs[1][2]) == ["infos", "iter", "model_state_dict", "optimizer_state_dict"]
    assert runs[1][3].obs_norm is None


def test_checkpoint_carries_the_normaliser(tmp_path):
    offset, scale = _spread()
    trainer = P.PPOTrainer(_Standin(N, seed=1, offset=offset, scale=scale), P.PPOConfig(**CFG), seed=3, normalize_obs=True, obs_norm_eps=2e-2)
    trainer.learn(2)
    path, plain_path = str(tmp_path / "model.pt"), str(tmp_path / "plain.pt")
    trainer.save(path)
    ck = torch.load(path)
    assert sorted(ck) == ["infos", "iter", "model_state_dict", "obs_norm_state_dict", "optimizer_state_dict"]
    assert sorted(ck["obs_norm_state_dict"]) == ["_mean", "_std", "_var", "count", "state64"]
    fresh = P.PPOTrainer(_Standin(N, seed=2, offset=offset, scale=scale), P.PPOConfig(**CFG), seed=4, normalize_obs=True, obs_norm_eps=2e-2)
    raw = offset.to(DEV) + scale.to(DEV) * torch.randn((50, 48), generator=torch.Generator(device=DEV).manual_seed(8), device=DEV)
    want = trainer.get_inference_policy()(raw)
    assert not torch.equal(fresh.get_inference_policy()(raw), want)
    fresh.load(path)
    assert _same(_state(fresh.obs_norm), _state(trainer.obs_norm)) and torch.equal(fresh.get_inference_policy()(raw), want)
    fresh.learn(1)
    assert fresh.iteration == 3 and int(fresh.obs_norm.count) == N * (1 + 2 * T) + N * (1 + T)       # (a load starts from a reset, whose observation counts)
    plain = P.PPOTrainer(_Standin(N, seed=2), P.PPOConfig(**CFG), seed=4)
    params = [p.detach().clone() for p in plain.actor_critic.parameters()]
    with pytest.raises(ValueError):
        plain.load(path)
    assert all(torch.equal(a, b) for a, b in zip(params, plain.actor_critic.parameters()))          # refused before anything was loaded
    plain.learn(1)
    plain.save(plain_path)
    with pytest.raises(ValueError):
        fresh.load(plain_path)


def test_the_device_update_still_reads_the_host_once_per_iteration(monkeypatch):
    offset, scale = _spread()
    trainer = P.PPOTrainer(_Standin(N, seed=1, offset=offset, scale=scale), P.PPOConfig(**CFG), seed=3, update="hip", normalize_obs=True)
    trainer.learn(1)                                                       # (the first iteration allocates)
    calls = dict(tolist=0, item=0, cpu=0)
    for name in calls:
        plain = getattr(torch.Tensor, name)

        def counted(self, *a, _name=name, _plain=plain, **kw):
            if self.is_cuda:
                calls[_name] += 1
            return _plain(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    trainer.learn(1)
    assert calls == dict(tolist=1, item=0, cpu=0), calls


def test_fold_normalizer_runs_through_weight_policy():
    """Statistics learnt from observations inside the task's +-5 clip (offsets up to 2, scales 0.2 .. 2): the folded state dict through WeightPolicy on raw
    observations against the float64 folded net."""
    offset, scale = _spread(seed=6)
    g = torch.Generator().manual_seed(7)
    norm = O.ObsNormalizer(48, device=DEV)
    for _ in range(6):
        norm((offset + scale * torch.randn((512, 48), generator=g)).clamp(-5, 5).to(DEV))
    raw = (offset + scale * torch.randn((300, 48), generator=g)).clamp(-5, 5)
    torch.manual_seed(5)
    ac = P.ActorCritic(48, 12, (64, 32), (64, 32))
    sd, nsd = ac.state_dict(), {k: v.cpu() for k, v in norm.state_dict().items()}
    folded = O.fold_normalizer(sd, nsd)
    assert all(v.dtype == torch.float32 for v in folded.values()) and torch.equal(folded["actor.2.weight"], sd["actor.2.weight"])
    folded64 = O.fold_normalizer({k: v.double() for k, v in sd.items()}, nsd)
    net = P.mlp(48, (64, 32), 12).double()
    net.load_state_dict({k[6:]: v for k, v in folded64.items() if k.startswith("actor.")})
    with torch.no_grad():
        want = net(raw.double())
        normalised = ac.double().actor((raw.double() - nsd["_mean"].double()) / (nsd["_std"] + torch.tensor(1e-2)).double())
    assert (want - normalised).abs().max() <= 1e-9 * normalised.abs().max()
    got = WeightPolicy.from_state_dict(folded, device=DEV).step(raw.to(DEV), return_actions=True)[1]
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=ACT_RTOL, atol=ACT_ATOL)
    # and the route for a caller who needs better: the normaliser in front of the unfolded policy
    got2 = WeightPolicy.from_state_dict(sd, device=DEV).step(norm(raw.to(DEV), update=False), return_actions=True)[1]
    np.testing.assert_allclose(got2.cpu().numpy(), want.numpy(), rtol=ACT_RTOL, atol=ACT_ATOL)


def _badly_scaled():
    offset = torch.tensor([-20.0, 0.0, 20.0])[torch.arange(48) % 3]
    scale = torch.tensor([0.01, 1.0, 50.0])[(torch.arange(48) // 3) % 3]
    return offset, scale


@pytest.mark.parametrize("update", ["torch", "hip"])
def test_learning_on_badly_scaled_observations(update):
    """tests/test_ppo_gpu.py's test_learning_sanity (256 environments, 30 iterations, nets (64, 32), noise 0.5; its recorded ratio is 0.41) with observations
    offset_c + scale_c z, offsets from {-20, 0, 20} and scales from {0.01, 1, 50}: after normalisation the problem is that test's in distribution, so the
    condition is that test's, RMS distance after <= 0.6 x before.  The ratio without normalisation is printed for the record and not asserted.  (Recorded: 0.32 with
    normalisation for either backend; 0.97 / 0.99 without.)"""
    offset, scale = _badly_scaled()
    cfg = P.PPOConfig(num_steps_per_env=24, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    ratios = {}
    for on in (True, False):
        env = _Standin(256, seed=0, offset=offset, scale=scale)
        trainer = P.PPOTrainer(env, cfg, seed=0, update=update, normalize_obs=on)
        policy = trainer.get_inference_policy()
        if on:
            trainer.obs = trainer._first_obs()                              # (statistics before the first measurement: one batch)
        before = env.rms(policy)
        infos = trainer.learn(30)
        after = env.rms(policy)
        ratios[on] = after / before
        print(f"update {update}, normalize_obs {on}: rms of clamp(mean) - c: {before:.3f} -> {after:.3f} (ratio {after / before:.2f})")
        if on:
            assert len(infos) == 30 and all(np.isfinite(list(i.values())).all() for i in infos)
    assert ratios[True] <= 0.6
