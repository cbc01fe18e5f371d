"""The episode statistics on the MI355X (include/mpc_episode.h, rl_mpc_locomotion_amd.episode) against the model of tests/episode_ref.py, whose text gives
the bounds: after every tick the accumulators, the window in deque order, the counts and the integer totals are ``==`` the model's, the float64 sums
and means within k 2^-52 sum|x|.  Shapes: the smallest at which ranks, offsets and the ring can go wrong (one wave, one workgroup of 256 lanes, two and more
of them; windows of 1, 3 and 100 entries against ticks that finish none, one, exactly cap, cap + 1 and everyone).  Then the trainer:
``infos``, ``evaluate``, ``init_at_random_ep_len``, and the one host read of an iteration."""
import math

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import episode as E, ppo as P, rl_task as R
from tests import episode_ref as ref
from tests.test_episode import build_shim, host_progress

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
GUARD = 8
BUFFERS = ("cur_return", "cur_length", "win_return", "win_length", "win_timed_out", "counters", "sums", "summary")
SENTINEL = {torch.float32: -7.25, torch.int32: -77, torch.long: -7777, torch.float64: -7.125}


def _stats(n, cap, G, groups):
    s = E.EpisodeStats(n, window=cap, groups=groups, num_groups=G, device=DEV, guard=GUARD)
    for t in s._raw.values():
        t[:GUARD] = SENTINEL[t.dtype]; t[-GUARD:] = SENTINEL[t.dtype]
    return s


def _guards_intact(s):
    return all(bool((t[:GUARD] == SENTINEL[t.dtype]).all()) and bool((t[-GUARD:] == SENTINEL[t.dtype]).all()) for t in s._raw.values())


def _state(s):
    """The device buffers as numpy (three copies: the 32-bit buffers by their bit patterns, the counters, the sums)."""
    words = torch.cat((s.cur_return.view(torch.int32), s.cur_length, s.win_return.view(torch.int32), s.win_length, s.win_timed_out)).cpu().numpy()
    n, cap = s.n, s.window
    cut = np.split(words, [n, 2 * n, 2 * n + cap, 2 * n + 2 * cap])
    return dict(cur_return=cut[0].view(np.float32), cur_length=cut[1].astype(np.int64), win_return=cut[2].view(np.float32), win_length=cut[3].astype(np.int64),
                win_timed_out=cut[4].astype(np.int64), counters=s.counters.cpu().numpy(), sums=s.sums.cpu().numpy())


@pytest.fixture(scope="module")
def cases():
    """The inputs of every (n, cap, G), made once and shared."""
    return {(n, cap, G): ref.make_case(n, cap, G, seed=1000 * n + 10 * cap + G) for n in ref.NS for cap in ref.CAPS for G in ref.GROUPS}


@pytest.mark.parametrize("cap", ref.CAPS)
@pytest.mark.parametrize("n", ref.NS)
def test_add_matches_the_model_after_every_tick(cases, n, cap):
    for G in ref.GROUPS:
        groups, ticks = cases[(n, cap, G)]
        model = ref.Model(n, cap, G, groups)
        s = _stats(n, cap, G, groups)
        dev = [tuple(x.to(DEV) for x in tick) for tick in ticks]
        ref.check_summary(model, s.summary.cpu().numpy(), f"n {n} cap {cap} G {G} before the first tick")       # an empty window reads 0.0
        for t, (cpu, d) in enumerate(zip(ticks, dev)):
            model.add(*cpu)
            s.add(*d)
            what = f"n {n} cap {cap} G {G} tick {t}"
            ref.check_state(model, _state(s), what)
            ref.check_summary(model, s.summary.cpu().numpy(), what)
        assert _guards_intact(s), f"n {n} cap {cap} G {G}: a sentinel beside a buffer was overwritten"
        # a rerun is bit-identical, the summary included
        again = _stats(n, cap, G, groups)
        for d in dev:
            again.add(*d)
        again.summary
        for k in BUFFERS:
            assert torch.equal(again._raw[k], s._raw[k]), f"n {n} cap {cap} G {G}: rerun differs in {k}"


def test_no_groups_counts_everyone_in_group_zero(cases):
    n, cap = 65, 3
    _, ticks = cases[(n, cap, 1)]
    model = ref.Model(n, cap, 1, None)
    s = _stats(n, cap, 1, None)
    for tick in ticks:
        model.add(*tick)
        s.add(*(x.to(DEV) for x in tick))
    ref.check_state(model, _state(s), "no groups")
    out = s.read()
    assert out["groups"][0] == {k: out[k] for k in out["groups"][0]} and out["episodes"] == model.blocks[0]["episodes"] > 0
    assert out["terminations"] == out["episodes"] - out["time_outs"] and out["episodes_in_window"] == cap


def test_restart_and_clear_do_what_they_say_and_nothing_else(cases):
    n, cap, G = 1025, 100, 3
    groups, ticks = cases[(n, cap, G)]
    s = _stats(n, cap, G, groups)
    model = ref.Model(n, cap, G, groups)
    for tick in ticks[:15]:
        model.add(*tick)
        s.add(*(x.to(DEV) for x in tick))
    s.summary
    before = {k: s._raw[k].clone() for k in BUFFERS}
    assert bool(s.cur_length.any()) and bool(s.counters[E.COUNT] > 0)
    s.restart()
    model.restart()
    for k in BUFFERS:
        if k in ("cur_return", "cur_length"):
            assert not bool(getattr(s, k).any()), k
        else:
            assert torch.equal(s._raw[k], before[k]), k
    assert _guards_intact(s)
    for tick in ticks[15:25]:                                                    # and the bookkeeping goes on from there as the model's does
        model.add(*tick)
        s.add(*(x.to(DEV) for x in tick))
    ref.check_state(model, _state(s), "after restart")
    ref.check_summary(model, s.summary.cpu().numpy(), "after restart")
    s.clear()
    for k in BUFFERS:
        inner = s._raw[k][GUARD:-GUARD]
        assert not bool(inner.any()), k
    assert _guards_intact(s)
    fresh = ref.Model(n, cap, G, groups)
    for tick in ticks[25:]:
        fresh.add(*tick)
        s.add(*(x.to(DEV) for x in tick))
    ref.check_state(fresh, _state(s), "after clear")


def test_add_never_waits_for_the_device(cases):
    n, cap, G = 2113, 100, 8
    groups, ticks = cases[(n, cap, G)]
    dev = [tuple(x.to(DEV) for x in tick) for tick in ticks]
    model = ref.Model(n, cap, G, groups)
    s = _stats(n, cap, G, groups)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # a torch call that waits for the device or copies to the host raises from here on
    try:
        for d in dev:
            s.add(*d)
        s.restart()
        summary = s.summary
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert summary.is_cuda and summary.dtype == torch.float64 and summary.numel() == E.S_TOTALS + E.S_STRIDE * (1 + G)
    for tick in ticks:
        model.add(*tick)
    model.restart()
    ref.check_state(model, _state(s), "under sync debug mode")


def test_arguments_are_checked():
    s = E.EpisodeStats(8, window=3, device=DEV)
    rew, flag = torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.long, device=DEV)
    for bad in ((rew.double(), flag, flag), (rew, flag.int(), flag), (rew, flag, flag[:7]), (torch.zeros(16, device=DEV)[::2], flag, flag)):
        with pytest.raises(ValueError):
            s.add(*bad)
    with pytest.raises(rl_mpc_locomotion_amd._lib.MpcLibraryError):
        s.add(rew.cpu(), flag, flag)
    with pytest.raises(ValueError):
        E.EpisodeStats(8, groups=[0] * 7, device=DEV)
    with pytest.raises(rl_mpc_locomotion_amd._lib.MpcLibraryError):
        E.EpisodeStats(8, num_groups=E.MAX_GROUPS + 1, device=DEV)
    assert not bool(s.counters.any())


@pytest.mark.parametrize("n", (1, 65, 1100))
def test_random_progress_equals_the_host_build(tmp_path, n):
    shim = build_shim(tmp_path)
    for seed, max_len in ((1, 2000), (2 ** 63 + 5, 40), (3, 2 ** 31)):
        raw = torch.full((n + 2 * GUARD,), -7777, dtype=torch.long, device=DEV)
        E.random_progress(raw[GUARD:GUARD + n], max_len, seed)
        got = raw.cpu().numpy()
        assert np.array_equal(got[GUARD:GUARD + n], host_progress(shim, seed, n, max_len)), (n, seed, max_len)
        assert (got[:GUARD] == -7777).all() and (got[GUARD + n:] == -7777).all()


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------
N, T = 64, 4
TYPES = [i % 3 for i in range(N)]
NEW_KEYS = ("mean_episode_return", "mean_episode_length", "episodes_in_window", "episodes_finished", "timeouts_in_window")
OLD_KEYS = ("iter", "mean_reward", "done_rate", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate")


class _Recorder:
    """An environment that keeps what BatchedRLTask.step returned on each tick (device copies: its buffers are rewritten by the next step), and the
    episode lengths it was given before its first step."""

    def __init__(self, env, ticks):
        self.env, self.k = env, 0
        self.num_envs, self.num_obs, self.num_actions, self.device = env.num_envs, env.num_obs, env.num_actions, env.device
        self.cfg, self.progress_buf, self.first_progress = env.cfg, env.progress_buf, None
        self.rew = torch.zeros((ticks, env.num_envs), dtype=torch.float32, device=env.device)
        self.reset_rec = torch.zeros((ticks, env.num_envs), dtype=torch.long, device=env.device)
        self.time_outs = torch.zeros((ticks, env.num_envs), dtype=torch.long, device=env.device)

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        if self.first_progress is None:
            self.first_progress = self.progress_buf.clone()
        out = self.env.step(actions)
        self.rew[self.k].copy_(out[1]); self.reset_rec[self.k].copy_(out[2]); self.time_outs[self.k].copy_(out[3]["time_outs"])
        self.k += 1
        return out

    def ticks(self, lo, hi):
        return [(self.rew[t].cpu(), self.reset_rec[t].cpu(), self.time_outs[t].cpu()) for t in range(lo, hi)]


def _trainer(ticks, episode_length_s=0.03, steps=T, update="torch", seed=11):
    task = R.BatchedRLTask(TYPES, [TROT] * N, cfg=R.TaskConfig(episode_length_s=episode_length_s, seed=5), device=DEV)      # 0.03 s: 3-tick episodes
    env = _Recorder(task, ticks)
    cfg = P.PPOConfig(num_steps_per_env=steps, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,), init_noise_std=0.5)
    return P.PPOTrainer(env, cfg, seed=seed, update=update), env, task


def _check_window(info, model, what):
    count, mean_r, bound_r, mean_l, bound_l, timed = model.window()
    assert info["episodes_in_window"] == count and info["timeouts_in_window"] == timed and info["episodes_finished"] == model.blocks[0]["episodes"], what
    assert abs(info["mean_episode_return"] - mean_r) <= bound_r and abs(info["mean_episode_length"] - mean_l) <= bound_l, what


def test_learn_reports_the_models_episode_statistics():
    trainer, env, _ = _trainer(2 * T)
    infos = trainer.learn(2)
    model = ref.Model(N, 100)
    for it in range(2):
        for tick in env.ticks(it * T, (it + 1) * T):
            model.add(*tick)
        _check_window(infos[it], model, f"iteration {it}")
        assert list(infos[it]) == list(OLD_KEYS + NEW_KEYS) and np.isfinite(list(infos[it].values())).all()
    assert infos[1]["episodes_finished"] >= infos[0]["episodes_finished"] > 0 and 0 < infos[1]["episodes_in_window"] <= 100 and infos[1]["timeouts_in_window"] > 0
    assert infos[1]["mean_episode_return"] >= 0 and infos[1]["mean_episode_length"] >= 1
    # the existing keys against a trainer stepped the old way: collect + update by hand, the float32 values read as they are
    old, _, _ = _trainer(2 * T)
    for it in range(2):
        old.collect()
        mean_reward, done_rate = old.storage.rewards.mean(), old.storage.dones.mean()
        value_loss, surrogate = old.alg.update(old.storage)
        stats = torch.stack((mean_reward, done_rate, value_loss, surrogate, old.actor_critic.std.detach().mean())).tolist()
        want = dict(iter=it + 1, mean_reward=stats[0], done_rate=stats[1], value_loss=stats[2], surrogate_loss=stats[3], mean_noise_std=stats[4],
                    learning_rate=old.alg.learning_rate)
        assert {k: infos[it][k] for k in OLD_KEYS} == want, f"iteration {it}"


def _learn_recording_noise(trainer, iterations):
    eps, collect = [], trainer.collect
    trainer.collect = lambda: collect(record_eps=eps)
    try:
        trainer.learn(iterations)
    finally:
        trainer.collect = collect
    return torch.stack(eps)


def test_evaluate_counts_episodes_per_robot_type_and_leaves_training_alone():
    K = 6                                                                        # ticks per iteration: not a multiple of the episodes' period
    trainer, env, task = _trainer(K + 12 + K, steps=K)
    trainer.learn(1)
    st, ep = trainer.storage, trainer.episode_stats
    fields = ("observations", "actions", "mu", "sigma", "values", "rewards", "dones", "actions_log_prob", "returns", "advantages")
    before = dict(tick=trainer.tick, storage=[getattr(st, f).clone() for f in fields], params=[p.detach().clone() for p in trainer.actor_critic.parameters()],
                  window=[ep._raw[k].clone() for k in ("win_return", "win_length", "win_timed_out", "counters", "sums")], infos=len(trainer.infos))
    assert bool(ep.cur_length.any())                                             # episodes are under way
    out = trainer.evaluate(12, groups=TYPES, num_groups=3)
    model = ref.Model(N, 100, 3, TYPES)
    for tick in env.ticks(K, K + 12):
        model.add(*tick)
    assert env.k == K + 12
    keys = ["episodes", "time_outs", "terminations", "mean_return", "mean_length"]
    assert list(out) == keys + ["groups"] and len(out["groups"]) == 3 and all(list(g) == keys for g in out["groups"])
    for got, blk in zip([out] + out["groups"], model.blocks):
        k = blk["episodes"]
        assert k > 0 and (got["episodes"], got["time_outs"], got["terminations"]) == (k, blk["timeouts"], k - blk["timeouts"])
        bound = k * 2.0 ** -52 * math.fsum(abs(x) for x in blk["returns"]) / k
        assert abs(got["mean_return"] - math.fsum(blk["returns"]) / k) <= bound and abs(got["mean_length"] - blk["sum_length"] / k) <= 2.0 ** -52 * blk["sum_length"] / k
    assert sum(g["episodes"] for g in out["groups"]) == out["episodes"] >= N and out["time_outs"] > 0
    # training is where it was: the tick, the storage, every parameter, the window; the accumulators restarted; obs is the environment's latest
    assert trainer.tick == before["tick"] and len(trainer.infos) == before["infos"] and st.step == 0
    assert all(torch.equal(getattr(st, f), b) for f, b in zip(fields, before["storage"]))
    assert all(torch.equal(p, b) for p, b in zip(trainer.actor_critic.parameters(), before["params"]))
    assert all(torch.equal(ep._raw[k], b) for k, b in zip(("win_return", "win_length", "win_timed_out", "counters", "sums"), before["window"]))
    assert not bool(ep.cur_length.any()) and not bool(ep.cur_return.any())
    assert torch.equal(trainer.obs, task.obs_buf)
    # the next iteration draws the noise it would have drawn without the evaluation
    eps = _learn_recording_noise(trainer, 1)
    plain, _, _ = _trainer(2 * K, steps=K)
    plain.learn(1)
    assert torch.equal(eps, _learn_recording_noise(plain, 1)) and trainer.tick == plain.tick == 2 * K


def test_init_at_random_ep_len_spreads_the_time_outs(tmp_path):
    shim = build_shim(tmp_path)
    trainer, env, _ = _trainer(40, episode_length_s=0.4, steps=40, seed=7)       # 40-tick episodes
    assert env.cfg.max_episode_length == 40
    trainer.learn(1, init_at_random_ep_len=True)
    assert np.array_equal(env.first_progress.cpu().numpy(), host_progress(shim, 7, N, 40))
    per_tick = env.time_outs.cpu().numpy().astype(bool).sum(1)
    print("time-outs per tick:", per_tick.tolist())
    assert per_tick.sum() > 0 and (per_tick > 0).sum() > 1 and per_tick.max() < N

    class Bare:
        num_envs, num_obs, num_actions, device = N, 48, 12, torch.device(DEV)
    with pytest.raises(ValueError):
        P.PPOTrainer(Bare(), trainer.cfg, seed=1).learn(1, init_at_random_ep_len=True)


def test_the_device_update_reads_the_host_once_per_iteration(monkeypatch):
    trainer, env, _ = _trainer(T, update="hip")
    calls = dict(tolist=0, item=0, cpu=0)
    for name in calls:
        plain = getattr(torch.Tensor, name)

        def counted(self, *a, _name=name, _plain=plain, **kw):
            if self.is_cuda:
                calls[_name] += 1
            return _plain(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    infos = trainer.learn(1)
    assert calls == dict(tolist=1, item=0, cpu=0), calls
    monkeypatch.undo()
    model = ref.Model(N, 100)
    for tick in env.ticks(0, T):
        model.add(*tick)
    _check_window(infos[0], model, "hip backend")
    assert list(infos[0]) == list(OLD_KEYS + NEW_KEYS) and np.isfinite(list(infos[0].values())).all()
    assert infos[0]["learning_rate"] == float(trainer.alg.lr_device.item()) == trainer.alg.optimizer.param_groups[0]["lr"]
