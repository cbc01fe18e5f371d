"""The recurrent actor-critic on the MI355X (csrc/mpc_recurrent.h, csrc/recurrent_cell.h, rl_mpc_locomotion_amd.recurrent): the cell kernel against
torch's float32 nn.LSTM under the rule of tests/test_ppo.py's check_log_prob (4 x torch's own float32-vs-float64 gap, the float64 side being
tests/recurrent_ref.py), resets, saving and the uncommitted step bit for bit, the composition with the existing act kernel, the parameters read in
place, a roll of eight ticks, and the trainer: collection, update through time, checkpoints."""
import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import ppo as P, privileged_obs as V, recurrent as RC, rl_task as R
from tests import recurrent_ref as ref
from tests.test_policy import ACT_ATOL, ACT_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
HIDDEN = ((32, 16), (16,))
SHAPES = ((48, 16), (64, 32), (240, 256), (256, 256))
ROWS = (1, 15, 16, 17, 33)
A, C = RC.ACTOR, RC.CRITIC


def _pair(I, H, seed, critic_width=None):
    """The same random recurrent actor-critic on the CPU (torch's reference) and on the device: torch's default scale, biases x 0.1."""
    torch.manual_seed(seed)
    cpu = RC.ActorCriticRecurrent(I, 12, *HIDDEN, init_noise_std=0.5, num_critic_obs=critic_width, rnn_hidden_size=H)
    with torch.no_grad():
        for name, p in cpu.named_parameters():
            if p.dim() == 1 and name != "std":
                p.copy_(torch.randn_like(p) * 0.1)
    dev = RC.ActorCriticRecurrent(I, 12, *HIDDEN, init_noise_std=0.5, num_critic_obs=critic_width, rnn_hidden_size=H)
    dev.load_state_dict(cpu.state_dict())
    return cpu, dev.to(DEV)


def _inputs(n, widths, H, seed):
    """Rows for each memory and a random state in [-1, 1] for each: ([x_a, x_c], [(h, c), (h, c)]) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, w, generator=g) for w in widths]
    states = [(torch.rand(n, H, generator=g) * 2 - 1, torch.rand(n, H, generator=g) * 2 - 1) for _ in widths]
    return xs, states


def _set_state(dev, states, n):
    for m, (h, c) in zip(dev.memories(), states):
        dh, dc, _ = m.state(n, torch.device(DEV))
        dh.copy_(h); dc.copy_(c)


def _lstm32(mem, x, h, c):
    """torch's float32 CPU nn.LSTM, one step."""
    with torch.no_grad():
        _, (h1, c1) = mem.rnn(x[None], (h[None].contiguous(), c[None].contiguous()))
    return h1[0], c1[0]


def _check_gap(got, t32, t64, what, floor=64):
    """check_log_prob's rule over everything given together: lists of (kernel, torch float32, float64) tensors of equal shapes."""
    cat = lambda ts: torch.cat([t.detach().double().reshape(-1).cpu() for t in ts])
    g, a, b = cat(got), cat(t32), cat(t64)
    assert g.numel() >= floor
    gap = float((a - b).abs().max())
    d = float((g - a).abs().max())
    print(f"{what}: off torch's float32 by {d:.3e}, gap {gap:.3e}, ratio {d / gap if gap > 0 else float('inf'):.3f} (bound 4)")
    assert gap > 0 and d <= 4 * gap, f"{what}: off by {d:.3e} > 4 x {gap:.3e}"


@pytest.mark.parametrize("I,H", SHAPES)
def test_cell_against_float64(I, H):
    cpu, dev = _pair(I, H, seed=I + H)
    got, t32, t64 = [], [], []
    for n in ROWS:
        xs, states = _inputs(n, (I, I), H, seed=n)
        _set_state(dev, states, n)
        outs = dev.cell_step({A: xs[0].to(DEV), C: xs[1].to(DEV)})
        for m_cpu, m_dev, x, (h, c), out in zip(cpu.memories(), dev.memories(), xs, states, outs):
            assert torch.equal(out, m_dev.h)                                     # committed: the state is h'
            h32, c32 = _lstm32(m_cpu, x, h, c)
            h64, c64 = ref.cell(x, h, c, *m_cpu.parameters_in_bind_order())
            got += [out, m_dev.c]; t32 += [h32, c32]; t64 += [h64, c64]
    _check_gap(got, t32, t64, f"cell I={I} H={H}")


def test_resets_saving_and_the_uncommitted_step():
    I, Wc, H, n = 64, 48, 32, 33
    _, dev = _pair(I, H, seed=4, critic_width=Wc)
    xs, states = _inputs(n, (I, Wc), H, seed=9)
    rows = {A: xs[0].to(DEV), C: xs[1].to(DEV)}
    flagged = [0, 15, 16, n - 1]
    reset = torch.zeros(n, dtype=torch.long, device=DEV)
    reset[flagged] = torch.tensor([1, 7, -1, 1], device=DEV)                     # any non-zero value is a reset
    keep = (reset == 0).cpu()
    nan = lambda: torch.full((n, H), float("nan"), device=DEV)
    saved = dict(h_a=nan(), c_a=nan(), h_c=nan(), c_c=nan())
    # commit = 0: the state stays, the output is written
    _set_state(dev, states, n)
    peek = [o.clone() for o in dev.cell_step(rows, reset, None, commit=False)]
    for m, (h, c) in zip(dev.memories(), states):
        assert torch.equal(m.h.cpu(), h) and torch.equal(m.c.cpu(), c)
    # commit = 1 with saving
    outs = [o.clone() for o in dev.cell_step(rows, reset, saved)]
    after = [(m.h.clone(), m.c.clone()) for m in dev.memories()]
    for k, (h, c) in zip(("a", "c"), states):
        sh, sc = saved["h_" + k].cpu(), saved["c_" + k].cpu()
        assert torch.equal(sh[keep], h[keep]) and torch.equal(sc[keep], c[keep])                     # bit for bit
        assert not sh[~keep].any() and not sc[~keep].any() and not torch.isnan(sh).any() and not torch.isnan(sc).any()
    for p, o, (h1, _) in zip(peek, outs, after):
        assert torch.equal(p, o) and torch.equal(o, h1)
    # the state zeroed by hand, no flags: the same output and state on every row
    zeroed = [(h * keep[:, None], c * keep[:, None]) for h, c in states]
    _set_state(dev, zeroed, n)
    by_hand = dev.cell_step(rows)
    for o, b, m, (h1, c1) in zip(outs, by_hand, dev.memories(), after):
        assert torch.equal(o, b) and torch.equal(m.h, h1) and torch.equal(m.c, c1)
    # one memory at a time: what evaluate and act_inference launch
    _set_state(dev, states, n)
    only_c, = dev.cell_step({C: rows[C]}, reset, None, commit=False)
    assert torch.equal(only_c, outs[1]) and torch.equal(dev.memory_a.h.cpu(), states[0][0])
    only_a, = dev.cell_step({A: rows[A]}, reset)
    assert torch.equal(only_a, outs[0]) and torch.equal(dev.memory_c.h.cpu(), states[1][0]) and torch.equal(dev.memory_a.c, after[0][1])


def test_act_is_the_cell_and_then_the_existing_act_kernel():
    I, Wc, H, n = 48, 64, 32, 33
    _, dev = _pair(I, H, seed=6, critic_width=Wc)
    plain = P.ActorCritic(H, 12, *HIDDEN, num_critic_obs=H)
    plain.load_state_dict({k: v for k, v in dev.state_dict().items() if not k.startswith("memory_")})
    plain = plain.to(DEV)
    xs, states = _inputs(n, (I, Wc), H, seed=2)
    _set_state(dev, states, n)
    with pytest.raises(ValueError, match="critic_obs"):
        dev.act(xs[0].to(DEV), 5, 3)
    out = dev.act(xs[0].to(DEV), seed=5, step=3, critic_obs=xs[1].to(DEV), return_eps=True)
    want = plain.act(dev.memory_a.out.clone(), seed=5, step=3, critic_obs=dev.memory_c.out.clone(), return_eps=True)
    for k in ("mu", "values", "actions", "actions_log_prob", "sigma", "eps"):
        assert torch.equal(out[k], want[k]), k
    assert torch.equal(dev.memory_a.out, dev.memory_a.h) and torch.equal(dev.memory_c.out, dev.memory_c.h)
    # evaluate peeks at the critic's memory, act_inference steps the actor's alone
    before = [(m.h.clone(), m.c.clone()) for m in dev.memories()]
    values = dev.evaluate(xs[1].to(DEV))
    assert torch.equal(values, plain.evaluate(dev.memory_c.out.clone()))
    for m, (h, c) in zip(dev.memories(), before):
        assert torch.equal(m.h, h) and torch.equal(m.c, c)
    mean = dev.act_inference(xs[0].to(DEV))
    assert torch.equal(mean, plain.act_inference(dev.memory_a.h.clone())) and not torch.equal(dev.memory_a.h, before[0][0])
    assert torch.equal(dev.memory_c.h, before[1][0]) and torch.equal(dev.memory_c.c, before[1][1])
    dev.reset_memory()
    assert not any(t.any() for m in dev.memories() for t in (m.h, m.c))


def test_parameters_are_read_in_place():
    I, H, n = 48, 32, 64
    cpu, dev = _pair(I, H, seed=8)
    xs, states = _inputs(n, (I, I), H, seed=3)
    obs = xs[0].to(DEV)
    _set_state(dev, states, n)
    before = dev.act(obs, seed=1, step=0)
    h_before = dev.memory_a.out.clone()
    with torch.no_grad():
        delta = torch.randn_like(cpu.memory_a.rnn.weight_hh_l0) * 0.2
        cpu.memory_a.rnn.weight_hh_l0.add_(delta)
        dev.memory_a.rnn.weight_hh_l0.add_(delta.to(DEV))                        # in place: the same address, no rebinding
    _set_state(dev, states, n)
    after = dev.act(obs, seed=1, step=0)
    assert (dev.memory_a.out - h_before).abs().max() > 1e-2 and (after["mu"] - before["mu"]).abs().max() > 100 * ACT_ATOL
    assert torch.equal(after["values"], before["values"])                        # (the critic's memory was not touched)
    h32, c32 = _lstm32(cpu.memory_a, xs[0], *states[0])
    h64, c64 = ref.cell(xs[0], *states[0], *cpu.memory_a.parameters_in_bind_order())
    _check_gap([dev.memory_a.out, dev.memory_a.c], [h32, c32], [h64, c64], "after an in-place add_")


def test_a_wide_cell_survives_the_bind_of_a_narrow_one():
    """cell_kernel's dynamic-LDS limit is one per device and kernel: the bind of a handle with small memories must not lower what a handle with
    wide ones launches with.  Wide: the smallest I = H (multiples of 16) whose 64 (I + H + 8) bytes reach 69 632, the deployed policy's need and
    the one size this project has recorded as over the default limit."""
    I = H = 544
    assert 64 * (I + H + 8) >= 69632 > 64 * (I - 16 + H - 16 + 8)
    n = 33                                                                       # two full workgroups and a partial one
    _, wide = _pair(I, H, seed=21)
    _, narrow = _pair(48, 32, seed=22)
    xs, states = _inputs(n, (I, I), H, seed=23)
    rows = {A: xs[0].to(DEV), C: xs[1].to(DEV)}

    def run():
        _set_state(wide, states, n)
        outs = wide.cell_step(rows)
        return [t.clone() for t in outs] + [t.clone() for m in wide.memories() for t in (m.h, m.c)]
    before = run()
    assert all(bool(torch.isfinite(t).all()) for t in before) and not torch.equal(before[2].cpu(), states[0][0])
    small_xs, small_states = _inputs(n, (48, 48), 32, seed=24)
    _set_state(narrow, small_states, n)
    small = narrow.cell_step({A: small_xs[0].to(DEV), C: small_xs[1].to(DEV)})   # creates and binds the narrow handle
    assert all(bool(torch.isfinite(t).all()) for t in small)
    after = run()
    assert len(after) == 6 and all(torch.equal(a, b) for a, b in zip(after, before))


def test_roll_of_eight_ticks_with_resets():
    T, n, I, H = 8, 33, 48, 32
    cpu, dev = _pair(I, H, seed=10)
    g = torch.Generator().manual_seed(12)
    xs = torch.randn(T, n, I, generator=g)
    resets = torch.zeros(T, n, dtype=torch.long)
    for t in (2, 3, 6):
        resets[t] = (torch.rand(n, generator=g) < 0.3).long()
    resets[5, [0, 15, 16, n - 1]] = 1
    _, states = _inputs(n, (I,), H, seed=13)
    h0, c0 = states[0]
    _set_state(dev, [(h0, c0), (h0, c0)], n)
    d_xs, d_resets = xs.to(DEV), resets.to(DEV)
    saved = {k: torch.zeros(T, n, H, device=DEV) for k in ("h_a", "c_a", "h_c", "c_c")}
    hs, cs = [], []
    for t in range(T):
        out, _ = dev.cell_step({A: d_xs[t], C: d_xs[t]}, d_resets[t] if t > 0 else None, {k: v[t] for k, v in saved.items()})
        hs.append(out.clone()); cs.append(dev.memory_a.c.clone())
    h32, c32, h, c = [], [], h0, c0
    for t in range(T):                                                           # torch's float32 roll of the same eight steps
        keep = (resets[t] == 0).float()[:, None] if t > 0 else 1.0
        h, c = _lstm32(cpu.memory_a, xs[t], h * keep, c * keep)
        h32.append(h); c32.append(c)
    resets[0] = 0
    h64, c64, sh64, sc64 = ref.roll(xs, resets, h0, c0, cpu.memory_a.parameters_in_bind_order())
    _check_gap([torch.stack(hs), torch.stack(cs)], [torch.stack(h32), torch.stack(c32)], [h64, c64], "roll of 8 ticks")
    assert torch.equal(saved["h_a"][0].cpu(), h0) and torch.equal(saved["c_a"][1:], torch.stack(cs)[:-1] * (d_resets[1:] == 0)[..., None])
    assert not saved["h_a"][5][[0, 15, 16, n - 1]].any()


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, H_TRAIN = 32, 4, 32


def _pcfg():
    return P.PPOConfig(num_steps_per_env=T_STEPS, num_mini_batches=2, num_learning_epochs=1, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,),
                       init_noise_std=0.5)


def _task(privileged=False):
    return R.BatchedRLTask([i % 3 for i in range(N_ENVS)], [TROT] * N_ENVS, cfg=R.TaskConfig(episode_length_s=0.03, seed=5), device=DEV,      # 3-tick episodes
                           privileged_obs=V.PrivilegedObs(N_ENVS, device=DEV) if privileged else None)


@pytest.fixture(scope="module")
def task():
    return _task()


def test_trainer_collection_fills_the_saved_states_and_matches_the_torch_path(task):
    trainer = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=RC.RecurrentConfig(hidden_size=H_TRAIN))
    ac, st = trainer.actor_critic, trainer.storage
    assert isinstance(ac, RC.ActorCriticRecurrent) and ac.memory_a.rnn.input_size == task.num_obs and ac.actor[0].in_features == H_TRAIN
    saved = (st.saved_h_a, st.saved_c_a, st.saved_h_c, st.saved_c_c)
    assert all(x.shape == (T_STEPS, N_ENVS, H_TRAIN) for x in saved)
    for x in saved:
        x.fill_(float("nan"))
    trainer.obs = trainer._first_obs()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # a torch call that waits for the device or copies to the host raises from here on
    try:
        trainer.collect()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not any(torch.isnan(x).any() for x in saved) and not any(x[0].any() for x in saved)       # filled; the first tick started from zero
    dones = st.dones[:, :, 0].bool()
    assert dones.any() and not dones.all()
    for x in saved:                                                              # zero after a done, the committed state otherwise
        assert not x[1:][dones[:-1]].any() and x[1:][~dones[:-1]].abs().sum(-1).min() > 0
    assert torch.equal(ac.memory_a.h, ac.memory_a.out) and not torch.equal(ac.memory_c.h, ac.memory_c.out)      # last_values peeked: h_c' was not committed
    # the float32 torch path from the saved t = 0 state reproduces the device's means and values
    cpu = RC.ActorCriticRecurrent(task.num_obs, 12, (64, 32), (32,), rnn_hidden_size=H_TRAIN)
    cpu.load_state_dict({k: v.cpu() for k, v in ac.state_dict().items()})
    state = ((st.saved_h_a[0].cpu(), st.saved_c_a[0].cpu()), (st.saved_h_c[0].cpu(), st.saved_c_c[0].cpu()))
    obs, host_dones = st.observations.cpu(), st.dones.cpu()
    with torch.no_grad():
        for t in range(T_STEPS):
            mu, value, state, used = cpu.step_torch(obs[t], None, state, host_dones[t - 1, :, 0] if t > 0 else None)
            np.testing.assert_allclose(st.mu[t].cpu().numpy(), mu.numpy(), rtol=ACT_RTOL, atol=ACT_ATOL, err_msg=f"mu, tick {t}")
            np.testing.assert_allclose(st.values[t].cpu().numpy(), value.numpy(), rtol=ACT_RTOL, atol=ACT_ATOL, err_msg=f"values, tick {t}")
            np.testing.assert_allclose(st.saved_c_a[t].cpu().numpy(), used[0][1].numpy(), rtol=ACT_RTOL, atol=ACT_ATOL, err_msg=f"saved c, tick {t}")


def test_trainer_learns_and_round_trips_checkpoints(task, tmp_path):
    trainer = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=RC.RecurrentConfig(hidden_size=H_TRAIN))
    ac = trainer.actor_critic
    # learn: finite records, every memory parameter moves
    before = {k: v.clone() for k, v in ac.state_dict().items() if k.startswith("memory_")}
    infos = trainer.learn(2)
    assert len(infos) == 2 and all(np.isfinite(v) for info in infos for v in info.values() if isinstance(v, float))
    assert len(before) == 8 and all(not torch.equal(ac.state_dict()[k], v) for k, v in before.items())
    # the checkpoint
    path = str(tmp_path / "model.pt")
    trainer.save(path)
    ck = torch.load(path)
    assert sorted(ck) == ["infos", "iter", "model_state_dict", "optimizer_state_dict"] and "memory_c.rnn.bias_hh_l0" in ck["model_state_dict"]
    fresh = P.PPOTrainer(task, _pcfg(), seed=4, recurrent=RC.RecurrentConfig(hidden_size=H_TRAIN))
    probe = torch.randn(50, task.num_obs, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    trainer.actor_critic.reset_memory()
    want = [trainer.actor_critic.act_inference(probe).clone() for _ in range(2)]
    assert not torch.equal(fresh.actor_critic.act_inference(probe), want[0])
    fresh.load(path)
    assert fresh.iteration == 2
    fresh.actor_critic.reset_memory()
    assert all(torch.equal(fresh.actor_critic.act_inference(probe), w) for w in want)
    # a checkpoint of the other kind is refused, both ways
    flat = P.PPOTrainer(task, _pcfg(), seed=4)
    with pytest.raises(ValueError, match="recurrent"):
        flat.load(path)
    flat_path = str(tmp_path / "flat.pt")
    flat.save(flat_path)
    with pytest.raises(ValueError, match="feed-forward"):
        fresh.load(flat_path)
    # evaluate starts episodes from zero state and leaves the memories zeroed
    result = fresh.evaluate(8)
    assert result["episodes"] > 0 and fresh._prev_reset is None and fresh.actor_critic.memory_a.h.shape == (N_ENVS, H_TRAIN)
    assert not any(t.any() for m in fresh.actor_critic.memories() if m.h is not None for t in (m.h, m.c))      # (the critic's memory was never stepped here)


def test_trainer_with_privileged_rows_and_normalisation():
    task = _task(privileged=True)
    trainer = P.PPOTrainer(task, _pcfg(), seed=3, normalize_obs=True, recurrent=RC.RecurrentConfig(hidden_size=H_TRAIN))
    ac = trainer.actor_critic
    assert ac.memory_a.rnn.input_size == task.num_obs and ac.memory_c.rnn.input_size == task.num_privileged_obs and ac.critic[0].in_features == H_TRAIN
    info = trainer.learn(1)[0]
    assert all(np.isfinite(info[k]) for k in ("mean_reward", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate"))
    assert torch.isfinite(trainer.storage.saved_h_c).all() and trainer.storage.saved_h_c[1:].any()
    with pytest.raises(ValueError, match="not built"):
        P.PPOTrainer(task, _pcfg(), update="hip", recurrent=RC.RecurrentConfig(hidden_size=H_TRAIN))
