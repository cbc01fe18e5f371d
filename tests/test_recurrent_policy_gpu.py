"""The deployed recurrent weight policy on the MI355X (csrc/mpc_recurrent_policy.h, csrc/recurrent_policy.h, weight_policy.RecurrentWeightPolicy): the
fused launch against torch's float32 path under the rule of tests/test_recurrent_gpu.py's _check_gap (4 x torch's own float32-vs-float64 gap, the float64
side being tests/recurrent_policy_ref.py), bit for bit against the two launches it fuses (the cell kernel, then the feed-forward policy kernel on h'),
resets and bounds, a roll of eight ticks that never waits for the device, the controller's run_policy, and a trainer's checkpoint."""
import functools

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, ppo as P, recurrent as RC, rl_task as R, weight_policy as WP
from tests import recurrent_policy_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
ROWS = (1, 15, 16, 17, 33)
# (I, H, the actor's hidden widths): one column block for eight waves; two; nine blocks -- an uneven second trip; the deployment shape
SHAPES = ((48, 16, (32, 16)), (64, 32, (16,)), (48, 144, (32,)), (48, 256, (512, 256, 128)))
DEPLOYED = SHAPES[3]
A = RC.ACTOR
SENTINEL = -777.25


@functools.lru_cache(maxsize=None)
def _pair(I, H, hidden, seed=None):
    """tests/test_recurrent_gpu.py's _pair recipe: the same random recurrent actor-critic on the CPU (torch's reference) and on the device -- torch's
    default scale, biases x 0.1 -- and, of its actor, the fused policy and the feed-forward policy that reads h'.  Shared, never modified."""
    torch.manual_seed(I + H if seed is None else seed)
    make = lambda: RC.ActorCriticRecurrent(I, 12, hidden, (16,), init_noise_std=0.5, rnn_hidden_size=H)
    cpu = make()
    with torch.no_grad():
        for name, p in cpu.named_parameters():
            if p.dim() == 1 and name != "std":
                p.copy_(torch.randn_like(p) * 0.1)
    dev = make()
    dev.load_state_dict(cpu.state_dict())
    fused = WP.WeightPolicy.from_state_dict(cpu.state_dict(), device=DEV)
    assert type(fused) is WP.RecurrentWeightPolicy and fused.num_obs == I and fused.hidden_size == H and fused.dims == [H, *hidden, 12]
    plain = WP.WeightPolicy(WP.actor_layers(cpu.state_dict()), device=DEV)
    return cpu, dev.to(DEV), fused, plain


def _inputs(n, I, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, I, generator=g), torch.rand(n, H, generator=g) * 2 - 1, torch.rand(n, H, generator=g) * 2 - 1


def _flags(n, seed):
    """Reset flags for n rows: the first, the last, the rows either side of a workgroup's edge, and a random third of the rest."""
    g = torch.Generator().manual_seed(seed)
    f = (torch.rand(n, generator=g) < 0.3).long()
    idx = [k for k in (0, 15, 16, n - 1) if k < n]
    f[idx] = torch.tensor([1, 7, -1, 1])[:len(idx)]                              # any non-zero value is a reset
    if n > 2:
        f[1] = 0
    return f


def _set(fused, h, c):
    n = h.shape[0]
    dh, dc = fused.state(n)
    dh.copy_(h); dc.copy_(c)


def _set_memory(dev, h, c):
    dh, dc, _ = dev.memory_a.state(h.shape[0], torch.device(DEV))
    dh.copy_(h); dc.copy_(c)


def _lstm32(mem, x, h, c):
    """torch's float32 CPU nn.LSTM, one step."""
    with torch.no_grad():
        _, (h1, c1) = mem.rnn(x[None], (h[None].contiguous(), c[None].contiguous()))
    return h1[0], c1[0]


def _check_gap(got, t32, t64, what, floor=64):
    """tests/test_recurrent_gpu.py's rule over everything given together: lists of (kernel, torch float32, float64) tensors of equal shapes.  The gap
    is the largest difference between torch's float32 path and the float64 restatement; the kernel may be off torch's float32 by 4 gaps."""
    cat = lambda ts: torch.cat([t.detach().double().reshape(-1).cpu() for t in ts])
    g, a, b = cat(got), cat(t32), cat(t64)
    assert g.numel() >= floor
    gap = float((a - b).abs().max())
    d = float((g - a).abs().max())
    print(f"{what}: off torch's float32 by {d:.3e}, gap {gap:.3e}, ratio {d / gap if gap > 0 else float('inf'):.3f} (bound 4)")
    assert gap > 0 and d <= 4 * gap, f"{what}: off by {d:.3e} > 4 x {gap:.3e}"
    return d / gap


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,H,hidden", SHAPES)
def test_fused_tick_against_float64(I, H, hidden):
    cpu, _, fused, _ = _pair(I, H, hidden)
    lstm, layers = pref.params(cpu.state_dict())
    got, t32, t64 = ([], [], []), ([], [], []), ([], [], [])
    for n in ROWS:
        x, h, c = _inputs(n, I, H, seed=n)
        _set(fused, h, c)
        weights, actions = fused.step(x.to(DEV), return_actions=True)
        h32, c32 = _lstm32(cpu.memory_a, x, h, c)
        with torch.no_grad():
            a32 = cpu.actor(h32)
        h64, c64, a64, _ = pref.tick(x, h, c, lstm, layers)
        for k, (g, a, b) in enumerate(((fused.h, h32, h64), (fused.c, c32, c64), (actions, a32, a64))):
            got[k].append(g.clone()); t32[k].append(a); t64[k].append(b)
        assert torch.equal(weights, torch.clamp(actions, -1, 1) * torch.tensor(WP.MPC_PARAM_SCALE, device=DEV) + torch.tensor(WP.MPC_PARAM_CONST, device=DEV))
    for k, name in enumerate(("h'", "c'", "raw actions")):                       # for the record: each output under its own gap
        cat = lambda ts: torch.cat([t.detach().double().reshape(-1).cpu() for t in ts])
        d, gap = float((cat(got[k]) - cat(t32[k])).abs().max()), float((cat(t32[k]) - cat(t64[k])).abs().max())
        print(f"  {name}: off {d:.3e}, own gap {gap:.3e}, ratio {d / gap:.3f}")
    _check_gap(sum(got, []), sum(t32, []), sum(t64, []), f"fused tick I={I} H={H} actor {hidden}")


# ---- 2. bit for bit against the two launches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,H,hidden", SHAPES)
def test_fused_tick_equals_the_two_launch_composition(I, H, hidden):
    _, dev, fused, plain = _pair(I, H, hidden)
    for n in ROWS:
        x, h, c = _inputs(n, I, H, seed=100 + n)
        obs = x.to(DEV)
        for reset in (None, _flags(n, seed=n).to(DEV)):
            _set(fused, h, c)
            _set_memory(dev, h, c)
            weights, actions = fused.step(obs, reset=reset, return_actions=True)
            h1, = dev.cell_step({A: obs}, reset)
            w2, a2 = plain.step(h1, return_actions=True)
            what = f"n={n} reset={'None' if reset is None else 'flags'}"
            assert torch.equal(fused.h, dev.memory_a.h) and torch.equal(fused.h, h1), what      # equality is the claim: every output is summed in the same order
            assert torch.equal(fused.c, dev.memory_a.c), what
            assert torch.equal(actions, a2) and torch.equal(weights, w2), what
            assert torch.equal(fused.step(obs, reset=reset), plain.step(dev.cell_step({A: obs}, reset)[0])), what      # a second tick, without the actions


# ---- 3. resets and bounds -----------------------------------------------------------------------------------------------------------------------------
def _raw_step(fused, n, obs, h, c, reset, actions, weights):
    """mpc_recurrent_policy_step on the caller's own buffers."""
    WP.recurrent_check(WP.recurrent_lib().mpc_recurrent_policy_step(fused._handle, n, obs.data_ptr(), h.data_ptr(), c.data_ptr(),
                                                                    reset.data_ptr() if reset is not None else None,
                                                                    actions.data_ptr() if actions is not None else None, weights.data_ptr(),
                                                                    _lib.stream(torch.device(DEV))), "mpc_recurrent_policy_step")


@pytest.mark.parametrize("I,H,hidden", (SHAPES[1], SHAPES[2]))
def test_resets_and_bounds(I, H, hidden):
    _, _, fused, _ = _pair(I, H, hidden)
    for n in ROWS:
        x, h, c = _inputs(n, I, H, seed=200 + n)
        obs = x.to(DEV)
        flags = _flags(n, seed=3 * n)
        keep = (flags == 0)
        guarded = lambda width: torch.full((n + 16, width), SENTINEL, device=DEV)      # 16 spare rows behind the n the kernel may write

        def run(h0, c0, reset, with_actions=True):
            gh, gc, ga, gw = guarded(H), guarded(H), guarded(12), guarded(12)
            gh[:n].copy_(h0); gc[:n].copy_(c0)
            _raw_step(fused, n, obs, gh, gc, reset, ga if with_actions else None, gw)
            for t in (gh, gc, ga, gw):
                assert bool((t[n:] == SENTINEL).all()), f"n={n}: a row past n was written"
            if not with_actions:
                assert bool((ga == SENTINEL).all())
            return gh[:n].clone(), gc[:n].clone(), ga[:n].clone(), gw[:n].clone()
        flagged = run(h, c, flags.to(DEV))
        by_hand = run(h * keep[:, None], c * keep[:, None], None)                # the flagged rows' state zeroed by hand, no flags
        for a, b in zip(flagged, by_hand):
            assert torch.equal(a, b), f"n={n}"
        unflagged = run(h, c, None)
        zero_flags = run(h, c, torch.zeros(n, dtype=torch.long, device=DEV))
        for a, b, f in zip(unflagged, zero_flags, flagged):
            assert torch.equal(a, b), f"n={n}: reset=None is all-zero flags"
            assert torch.equal(a[keep], f[keep]), f"n={n}: a flag moved an unflagged row"
        if bool((~keep).any()) and bool(h[~keep].any()):
            assert not torch.equal(unflagged[0][~keep], flagged[0][~keep])
        no_actions = run(h, c, None, with_actions=False)
        assert torch.equal(no_actions[0], unflagged[0]) and torch.equal(no_actions[1], unflagged[1]) and torch.equal(no_actions[3], unflagged[3])
    # reset_memory: all rows, the given rows (a device index, a list), and a new n starts from zero
    n = 33
    x, h, c = _inputs(n, I, H, seed=9)
    _set(fused, h, c)
    ids = torch.tensor([0, 15, 16, 32], device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fused.reset_memory(ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rest = torch.ones(n, dtype=torch.bool)
    rest[ids.cpu()] = False
    assert not fused.h[ids].any() and not fused.c[ids].any() and torch.equal(fused.h[rest].cpu(), h[rest]) and torch.equal(fused.c[rest].cpu(), c[rest])
    fused.reset_memory([1, 2])
    assert not fused.h[:3].any() and torch.equal(fused.h[3:15].cpu(), h[3:15])
    fused.reset_memory()
    assert not fused.h.any() and not fused.c.any()
    _set(fused, h, c)
    fused.step(torch.zeros(5, I, device=DEV))
    assert fused.h.shape == (5, H) and fused.c.shape == (5, H)
    with pytest.raises(ValueError, match="obs"):
        fused.step(torch.zeros(5, I + 16, device=DEV))
    with pytest.raises(ValueError, match="reset"):
        fused.step(torch.zeros(5, I, device=DEV), reset=torch.zeros(5, dtype=torch.int32, device=DEV))


def test_a_wide_policy_survives_the_creation_of_a_narrow_one():
    """The deployment shape needs more dynamic LDS than a kernel gets by default; a later handle with a small net must not lower the limit."""
    I, H, hidden = DEPLOYED
    _, _, wide, _ = _pair(I, H, hidden)
    x, h, c = _inputs(33, I, H, seed=31)
    _set(wide, h, c)
    before = [t.clone() for t in wide.step(x.to(DEV), return_actions=True)] + [wide.h.clone(), wide.c.clone()]
    narrow = WP.RecurrentWeightPolicy.from_state_dict(_pair(*SHAPES[0])[0].state_dict(), device=DEV)
    assert torch.isfinite(narrow.step(torch.zeros(5, SHAPES[0][0], device=DEV))).all()
    _set(wide, h, c)
    after = list(wide.step(x.to(DEV), return_actions=True)) + [wide.h, wide.c]
    assert all(torch.equal(a, b) for a, b in zip(after, before)) and bool(torch.isfinite(after[0]).all())


# ---- 4. a roll ------------------------------------------------------------------------------------------------------------------------------------------
def test_roll_of_eight_ticks_with_resets():
    T, n = 8, 33
    I, H, hidden = DEPLOYED
    cpu, dev, fused, _ = _pair(I, H, hidden)
    g = torch.Generator().manual_seed(12)
    xs = torch.randn(T, n, I, generator=g)
    resets = torch.zeros(T, n, dtype=torch.long)
    for t in (2, 3, 6):
        resets[t] = (torch.rand(n, generator=g) < 0.3).long()
    resets[5, [0, 15, 16, n - 1]] = 1
    _, h0, c0 = _inputs(n, I, H, seed=13)
    d_xs, d_resets = xs.to(DEV), resets.to(DEV)
    fused.step(d_xs[0])                                                          # (the code object is loaded before the no-wait section)
    _set(fused, h0, c0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # a torch call that waits for the device or copies to the host raises from here on
    try:
        hs, cs, acts, ws = [], [], [], []
        for t in range(T):
            w, a = fused.step(d_xs[t], reset=d_resets[t] if t > 0 else None, return_actions=True)
            hs.append(fused.h.clone()); cs.append(fused.c.clone()); acts.append(a); ws.append(w)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the live two-launch path, tick by tick
    _set_memory(dev, h0, c0)
    for t in range(T):
        mean = dev.act_inference(d_xs[t], reset=d_resets[t] if t > 0 else None)
        assert torch.equal(mean, acts[t]) and torch.equal(dev.memory_a.h, hs[t]) and torch.equal(dev.memory_a.c, cs[t]), t
    # torch's float32 roll and the float64 roll of the same eight ticks
    h32, c32, a32, h, c = [], [], [], h0, c0
    for t in range(T):
        keep = (resets[t] == 0).float()[:, None] if t > 0 else 1.0
        h, c = _lstm32(cpu.memory_a, xs[t], h * keep, c * keep)
        with torch.no_grad():
            a32.append(cpu.actor(h))
        h32.append(h); c32.append(c)
    resets[0] = 0
    h64, c64, a64, _ = pref.roll(xs, resets, h0, c0, *pref.params(cpu.state_dict()))
    _check_gap([torch.stack(hs), torch.stack(cs), torch.stack(acts)], [torch.stack(h32), torch.stack(c32), torch.stack(a32)], [h64, c64, a64], "roll of 8 ticks")


# ---- 5. through the controller --------------------------------------------------------------------------------------------------------------------------
def test_run_policy_with_a_recurrent_policy_equals_its_unfused_composition():
    from rl_mpc_locomotion_amd.locomotion import BatchedLocomotion
    from rl_mpc_locomotion_amd.quadruped import ROBOT_TABLE64
    from rl_mpc_locomotion_amd.synthetic import TickStream
    I, H, hidden = DEPLOYED
    _, dev, fused, plain = _pair(I, H, hidden)
    n = 48
    ts = TickStream(n, seed=13, config=3)
    a = BatchedLocomotion(ts.robot_type, ts.gait_id, horizon=10)
    b = BatchedLocomotion(ts.robot_type, ts.gait_id, horizon=10)
    for ctl in (a, b):
        ctl.fsm_init(np.full(n, BatchedLocomotion.LOCOMOTION), operating_mode=1, check_safety=True)
    req = torch.full((n,), BatchedLocomotion.LOCOMOTION, dtype=torch.int32, device=DEV)
    wa = wb = torch.from_numpy(np.tile(ROBOT_TABLE64[0, 12:24].astype(np.float32), (n, 1))).to(DEV)
    fused.state(n)
    fused.reset_memory()                                                         # both memories from zero state
    dev.memory_a.state(n, torch.device(DEV))
    dev.reset_memory()
    some = torch.zeros(n, dtype=torch.long, device=DEV)
    some[[0, 15, 16, 31, 47]] = 1
    for tick in range(6):
        dof, body, cmd16 = ts.tick(tick)
        dof_t, body_t = torch.from_numpy(dof).to(DEV), torch.from_numpy(body).to(DEV)
        cmd3 = torch.from_numpy(np.ascontiguousarray(cmd16[:, :3])).to(DEV)
        reset = some if tick == 3 else None
        if reset is None:                                                        # (today's call, without the argument)
            ta, wa = a.run_policy(fused, dof_t, body_t, cmd3, wa, req)
        else:
            ta, wa = a.run_policy(fused, dof_t, body_t, cmd3, wa, req, reset=reset)
        ta = ta.clone()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mpc_ctrl_update_estimate(b._handle, body_t.data_ptr(), stream), "mpc_ctrl_update_estimate")
        est, nrm = b.estimate()
        h1, = dev.cell_step({A: plain.compute_observations(dof_t, est, nrm, cmd3, wb)}, reset)
        wb = plain.step(h1)
        tb = b.run_fsm(dof_t, body_t, plain.pack_commands(cmd3, wb), req)
        assert torch.equal(wa, wb) and torch.equal(ta, tb), tick
        assert np.array_equal(a.fsm_state(), b.fsm_state()), tick
        assert torch.equal(fused.h, dev.memory_a.h) and torch.equal(fused.c, dev.memory_a.c), tick


# ---- 6. from the trainer --------------------------------------------------------------------------------------------------------------------------------
def test_a_trainers_checkpoint_loads_as_the_policy_it_trained(tmp_path):
    n_envs, H = 32, 32
    cfg = P.PPOConfig(num_steps_per_env=4, num_mini_batches=2, num_learning_epochs=1, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,), init_noise_std=0.5)
    task = R.BatchedRLTask([i % 3 for i in range(n_envs)], [TROT] * n_envs, cfg=R.TaskConfig(episode_length_s=0.03, seed=5), device=DEV)
    trainer = P.PPOTrainer(task, cfg, seed=11, recurrent=RC.RecurrentConfig(hidden_size=H))
    trainer.learn(1)
    path = str(tmp_path / "model.pt")
    trainer.save(path)
    policy = WP.WeightPolicy.from_state_dict(torch.load(path)["model_state_dict"], device=DEV)
    assert type(policy) is WP.RecurrentWeightPolicy and policy.num_obs == task.num_obs and policy.hidden_size == H and policy.dims == [H, 64, 32, 12]
    g = torch.Generator().manual_seed(21)
    obs = torch.randn(3, n_envs, task.num_obs, generator=g).to(DEV)
    resets = (torch.rand(3, n_envs, generator=g) < 0.3).long().to(DEV)
    live = trainer.get_inference_policy()
    trainer.actor_critic.reset_memory()                                          # both from zero state
    for t in range(3):
        reset = resets[t] if t > 0 else None
        _, actions = policy.step(obs[t], reset=reset, return_actions=True)
        assert torch.equal(actions, live(obs[t], reset=reset)), t
    assert bool(policy.h.any()) and torch.equal(policy.h, trainer.actor_critic.memory_a.h)
    # a feed-forward trainer's checkpoint still loads as the plain class
    flat = P.PPOTrainer(task, cfg, seed=4)
    flat_path = str(tmp_path / "flat.pt")
    flat.save(flat_path)
    plain = WP.WeightPolicy.from_state_dict(torch.load(flat_path)["model_state_dict"], device=DEV)
    assert type(plain) is WP.WeightPolicy and plain.num_obs == task.num_obs
    assert torch.equal(plain.step(obs[0], return_actions=True)[1], flat.get_inference_policy()(obs[0]))
