"""The RL task's post-physics half on the MI355X (include/mpc_task.h, rl_mpc_locomotion_amd.rl_task): the two kernels against the reference's golden
(batch and 120-tick sequence, the rules of tests/test_rl_task.py) and against a torch composition of the same half on 4096+ random rows, the two
contact forms, resets without host traffic, the closed loop on the toy plant, and determinism."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import rl_task as R
from tests.test_closed_loop import _cases
from tests.test_rl_task import ROBOTS, ROT, batch_config, check_outputs, compact_ids, gold, replay_sequence, sequence_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the goldens are read-only)
    return t if dtype is None else t.to(dtype)


def _host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _indices(g):
    return dict(base_index=int(g["base_index"]), knee_indices=g["knee_indices"], hip_indices=g["hip_indices"])


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_the_batch_golden(robot):
    import torch
    g = gold(robot)
    n = len(g["b_root"])
    t = R.TaskPostPhysics(n, batch_config(), device=DEV)
    t.progress_buf.copy_(_dev(g["b_episode"]))
    t.commands.copy_(_dev(g["b_commands"]))
    obs, rew, reset = t.finish(_dev(g["b_root"]), _dev(g["b_dof"]), _dev(g["b_actions"]), _dev(g["b_torques"]), contact_forces=_dev(g["b_contact"]), **_indices(g))
    assert obs is t.obs_buf and reset.dtype == torch.long
    check_outputs(*_host(obs, rew, reset), g["b_obs"], g["b_rew"], g["b_reset"], float(g["b_gap_rot"]), float(g["b_gap_rew"]), float(g["clip"]), f"{robot} batch")


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_the_sequence_golden(robot):
    g = gold(robot)
    n = g["s_progress"].shape[1]
    cfg = sequence_config(seed=3)
    t = R.TaskPostPhysics(n, cfg, device=DEV)
    s = {k: _dev(g["s_" + k]) for k in ("root", "dof", "actions", "torques", "contact", "commands")}

    def begin():
        ids = t.begin()
        return _host(t.progress_buf, t.timeout_buf, ids, t.commands)

    def finish(k, cmd):
        t.commands.copy_(s["commands"][k])
        return _host(*t.finish(s["root"][k], s["dof"][k], s["actions"][k], s["torques"][k], contact_forces=s["contact"][k], **_indices(g)))

    replay_sequence(g, cfg, begin, finish)


def _torch_half(cfg, dt, root, dof, commands, actions, torques, cf, idx, progress, reset_buf):
    """The post-physics half as the plain torch composition (vec_task.py:326, aliengo.py:273-281 with the task-buffer part of reset_idx, :357-444,
    vec_task.py:337), in dtype dt; commands of the environments being reset are left to the caller.  Returns timeout, progress, env_ids, obs, rew, reset."""
    import torch
    f = lambda x: x.to(dt)
    root, dof, commands, actions, torques, cf = f(root), f(dof), f(commands), f(actions), f(torques), f(cf)
    rs = dict(zip(R.REWARD_TERMS, cfg.reward_scales()))
    timeout = torch.where(progress >= cfg.max_episode_length - 1, torch.ones_like(progress), torch.zeros_like(progress))
    progress = progress + 1
    env_ids = reset_buf.nonzero(as_tuple=False).squeeze(-1)
    progress[env_ids] = 0

    def qri(q, v):
        q_w, q_vec = q[:, -1], q[:, :3]
        a = v * (2.0 * q_w ** 2 - 1.0).unsqueeze(-1)
        b = torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0
        c = q_vec * (q_vec * v).sum(-1, keepdim=True) * 2.0
        return a - b + c
    quat = root[:, 3:7]
    lin, ang = qri(quat, root[:, 7:10]), qri(quat, root[:, 10:13])
    dofv = dof.view(-1, 12, 2)
    default = torch.tensor(cfg.default_dof_pos, dtype=dt, device=root.device)
    scaled = commands * torch.tensor([cfg.lin_vel_scale, cfg.lin_vel_scale, cfg.ang_vel_scale], device=root.device)
    obs = torch.cat((root[:, 0:3], lin * cfg.lin_vel_scale, ang * cfg.ang_vel_scale, scaled, (dofv[..., 0] - default) * cfg.dof_pos_scale,
                     dofv[..., 1] * cfg.dof_vel_scale, actions), dim=-1)
    obs = torch.clamp(obs, -cfg.clip_observations, cfg.clip_observations)
    lin_err = torch.sum(torch.square(commands[:, :2] - lin[:, :2]), dim=1)
    ang_err = torch.square(commands[:, 2] - ang[:, 2])
    knee = torch.norm(cf[:, idx["knee_indices"], :], dim=2) > 1.
    total = (torch.exp(-lin_err / 0.25) * rs["lin_vel_xy"] + torch.square(lin[:, 2]) * rs["lin_vel_z"] + torch.sum(torch.square(ang[:, :2]), dim=1) * rs["ang_vel_xy"]
             + torch.exp(-ang_err / 0.25) * rs["ang_vel_z"] + torch.sum(torch.square(torques), dim=1) * rs["torque"] + torch.sum(knee, dim=1) * rs["collision"])
    rew = torch.clip(total, 0., None)
    reset = torch.norm(cf[:, idx["base_index"], :], dim=1) > 1.
    reset = reset | torch.any(knee, dim=1) | torch.any(torch.norm(cf[:, idx["hip_indices"], :], dim=2) > 1., dim=1) | (progress > cfg.max_episode_length)
    return timeout, progress, env_ids, obs, rew, reset


def test_kernels_match_a_torch_composition_on_random_rows():
    import torch
    n = 4096 + 37                                  # 65 workgroups, the last one with 37 rows
    rng = np.random.default_rng(8)
    cfg = R.TaskConfig(lin_vel_scale=2.0, ang_vel_scale=0.25, dof_vel_scale=0.05, rew_collision=-0.25, episode_length_s=3.0, seed=5)
    L = cfg.max_episode_length
    bodies, idx = 9, dict(base_index=4, knee_indices=[0, 2, 6, 8], hip_indices=[1, 3, 5, 7])
    q = rng.standard_normal((n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    commands = rng.uniform(-1, 1, (n, 3)) * [0.6, 0.4, 0.6]
    root = np.concatenate([rng.uniform(-7, 7, (n, 3)), q, rng.normal(0, 0.3, (n, 6))], 1).astype(np.float32)
    dof = rng.normal(0, 2.0, (n * 12, 2)).astype(np.float32)
    dof[:: 7, 1] *= 80.0
    nrm = np.where(rng.random((n, bodies)) < 0.04, rng.uniform(2, 30, (n, bodies)), rng.uniform(0, 0.5, (n, bodies)))
    d = rng.standard_normal((n, bodies, 3)); d /= np.linalg.norm(d, axis=2, keepdims=True)
    cf = (d * nrm[..., None]).astype(np.float32)
    progress = rng.choice([0, 1, L - 3, L - 2, L - 1, L, L + 1, 57], n)         # both sides of `>= L - 1` (before the increment) and of `> L` (after it)
    reset_in = (rng.random(n) < 0.3).astype(np.int64)
    root, dof, commands, cf = _dev(root), _dev(dof), _dev(commands.astype(np.float32)), _dev(cf)
    actions, torques = _dev(rng.uniform(-1, 1, (n, 12)).astype(np.float32)), _dev(rng.normal(0, 10, (n, 12)).astype(np.float32))
    t = R.TaskPostPhysics(n, cfg, device=DEV)
    t.progress_buf.copy_(_dev(progress)); t.reset_buf.copy_(_dev(reset_in)); t.commands.copy_(commands)
    ids = t.begin()
    hit = ids >= 0
    ref = {}
    for dt in (torch.float32, torch.float64):
        ref[dt] = _torch_half(cfg, dt, root, dof, t.commands, actions, torques, cf, idx, _dev(progress), _dev(reset_in))
    timeout, prog, env_ids, obs32, rew32, reset32 = ref[torch.float32]
    _, _, _, obs64, rew64, reset64 = ref[torch.float64]
    assert torch.equal(t.timeout_buf, timeout) and torch.equal(t.progress_buf, prog) and torch.equal(ids[hit].long(), env_ids)
    assert torch.equal(torch.arange(n, device=DEV)[hit].int(), ids[hit]) and (t.reset_buf[hit] == 1).all().item()
    assert torch.equal(t.commands[~hit], commands[~hit]) and not torch.equal(t.commands[hit], commands[hit])
    assert 0.2 * n < int(hit.sum()) < 0.4 * n and int(timeout.sum()) > 0.2 * n
    obs, rew, reset = t.finish(root, dof, actions, torques, contact_forces=cf, **idx)
    assert torch.equal(reset32, reset64) and 0.1 * n < int(reset32.sum()) < 0.9 * n and (obs32.abs() == 5.0).any(1).float().mean().item() > 0.1
    gap_rot = float((obs32[:, ROT] - obs64[:, ROT]).abs().max())
    gap_rew = float((rew32 - rew64).abs().max())
    assert (rew32 > 0).float().mean().item() > 0.1           # (velocities are unrelated to the commands here: many rewards clip to 0, the golden covers the rest)
    check_outputs(*_host(obs, rew, reset), *_host(obs32, rew32, reset32), gap_rot, gap_rew, cfg.clip_observations, "torch composition")


def test_contact_forms_agree():
    import torch
    g = gold("go1")
    n = len(g["b_root"])
    idx = _indices(g)
    nrm = np.linalg.norm(g["b_contact"].astype(np.float64), axis=2)
    fell = nrm[:, idx["base_index"]] > 1
    only_base = np.zeros_like(g["b_contact"])
    only_base[:, idx["base_index"]] = g["b_contact"][:, idx["base_index"]]
    t = R.TaskPostPhysics(n, batch_config(), device=DEV)
    t.progress_buf.copy_(_dev(g["b_episode"])); t.commands.copy_(_dev(g["b_commands"]))
    args = [_dev(g[k]) for k in ("b_root", "b_dof", "b_actions", "b_torques")]
    outs = []
    for kw in (dict(contact_forces=_dev(only_base), **idx), dict(fell=_dev(fell)), dict(fell=_dev(fell.astype(np.uint8))),
               dict(contact_forces=_dev(only_base), fell=_dev(fell), **idx), dict()):
        outs.append(_host(*t.finish(*args, **kw)))
    for o in outs[1:4]:
        assert all(np.array_equal(x, y) for x, y in zip(outs[0], o))
    assert fell.sum() >= 8 and (outs[0][2][fell] == 1).all()
    assert np.array_equal(outs[4][2].astype(bool), g["b_episode"] > g["b_max_len"])
    with pytest.raises(ValueError):
        t.finish(*args, contact_forces=_dev(only_base))          # contact forces without the body indices
    with pytest.raises(R._lib.MpcLibraryError):
        t.finish(*args, contact_forces=_dev(only_base), base_index=99, knee_indices=idx["knee_indices"], hip_indices=idx["hip_indices"])


def _task(n, cfg, robots=None, **kw):
    rt = [i % 3 for i in range(n)] if robots is None else robots
    return R.BatchedRLTask(rt, [TROT] * n, cfg=cfg, device=DEV, **kw)


def test_pending_resets_touch_nothing_else_and_nothing_reaches_the_host():
    import torch
    n, flagged = 192, [3, 64, 65, 130, 191]
    others = [i for i in range(n) if i not in flagged]
    cfg = R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), seed=21)
    rng = np.random.default_rng(4)
    actions = _dev(rng.uniform(-1.2, 1.2, (50, n, 12)).astype(np.float32))
    mask = torch.zeros(n, dtype=torch.long, device=DEV)
    mask[flagged] = 1
    runs = []
    for with_flags in (False, True):
        task = _task(n, cfg)
        ptrs = [x.data_ptr() for x in (task.obs_buf, task.rew_buf, task.reset_buf, task.progress_buf, task.commands, task.sim.dof_state, task.sim.root_states)]
        tau = torch.zeros((50, n, 12), dtype=torch.float32, device=DEV)
        obs = torch.zeros((50, n, 48), dtype=torch.float32, device=DEV)
        task.reset()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")      # a torch call that waits for the device or copies to the host raises from here on
        try:
            with pytest.raises(RuntimeError):        # (the reference's own first statement does)
                task.reset_buf.nonzero()
            for k in range(50):
                if with_flags and k in (20, 21, 35):
                    task.reset_buf.bitwise_or_(mask)                             # resets pending for the next step
                o, r, d, extras = task.step(actions[k])
                tau[k].copy_(task.torques); obs[k].copy_(o)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert ptrs == [x.data_ptr() for x in (o, r, d, task.progress_buf, task.commands, task.sim.dof_state, task.sim.root_states)]
        assert extras["time_outs"] is task.timeout_buf
        st = task.sim.get_state()
        runs.append((tau.cpu().numpy(), obs.cpu().numpy(), st["f64"], st["i32"], task.bridge.ctl.solver_record(), task.progress_buf.cpu().numpy(), task.commands.cpu().numpy()))
    a, b = runs
    for x, y in zip(a, b):
        assert np.array_equal(x[..., others, :] if x.ndim == 3 else x[others], y[..., others, :] if y.ndim == 3 else y[others])
    assert (a[5] == 50).all() and (b[5][flagged] == 14).all() and (b[5][others] == 50).all()      # progress: reset on tick 35, 14 increments since
    assert not np.array_equal(a[6][flagged], b[6][flagged])                                          # fresh commands
    assert not np.array_equal(a[2][flagged], b[2][flagged])                                          # and the flagged robots were put back standing


def test_closed_loop_of_golden_trot_robots():
    import torch
    n, ticks = 4096, 1000
    g, names = _cases()
    trot = [nm for nm in names if nm.endswith("_trot_flat")]
    assert len(trot) == 3
    meta = [g[nm + "/meta"] for nm in trot]
    which = np.arange(n) % 3
    cmd16 = np.stack([g[trot[w] + "/cmd"] for w in which]).astype(np.float32)
    assert (cmd16[:, 3:15] == np.array([5, 5, 5, 50, 50, 50, 1, 1, 1, 1, 1, 1], np.float32)).all()      # the golden's weights are the bridge's at zero actions
    cmd = _dev(cmd16[:, :3])
    cfg = R.TaskConfig(episode_length_s=2.0, command_x_range=(-0.3, 0.5), command_y_range=(0.0, 0.1), command_yaw_range=(-0.2, 0.3), seed=2)
    L = cfg.max_episode_length
    assert L == 200
    task = _task(n, cfg, robots=[int(meta[w][0]) for w in which], yaw0=np.array([meta[w][5] for w in which]), flat_ground=True)
    zero = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
    n_reset = torch.zeros(ticks, dtype=torch.long, device=DEV)
    n_timeout = torch.zeros(ticks, dtype=torch.long, device=DEV)
    max_progress = torch.zeros(ticks, dtype=torch.long, device=DEV)
    positive = torch.zeros((), dtype=torch.long, device=DEV)
    bad_obs = torch.zeros((), dtype=torch.long, device=DEV)
    fell_any = torch.zeros((), dtype=torch.long, device=DEV)
    for k in range(ticks):
        obs, rew, reset, extras = task.step(zero)
        task.commands.copy_(cmd)                     # the golden's commands, whatever a reset drew (a caller may overwrite `commands`)
        n_reset[k] = (task.task.reset_ids >= 0).sum()
        n_timeout[k] = extras["time_outs"].sum()
        max_progress[k] = task.progress_buf.max()
        positive += (rew > 0).sum()
        bad_obs += (~torch.isfinite(obs) | (obs.abs() > cfg.clip_observations)).sum()
        fell_any += task.sim.flags()[1].sum()
    n_reset, n_timeout, max_progress = _host(n_reset, n_timeout, max_progress)
    # progress runs 0 .. L + 1; the flag of tick k resets on tick k + 1: every L + 2 ticks, all environments together
    reset_ticks = np.flatnonzero(n_reset)
    assert np.array_equal(reset_ticks, np.arange(0, ticks, L + 2)) and (n_reset[reset_ticks] == n).all()
    assert set(np.unique(n_timeout)) == {0, n} and np.array_equal(np.flatnonzero(n_timeout)[:3], [L, L + 1, L + 2])       # vec_task.py:326
    assert max_progress.max() == L + 1
    assert fell_any.item() == 0, "a robot fell"
    assert bad_obs.item() == 0
    share = positive.item() / (n * ticks)
    print(f"reward positive on {share:.3f} of the robot-ticks")
    assert share > 0.5


def test_determinism_and_seed():
    import torch
    n = 256
    outs = []
    for seed in (7, 7, 8):
        task = _task(n, R.TaskConfig(episode_length_s=1.0, seed=seed))
        rng = np.random.default_rng(1)
        actions = _dev(rng.uniform(-1, 1, (n, 12)).astype(np.float32))
        task.reset()
        first = task.commands.clone()
        for k in range(300):
            obs, rew, reset, _ = task.step(actions)
        st = task.sim.get_state()
        outs.append(_host(first, obs, rew, reset, task.commands, task.progress_buf) + (st["f64"], st["i32"]))
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x, y, equal_nan=True)
    assert not np.array_equal(outs[0][0], outs[2][0]) and not np.array_equal(outs[0][4], outs[2][4])
    assert not np.array_equal(outs[0][0], outs[0][4])            # the commands of a later episode differ from the first one's
