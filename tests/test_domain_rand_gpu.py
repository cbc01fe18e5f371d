"""The domain randomisation on the MI355X (csrc/mpc_domain_rand.h, rl_mpc_locomotion_amd.domain_rand): the noise kernel against the restatement of
tests/domain_rand_ref.py on the crafted batch (uniform draws and outputs EQUAL, pads and guards untouched, NaN kept, the device's normal draws
within 4 x the host build's recorded gap to float64), the moments of the device's draws, the push kernel on the plant's state, and the three hooks
in BatchedRLTask.step and in PPOTrainer.learn.

Figures of one run (printed with -s): the device's worst normal gap is 1.28e-06 on the crafted batch and 1.59e-06 on the moment batch; the host
build's is 1.60e-06 (HOST_NORMAL_GAP 1.61e-06, so the bound here is 6.44e-06)."""
import functools
import math

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import domain_rand as DR, height_scan as HS, rl_task as R, terrain as TR
from tests import domain_rand_ref as ref
from tests.domain_rand_ref import MOMENT_SEEDS, MOMENT_SHAPE, SEED, check_against_restatement, check_moments, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
GUARD = 64
F = np.float32
GAP_BOUND = 4 * ref.HOST_NORMAL_GAP     # the device's logf / cosf / sinf are other implementations than glibc's: this project's factor for float32 restatements


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _robots(n):
    return [i % 3 for i in range(n)]


def _guarded(n, w, fill):
    """A [n, w] float32 view with GUARD sentinel words on either side of it, and the whole block."""
    import torch
    block = torch.full((n * w + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    return block[GUARD:GUARD + n * w].view(n, w), block


def _params(dist, rng, corr):
    names = ("mu", "var", "mu_corr", "var_corr") if dist == "gaussian" else ("lo", "hi", "lo_corr", "hi_corr")
    return dict(zip(names, (rng[0], rng[1], corr[0], corr[1])))


def _noise(dr, target, x_np, active, tick, params, in_place=False):
    """(out, d, zc) of one launch, the guards checked."""
    import torch
    n, W = x_np.shape
    x, x_block = _guarded(n, W, -123.0)
    x.copy_(_dev(x_np))
    out, out_block = (x, x_block) if in_place else _guarded(n, W, -321.0)
    draws, d_block = _guarded(n, 2 * active, -55.0)
    got = dr.noise(target, x, out=None if in_place else out, active=active, clip=ref.CLIP, tick=tick, params=params, draws=draws.view(n, active, 2))
    assert got.data_ptr() == out.data_ptr()
    for block, fill in ((x_block, -123.0), (out_block, -123.0 if in_place else -321.0), (d_block, -55.0)):
        b = block.cpu().numpy()
        assert (b[:GUARD] == F(fill)).all() and (b[-GUARD:] == F(fill)).all()
    if not in_place:
        assert same(x.cpu().numpy(), x_np)
    dz = draws.view(n, active, 2).cpu().numpy()
    return out.cpu().numpy(), np.ascontiguousarray(dz[:, :, 0]), np.ascontiguousarray(dz[:, :, 1])


@pytest.mark.parametrize("W,active", ref.SHAPES)
def test_noise_kernel_equals_the_restatement_on_the_crafted_batch(W, active):
    x = ref.crafted(ref.N, W)
    worst, k = 0.0, 0
    for dist, op, rng, corr in ref.CASES:
        for col_scale in (None, ref.column_scale(W)):
            spec = DR.NoiseSpec(dist, op, rng, corr, column_scale=col_scale)
            dr = DR.DomainRand(ref.N, observations=spec, actions=spec, seed=SEED, device=DEV)
            target, tick = ("observations", "actions")[k % 2], (0, 3)[(k // 2) % 2]
            k += 1
            out, d, zc = _noise(dr, target, x, active, tick, _params(dist, rng, corr))
            worst = max(worst, check_against_restatement(x, out, d, zc, int(corr != (0.0, 0.0)), target, SEED, dist, op, rng, corr, active, tick, col_scale,
                                                         GAP_BOUND))
            out2, d2, zc2 = _noise(dr, target, x, active, tick, _params(dist, rng, corr), in_place=True)
            assert same(out2, out) and same(d2, d) and same(zc2, zc)                # in place == out of place, and a rerun is bit-identical
            assert dr.launches[target] == 2
    print(f"device normal gap on [{ref.N}, {W}] (active {active}): {worst:.3e}; host build {ref.HOST_NORMAL_GAP:.2e}, bound {GAP_BOUND:.2e}")


def test_noise_kernel_beyond_one_pass_of_its_grid():
    """4500 x 120 column pairs are more than 2048 workgroups of 256 lanes: the grid-stride loop's second pass, and a last pass that is not full."""
    n, W, active = 4500, 240, 235
    assert n * W // 2 > 2048 * 256 and (n * W // 2) % (2048 * 256) != 0
    x = np.random.default_rng(8).standard_normal((n, W)).astype(F)
    dist, op, rng, corr = ref.CASES[5]                                               # uniform, additive, with the kept term
    cs = ref.column_scale(W)
    dr = DR.DomainRand(n, observations=DR.NoiseSpec(dist, op, rng, corr, column_scale=cs), seed=SEED, device=DEV)
    out, d, zc = _noise(dr, "observations", x, active, 9, _params(dist, rng, corr))
    assert same(d, ref.uniform_draws("observations", SEED, n, active, 9))
    assert float(np.abs(zc.astype(np.float64) - ref.normal_draws64("observations", SEED, n, active, 9, corr=True)).max()) <= GAP_BOUND
    assert same(out[:, :active], ref.apply(x[:, :active], d, zc, *ref.kernel_params(dist, rng, corr), ref.CLIP, False, cs)) and same(out[:, active:], x[:, active:])
    small = DR.DomainRand(ref.N, observations=DR.NoiseSpec(dist, op, rng, corr), seed=SEED, device=DEV)
    _, d67, zc67 = _noise(small, "observations", x[:ref.N, :48].copy(), 48, 9, _params(dist, rng, corr))
    assert same(d67, d[:ref.N, :48]) and same(zc67, zc[:ref.N, :48])                 # a draw is the same in a batch of 67 and of 4500, 48 and 240 wide


@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_moments_of_the_devices_draws(dist):
    import torch
    n, W, ticks = MOMENT_SHAPE
    seed = MOMENT_SEEDS[dist]
    rng = (0.0, 1.0)
    dr = DR.DomainRand(n, observations=DR.NoiseSpec(dist, "additive", rng), seed=seed, device=DEV)
    x = torch.zeros((n, W), dtype=torch.float32, device=DEV)
    out = torch.empty_like(x)
    draws = torch.empty((ticks, n, W, 2), dtype=torch.float32, device=DEV)
    for t in range(ticks):
        dr.noise("observations", x, out=out, clip=math.inf, tick=t, params=_params(dist, rng, (0.0, 0.0)), draws=draws[t])
    d = draws[..., 0].cpu().numpy()
    check_moments(d, dist)
    assert same(out.cpu().numpy(), d[-1])                                            # 0 + d * 1 + 0, unclipped
    if dist == "gaussian":
        gap = max(float(np.abs(d[t].astype(np.float64) - ref.normal_draws64("observations", seed, n, W, t)).max()) for t in range(ticks))
        print(f"device normal gap on the moment batch: {gap:.3e}; host build {ref.HOST_NORMAL_GAP:.2e}, bound {GAP_BOUND:.2e}")
        assert gap <= GAP_BOUND
    else:
        assert all(same(d[t], ref.uniform_draws("observations", seed, n, W, t)) for t in range(ticks))


def test_push_writes_two_words_of_the_standing_robots_and_nothing_else():
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    n, v, k = 130, 0.8, 3
    fallen = [0, 5, 63, 64, 65, 100, 129]
    sim = BatchedToySim(_robots(n), device=DEV, yaw0=np.linspace(-3, 3, n))
    st = sim.get_state()
    st["f64"][:, 7:13] = np.random.default_rng(4).uniform(-0.3, 0.3, (n, 6))
    st["i32"][fallen, 8] = 1
    sim.set_state(st)
    dr = DR.DomainRand(n, push=DR.PushSpec(interval_s=1.0, max_vel_xy=v), seed=SEED, device=DEV)
    with pytest.raises(rl_mpc_locomotion_amd._lib.MpcLibraryError, match="no sim bound"):
        dr.push_robots(sim.root_states, k)
    dr.bind(sim, dt=0.01)
    assert dr.push_interval == 100
    before, root_before = sim.get_state(), sim.root_states.cpu().numpy()
    dof_before = sim.dof_state.cpu().numpy()
    dr.push_robots(sim.root_states, k)
    after, root_after = sim.get_state(), sim.root_states.cpu().numpy()
    want = ref.push_value(SEED, np.arange(n, dtype=np.uint64)[:, None], k, np.arange(2, dtype=np.uint64)[None, :], v)
    standing = np.setdiff1d(np.arange(n), fallen)
    assert same(after["f64"][standing, 7:9], want[standing].astype(np.float64))      # the double of the float32 draw
    assert same(root_after[standing, 7:9], want[standing])
    assert (np.abs(want) <= F(v)).all() and len(np.unique(want[standing])) > 200
    keep = np.ones(49, bool); keep[7:9] = False
    assert same(after["f64"][:, keep], before["f64"][:, keep]) and same(after["i32"], before["i32"])
    assert same(after["f64"][fallen], before["f64"][fallen]) and same(root_after[fallen], root_before[fallen])
    rk = np.ones(13, bool); rk[7:9] = False
    assert same(root_after[:, rk], root_before[:, rk]) and same(sim.dof_state.cpu().numpy(), dof_before)
    assert not same(after["f64"][standing, 7:9], before["f64"][standing, 7:9]) and dr.launches["push"] == 1
    other = DR.DomainRand(67, push=DR.PushSpec(), device=DEV)
    with pytest.raises(rl_mpc_locomotion_amd._lib.MpcLibraryError, match="130 robots"):
        other.bind(sim)


# ---- the task --------------------------------------------------------------------------------------------------------------------------------
N_TASK, TICKS, ACTIVE, WIDE = 195, 60, 235, 240
PUSH_EVERY = 10


@functools.lru_cache(maxsize=None)
def _terrain():
    return TR.Terrain.mild(seed=3, rows=128, cols=128)


def _cfg():
    return R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), episode_length_s=0.17, seed=5)


def _run(make_dr=None, disabled=False):
    """60 ticks of 195 environments on the 128 x 128 mild field with the height scan, under the sync debug mode after the warm-up: per tick the
    observations, rewards, reset flags, root states, the reset flags the tick consumed, the fallen flags and the push launches so far; the plant's
    final state."""
    import torch
    n = N_TASK
    scan = HS.HeightScan(n, device=DEV)
    dr = make_dr(scan) if make_dr is not None else None
    if disabled:
        dr.enabled = False
    origin = np.random.default_rng(2).uniform(0.0, 3.0, (n, 2))
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=_cfg(), device=DEV, yaw0=np.random.default_rng(6).uniform(-np.pi, np.pi, n), terrain=_terrain(),
                           origin=origin, height_scan=scan, domain_rand=dr)
    assert task.num_obs == WIDE and task.domain_rand is dr
    actions = _dev(np.random.default_rng(3).uniform(-1.2, 1.2, (TICKS, n, 12)).astype(F))
    rec = [torch.zeros((TICKS, n, k), dtype=torch.float32, device=DEV) for k in (WIDE, 1, 1, 13, 1, 1, 12)]
    pushes = []
    task.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # a torch call that waits for the device or copies to the host raises from here on
    try:
        for k in range(TICKS):
            rec[4][k, :, 0].copy_(task.reset_buf)
            o, r, d, _ = task.step(actions[k])
            rec[0][k].copy_(o); rec[1][k, :, 0].copy_(r); rec[2][k, :, 0].copy_(d); rec[3][k].copy_(task.sim.root_states)
            rec[5][k, :, 0].copy_(task.sim.flags()[1]); rec[6][k].copy_(task.actions)
            pushes.append(dr.launches["push"] if dr is not None else 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    names = ("obs", "rew", "reset", "root", "consumed", "fell", "actions")
    res = {nm: x.cpu().numpy() for nm, x in zip(names, rec)}
    res.update(state=task.sim.get_state(), pushes=pushes, dr=dr, clip_actions=task.cfg.clip_actions, raw_actions=actions.cpu().numpy())
    return res


@functools.lru_cache(maxsize=None)
def _twin():
    return _run()


def _equal_runs(a, b):
    return (all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("obs", "rew", "reset", "root", "actions"))
            and np.array_equal(a["state"]["f64"], b["state"]["f64"], equal_nan=True) and np.array_equal(a["state"]["i32"], b["state"]["i32"]))


def test_task_with_zero_noise_and_with_the_option_switched_off_is_the_twin():
    twin = _twin()
    assert twin["consumed"].sum(0).min() >= 2                                         # every environment was reset inside the window
    zero = DR.NoiseSpec("gaussian", "additive", (0.0, 0.0))
    got = _run(lambda scan: DR.DomainRand(N_TASK, observations=zero, actions=zero, seed=SEED, device=DEV))
    assert _equal_runs(got, twin)                                                      # (a): np.array_equal as torch.equal: -0 == +0
    assert got["dr"].launches == {"observations": TICKS + 1, "actions": TICKS + 1, "push": 0} and got["dr"].common_step_counter == TICKS + 1
    full = dict(observations=None, actions=DR.NoiseSpec("gaussian", "additive", (0.0, 0.3)), push=DR.PushSpec(interval_s=0.1, max_vel_xy=0.7))
    off = _run(lambda scan: DR.DomainRand(N_TASK, seed=SEED, device=DEV, **dict(full, observations=DR.NoiseSpec.legged_gym(_cfg(), height_scan=scan))),
               disabled=True)
    assert _equal_runs(off, twin)                                                      # (d)
    assert off["dr"].launches == {"observations": 0, "actions": 0, "push": 0} and off["dr"].common_step_counter == 0


def test_task_observation_noise_is_the_restated_term_on_the_twins_observations():
    twin = _twin()
    got = _run(lambda scan: DR.DomainRand(N_TASK, observations=DR.NoiseSpec.legged_gym(_cfg(), height_scan=scan), seed=SEED, device=DEV))
    spec = got["dr"].specs["observations"]
    cs = np.asarray(spec.column_scale, F)
    assert cs.shape == (WIDE,) and (cs[ACTIVE:] == 0).all() and (cs[48:ACTIVE] == F(0.5)).all()
    for name in ("rew", "reset", "root", "actions"):                                  # the noise touches nothing but obs_buf
        assert np.array_equal(got[name], twin[name], equal_nan=True), name
    differ = 0
    for k in range(TICKS):
        tick = k + 1                                                                   # reset() was tick 0
        d = ref.uniform_draws("observations", SEED, N_TASK, ACTIVE, tick)
        clean = twin["obs"][k, :, :ACTIVE]
        want = ref.apply(clean, d, np.zeros_like(d), -1.0, 2.0, 0.0, 0.0, 5.0, False, cs)
        assert same(got["obs"][k, :, :ACTIVE], want), k                               # clamp(x + term), so obs - twin is the term wherever neither is at the clip
        inside = (np.abs(want) < 5) & (np.abs(clean) < 5)
        term = ((F(0.0) + d * F(2.0)) + F(-1.0)) * cs[None, :ACTIVE]
        assert same((clean + term)[inside], got["obs"][k, :, :ACTIVE][inside]) and inside.mean() > 0.9
        assert (got["obs"][k, :, ACTIVE:] == 0).all()                                  # the pad
        differ += int((got["obs"][k, :, :ACTIVE] != clean).sum())
    assert differ > 0.6 * TICKS * N_TASK * (6 + 24 + 187)                              # the columns with a scale moved, the rest did not
    assert np.array_equal(got["obs"][:, :, 0:3], twin["obs"][:, :, 0:3]) and np.array_equal(got["obs"][:, :, 36:48], twin["obs"][:, :, 36:48])


def test_task_pushes_on_push_ticks_only():
    v = 0.7
    got = _run(lambda scan: DR.DomainRand(N_TASK, push=DR.PushSpec(interval_s=PUSH_EVERY * 0.01, max_vel_xy=v), seed=SEED, device=DEV))
    assert got["dr"].push_interval == PUSH_EVERY
    env, axis = np.arange(N_TASK, dtype=np.uint64)[:, None], np.arange(2, dtype=np.uint64)[None, :]
    launches, checked = 0, 0
    for k in range(TICKS):
        counter = k + 2                                                                # reset() was the first step
        if counter % PUSH_EVERY == 0:
            launches += 1
            want = ref.push_value(SEED, env, counter // PUSH_EVERY, axis, v)
            rows = (got["consumed"][k, :, 0] == 0) & (got["fell"][k, :, 0] == 0)       # neither reset nor fallen in this tick
            assert same(got["root"][k][rows, 7:9], want[rows]), k
            checked += int(rows.sum())
        assert got["pushes"][k] == launches, k                                         # on other ticks no push kernel is launched
    assert launches == 6 and checked > 3 * N_TASK and got["dr"].launches == {"observations": 0, "actions": 0, "push": 6}
    assert not _equal_runs(got, _twin())


def test_task_runs_repeat_with_the_seed_and_differ_with_another():
    def make(seed):
        return lambda scan: DR.DomainRand(N_TASK, observations=DR.NoiseSpec.legged_gym(_cfg(), height_scan=scan),
                                          actions=DR.NoiseSpec("gaussian", "additive", (0.0, 0.3), (0.0, 0.1)),
                                          push=DR.PushSpec(interval_s=PUSH_EVERY * 0.01, max_vel_xy=0.7), seed=seed, device=DEV)
    a, b, c = _run(make(11)), _run(make(11)), _run(make(12))
    assert _equal_runs(a, b) and same(a["obs"], b["obs"]) and same(a["root"], b["root"])
    assert not np.array_equal(a["obs"], c["obs"]) and not np.array_equal(a["actions"], c["actions"]) and not np.array_equal(a["root"], c["root"])
    # the controller and the observation saw the noisy actions: clamp(a + zc * 0.1 + d * 0.3) with the kernel's keys, within the device's normal gap
    k, tick = 7, 8
    d, zc = ref.normal_draws64("actions", 11, N_TASK, 12, tick), ref.normal_draws64("actions", 11, N_TASK, 12, tick, corr=True)
    want = np.clip(a["raw_actions"][k] + (zc * 0.1 + d * 0.3), -a["clip_actions"], a["clip_actions"])
    assert np.abs(a["actions"][k] - want).max() <= 0.4 * GAP_BOUND + 3 * 2.0 ** -24 * 2
    assert np.abs(a["actions"]).max() <= a["clip_actions"] and (np.abs(a["actions"]) == a["clip_actions"]).any()
    assert np.array_equal(a["obs"][k, :, 36:48], a["actions"][k])                              # (legged_gym's vector puts no noise on these columns)
    assert a["dr"].launches == {"observations": TICKS + 1, "actions": TICKS + 1, "push": 6}


@pytest.mark.parametrize("update", ["torch", "hip"])
def test_trainer_learns_under_noise_and_pushes(update):
    import torch
    from rl_mpc_locomotion_amd import ppo as P
    n = 64
    cfg = R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), episode_length_s=0.05, seed=4)
    scan = HS.HeightScan(n, device=DEV)
    dr = DR.DomainRand(n, observations=DR.NoiseSpec.legged_gym(cfg, height_scan=scan), actions=DR.NoiseSpec("gaussian", "additive", (0.0, 0.05)),
                       push=DR.PushSpec(interval_s=0.04, max_vel_xy=0.5), seed=9, device=DEV)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, terrain=_terrain(), origin=np.random.default_rng(2).uniform(0.0, 3.0, (n, 2)),
                           height_scan=scan, domain_rand=dr)
    pcfg = P.PPOConfig(num_steps_per_env=8, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    trainer = P.PPOTrainer(task, pcfg, seed=3, update=update)
    before = [p.detach().clone() for p in trainer.actor_critic.parameters()]
    infos = trainer.learn(1)
    assert len(infos) == 1 and all(np.isfinite(v) for k, v in infos[0].items() if k != "terrain_level_by_type")
    assert any(not torch.equal(a, b) for a, b in zip(before, trainer.actor_critic.parameters()))
    assert torch.isfinite(task.obs_buf).all().item() and torch.isfinite(trainer.storage.observations).all().item()
    assert (task.obs_buf[:, ACTIVE:] == 0).all().item()
    assert dr.launches["observations"] == dr.launches["actions"] == dr.common_step_counter >= 9 and dr.launches["push"] == dr.common_step_counter // 4
