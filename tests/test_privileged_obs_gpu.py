"""The critic's privileged observation row on the MI355X (csrc/mpc_privileged_obs.h, rl_mpc_locomotion_amd.privileged_obs): the kernel against the
numpy restatement of tests/privileged_obs_ref.py bit for bit -- on crafted contact flags and counters with guard words around the output, and in
BatchedRLTask.step after a few ticks, with feet in the air and environments reset -- and the row under observation noise: the noisy task's
privileged row is the noise-free task's observation."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, domain_rand as D, gait, height_scan as HS, privileged_obs as V, rl_task as R
from tests import privileged_obs_ref as ref
from tests.test_height_scan_gpu import DEV, GUARD, TROT, _cfg, _dev, _guarded, _robots, _yaw, grid, same

pytestmark = pytest.mark.gpu
NAN = float("nan")
SCANS = {0: None, 15: ((-0.4, -0.2, 0.0, 0.2, 0.4), (-0.2, 0.0, 0.2)), 187: (HS.POINTS_X, HS.POINTS_Y)}      # P -> the scan's points
TICKS = 5


def _scan(n, P):
    return None if SCANS[P] is None else HS.HeightScan(n, points_x=SCANS[P][0], points_y=SCANS[P][1], device=DEV)


@pytest.mark.parametrize("P, w_in", ((0, 48), (0, 64), (15, 64), (187, 240), (6, 64)))
@pytest.mark.parametrize("n", (1, 3, 64, 65, 130))
def test_kernel_equals_the_restatement_on_crafted_flags(n, P, w_in):
    """One lane per float4: 3 x 16 quads are less than a wave, 65 x 16 and 65 x 60 more than one workgroup of 256, and 130 x 60 ends in a partial one.
    P = 6 and 15 end the live columns inside a quad (54 = 13 x 4 + 2, 63 = 15 x 4 + 3), P = 0 and 187 leave 48 and 235 = 58 x 4 + 3."""
    import torch
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    rng = np.random.default_rng(100 * n + P)
    sim = BatchedToySim(_robots(n), device=DEV)
    state = sim.get_state()
    state["i32"][:, :4] = rng.integers(0, 2, (n, 4))
    state["i32"][0, :4] = (1, 0, 0, 1)
    sim.set_state(state)
    priv = V.PrivilegedObs(n, device=DEV)
    priv.bind(sim)
    obs_np = ref.sentinel_obs(n, w_in, seed=n)
    progress = rng.integers(0, 2000, n).astype(np.int64)
    progress[0] = 1999
    inv = ref.inverse_length(2000)
    want = ref.row(obs_np, state["i32"][:, :4], progress, inv, P)
    w = ref.width(P)
    obs, prog = _dev(obs_np), _dev(progress)
    out, block = _guarded(n, w, -123.0)
    runs = []
    for _ in range(2):                                                     # the whole row is rewritten, pad included, and a rerun is bit-identical
        out.fill_(NAN)
        got = priv.assemble(obs, prog, inv, num_scan=P, out=out)
        assert got.data_ptr() == out.data_ptr()
        runs.append(block.cpu().numpy())
    assert same(runs[0], runs[1])
    rows = runs[0][GUARD:-GUARD].reshape(n, w)
    assert same(rows, want)
    assert (runs[0][:GUARD] == np.float32(-123.0)).all() and (runs[0][-GUARD:] == np.float32(-123.0)).all()
    _, c0, ph, pad, _ = ref.offsets(P)
    assert same(rows[:, :c0], obs_np[:, :c0]) and (rows[:, pad:].view(np.uint32) == 0).all()      # the pad: +0.0 exactly
    assert same(rows[:, c0:ph], (state["i32"][:, :4] != 0).astype(np.float32)) and rows[0, ph] == np.float32(1999) * inv
    assert same(obs.cpu().numpy(), obs_np) and same(sim.get_state()["i32"], state["i32"])         # the inputs are untouched
    fresh = priv.assemble(obs, prog, V.inverse_length(2000), num_scan=P)   # no out
    assert fresh.shape == (n, w) and same(fresh.cpu().numpy(), want)


@pytest.mark.parametrize("P", sorted(SCANS))
@pytest.mark.parametrize("n", (3, 65))
def test_in_the_task_the_row_is_the_clean_observation_the_contacts_and_the_phase(n, P):
    """TICKS ticks after the reset, with every second environment's counter moved to three ticks before its time-out: the trot's table says FR and
    RL are half-way through their first swing (5 segments of iterations_between_mpc ticks each) where no reset intervened, so some feet are in the
    air, and the moved environments have been reset inside the window, so the counters differ."""
    import torch
    g = grid()
    cfg = _cfg(episode_length_s=0.08, seed=5)
    assert cfg.max_episode_length == 8
    origin = g.tile_origins.reshape(-1, 2)[np.arange(n) % 6] + np.random.default_rng(2).uniform(-1.2, 1.2, (n, 2))
    scan = _scan(n, P)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), terrain=g.terrain, origin=origin, height_scan=scan,
                           privileged_obs=V.PrivilegedObs(n, device=DEV))
    w = ref.width(P)
    assert task.num_privileged_obs == w == {0: 64, 15: 80, 187: 240}[P] and task.privileged_obs_buf.shape == (n, w)
    assert task.get_privileged_observations().data_ptr() == task.privileged_obs_buf.data_ptr()
    assert task.num_obs == (48 if P == 0 else scan.width(48)) and task.obs_buf.shape[1] == task.num_obs      # the actor's row is what it was
    ibm = task.bridge.ctl.iterations_between_mpc
    assert TICKS + 1 < 5 * ibm                                             # inside the first half cycle
    assert gait.mpc_table([TROT], TICKS + 1, ibm)[0, :4].tolist() == [1.0, 0.0, 0.0, 1.0]       # FL FR RL RR: FR and RL swing
    actions = _dev(np.random.default_rng(3).uniform(-1, 1, (TICKS, n, 12)).astype(np.float32))
    task.reset()
    task.progress_buf[1::2] = cfg.max_episode_length - 3
    resets = torch.zeros(n, dtype=torch.long, device=DEV)
    for k in range(TICKS):
        task.privileged_obs_buf.fill_(NAN)
        resets += task.reset_buf                                           # the flags this step's begin consumes
        task.step(actions[k])
    rows = task.privileged_obs_buf.cpu().numpy()
    state, progress = task.sim.get_state(), task.progress_buf.cpu().numpy()
    want = ref.row(task.obs_buf.cpu().numpy(), state["i32"][:, :4], progress, ref.inverse_length(cfg.max_episode_length), P)
    assert same(rows, want)
    _, c0, ph, pad, _ = ref.offsets(P)
    assert (c0, ph) == (V.contact_offset(P), V.phase_offset(P))
    assert same(rows[:, :c0], task.obs_buf.cpu().numpy()[:, :c0]) and (rows[:, pad:].view(np.uint32) == 0).all() and np.isfinite(rows).all()
    contact, _ = task.sim.flags()
    assert same(rows[:, c0:ph], contact.cpu().numpy().astype(np.float32))
    resets = resets.cpu().numpy()
    print(f"n = {n}, P = {P}: contacts {rows[:, c0:ph].mean(0)}, counters {sorted(set(progress.tolist()))}, resets {resets.tolist()[:6]}")
    assert 0 < rows[:, c0:ph].mean() < 1                                   # some feet in the air, some on the ground
    assert (resets[1::2] >= 1).all() and (progress[1::2] < TICKS).all() and len(set(progress.tolist())) >= 2
    assert len(set(rows[:, ph].tolist())) >= 2 and rows[:, ph].max() < 1


@pytest.mark.parametrize("P", (0, 187))
def test_the_row_stays_clean_under_observation_noise(P):
    """Two tasks that differ in one thing: the second has large gaussian additive observation noise (no action noise, no pushes, and the same
    actions, so the plants move alike).  After five ticks the noisy task's privileged row holds the other's observation, bit for bit."""
    n, g = 8, grid()
    cfg = _cfg(episode_length_s=0.04, seed=7)
    origin = g.tile_origins.reshape(-1, 2)[np.arange(n) % 6]
    actions = _dev(np.random.default_rng(4).uniform(-1, 1, (TICKS, n, 12)).astype(np.float32))
    tasks = []
    for noisy in (False, True):
        dr = D.DomainRand(n, observations=D.NoiseSpec("gaussian", "additive", (0.0, 0.5)), seed=3, device=DEV) if noisy else None
        task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), terrain=g.terrain, origin=origin, height_scan=_scan(n, P),
                               domain_rand=dr, privileged_obs=V.PrivilegedObs(n, device=DEV))
        task.reset()
        for k in range(TICKS):
            task.step(actions[k])
        tasks.append(task)
    clean, noisy = tasks
    live = 48 + P
    a, b = clean.obs_buf.cpu().numpy(), noisy.obs_buf.cpu().numpy()
    assert noisy.domain_rand.launches["observations"] == TICKS + 1
    assert same(noisy.privileged_obs_buf.cpu().numpy()[:, :live], a[:, :live])
    assert same(noisy.privileged_obs_buf.cpu().numpy(), clean.privileged_obs_buf.cpu().numpy())      # contacts and phase too: the same dynamics
    assert same(clean.sim.root_states.cpu().numpy(), noisy.sim.root_states.cpu().numpy())
    differ = (a[:, :live] != b[:, :live]).mean()
    print(f"P = {P}: {differ:.3f} of the noisy task's own live columns differ from the clean ones")
    assert differ > 0.5 and same(a[:, live:], b[:, live:])                 # its own observation is noisy; the scan's pad is not


def test_argument_errors_come_back_before_any_launch():
    import torch
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    n = 8
    priv = V.PrivilegedObs(n, device=DEV)
    obs = torch.zeros((n, 48), dtype=torch.float32, device=DEV)
    prog = torch.zeros(n, dtype=torch.long, device=DEV)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*no sim bound"):
        priv.assemble(obs, prog, 0.001)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*9 robots"):
        priv.bind(BatchedToySim(_robots(n + 1), device=DEV))
    priv.bind(BatchedToySim(_robots(n), device=DEV))
    for bad in (dict(obs=obs.double()), dict(obs=obs[:-1]), dict(obs=obs[:, ::2]), dict(progress_buf=prog.int()), dict(progress_buf=prog[:-1]),
                dict(out=torch.zeros((n, 48), dtype=torch.float32, device=DEV)), dict(num_scan=209)):
        with pytest.raises(ValueError):
            priv.assemble(**{**dict(obs=obs, progress_buf=prog, inv_len=0.001), **bad})
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*obs_width"):
        priv.assemble(obs, prog, 0.001, num_scan=15)                       # 48 columns cannot hold 48 + 15
    with pytest.raises(ValueError, match="environments"):
        R.BatchedRLTask(_robots(n + 1), [TROT] * (n + 1), device=DEV, privileged_obs=priv)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, device=DEV)
    assert task.privileged_obs_buf is None and task.num_privileged_obs is None and task.get_privileged_observations() is None
    assert priv.assemble(obs, prog, 0.001).shape == (n, 64)                # and the bound handle still runs
