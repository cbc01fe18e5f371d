"""The terrain height scan on the MI355X (csrc/mpc_height_scan.h, rl_mpc_locomotion_amd.height_scan): the kernel against the restatement of
tests/height_scan_ref.py on the crafted batch (wide rows and heights EQUAL, guards untouched, pads rewritten, reruns identical), against the plant's
own terrain query on a monotone field, and the hook in BatchedRLTask.step, with a curriculum, and in PPOTrainer.learn."""
import functools

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, curriculum as K, height_scan as HS, rl_task as R, terrain as TR
from tests import height_scan_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
SIZES = (1, 63, 64, 65, 130)           # one wave, a workgroup less one wave, sixteen full workgroups, one wave into the next, a partial last one
GUARD = 64
LEVELS, TYPES, TILE = 3, 2, 4.0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _robots(n):
    return [i % 3 for i in range(n)]


def _field_of(t):
    return dict(heights=t.heights, hscale=t.hscale, vscale=t.vscale, x0=t.x0, y0=t.y0)


def _sim(n, terrain, origin):
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    return BatchedToySim(_robots(n), device=DEV, terrain=terrain, origin=origin)


def _guarded(n, w, fill):
    """A [n, w] float32 view with GUARD sentinel words on either side of it, and the whole block."""
    import torch
    block = torch.full((n * w + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    return block[GUARD:GUARD + n * w].view(n, w), block


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _crafted_terrain():
    f = ref.crafted_field()
    return TR.Terrain(f["heights"], f["hscale"], f["vscale"], f["x0"], f["y0"]), f


@pytest.mark.parametrize("grid", list(ref.GRIDS))
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_restatement_on_the_crafted_batch(n, grid):
    import torch
    x, y = ref.GRIDS[grid]
    points = ref.height_points(x, y)
    terrain, field = _crafted_terrain()
    case, obs_np = ref.crafted(n, points), ref.sentinel_obs(n)
    want = ref.scan(field, case["root"], case["origin"], points, obs_np)
    scan = HS.HeightScan(n, points_x=x, points_y=y, device=DEV)
    assert scan.num_points == len(points) and same(scan.points, points)
    w = scan.width(48)
    assert w == want["wide"].shape[1] == {"17x11": 240, "4x4": 64, "1x1": 64, "16x13": 256}[grid]
    sim = _sim(n, terrain, case["origin"])
    scan.bind(sim)
    root, obs_in = _dev(case["root"]), _dev(obs_np)
    out, out_block = _guarded(n, w, -123.0)
    heights, h_block = _guarded(n, scan.num_points, -321.0)
    runs = []
    for k in range(2):                                                     # twice in a row: the pad is rewritten, the rerun bit-identical
        out[:, 48 + scan.num_points:] = 77.0
        got = scan.measure(root, obs_in, out=out, heights=heights)
        assert got.data_ptr() == out.data_ptr()
        runs.append((out_block.cpu().numpy(), h_block.cpu().numpy()))
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1])
    wide, hs = runs[0][0][GUARD:-GUARD].reshape(n, w), runs[0][1][GUARD:-GUARD].reshape(n, -1)
    assert same(wide, want["wide"]) and same(hs, want["heights"])
    assert same(wide[:, :48], obs_np) and (wide[:, 48 + scan.num_points:] == 0).all()
    for block, fill in ((runs[0][0], -123.0), (runs[0][1], -321.0)):
        assert (block[:GUARD] == np.float32(fill)).all() and (block[-GUARD:] == np.float32(fill)).all()
    assert same(obs_in.cpu().numpy(), obs_np) and same(root.cpu().numpy(), case["root"])
    fresh = scan.measure(root, obs_in)                                     # no out, no heights
    assert fresh.shape == (n, w) and same(fresh.cpu().numpy(), want["wide"])


def test_other_scalars_and_input_widths():
    import torch
    n = 65
    x, y = ref.GRIDS["4x4"]
    points = ref.height_points(x, y)
    terrain, field = _crafted_terrain()
    case = ref.crafted(n, points)
    sim = _sim(n, terrain, case["origin"])
    for in_width, kw in ((0, {}), (7, dict(offset=0.31, clip=0.4, scale=2.5, obs_clip=0.9)), (80, dict(offset=-0.2, clip=2.0, scale=5.0, obs_clip=5.0))):
        scan = HS.HeightScan(n, points_x=x, points_y=y, device=DEV, **kw)
        scan.bind(sim)
        obs_np = ref.sentinel_obs(n, in_width)
        want = ref.scan(field, case["root"], case["origin"], points, obs_np, **kw)
        got = scan.measure(_dev(case["root"]), _dev(obs_np) if in_width else torch.zeros((n, 0), dtype=torch.float32, device=DEV))
        assert same(got.cpu().numpy(), want["wide"]), in_width


def test_on_nodes_of_a_monotone_field_the_scan_is_the_plants_own_query():
    """Where the heights do not decrease along either index the lowest of a cell's three nodes is H[i][j]; at a sample point exactly on node (i, j) the
    plant's triangle interpolation (mpc_terrain_query: other code, float64) gives vscale * H[i][j] too.  With vscale a power of two both products
    are exact, so the two agree to the bit."""
    import torch
    n, hscale, vscale, x0, y0 = 65, 0.25, 2.0 ** -7, -1.0, -0.75
    rng = np.random.default_rng(3)
    H = (np.cumsum(rng.integers(0, 9, 24))[:, None] + np.cumsum(rng.integers(0, 7, 20))[None, :] - 40).astype(np.int16)
    assert (np.diff(H, axis=0) >= 0).all() and (np.diff(H, axis=1) >= 0).all() and len(np.unique(H)) > 50
    terrain = TR.Terrain(H, hscale, vscale, x0, y0)
    px, py = [-0.5, -0.25, 0.0, 0.25, 0.5], [-0.25, 0.0, 0.25]            # whole cells apart
    points = ref.height_points(px, py)
    ci, cj = rng.integers(2, 24 - 4, n), rng.integers(1, 20 - 3, n)       # the base's node: every sample stays below the last row and column
    origin = np.stack([hscale * rng.integers(-3, 4, n), hscale * rng.integers(-3, 4, n)], -1).astype(np.float64)
    root = np.zeros((n, 13), np.float32)
    root[:, 0], root[:, 1], root[:, 2] = x0 + hscale * ci - origin[:, 0], y0 + hscale * cj - origin[:, 1], 0.6
    root[:, 3:7] = np.where((np.arange(n) % 2 == 0)[:, None], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0])      # yaw 0 and 180 degrees: exact
    sim = _sim(n, terrain, origin)
    scan = HS.HeightScan(n, points_x=px, points_y=py, device=DEV)
    scan.bind(sim)
    heights = torch.zeros((n, len(points)), dtype=torch.float32, device=DEV)
    scan.measure(_dev(root), torch.zeros((n, 48), dtype=torch.float32, device=DEV), heights=heights)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None, None]
    xy = (sign * points[None].astype(np.float64) + root[:, None, :2].astype(np.float64) + origin[:, None, :])      # exact: multiples of 0.25
    u, v = (xy[..., 0] - x0) / hscale, (xy[..., 1] - y0) / hscale
    assert np.array_equal(u, np.rint(u)) and np.array_equal(v, np.rint(v)) and u.min() >= 0 and u.max() <= 22 and v.min() >= 0 and v.max() <= 18
    z, _ = sim.terrain_query(_dev(xy.reshape(-1, 2)), normals=False)
    got = heights.cpu().numpy()
    assert same(got, z.cpu().numpy().astype(np.float32).reshape(n, -1))
    assert same(got, (H[u.astype(int), v.astype(int)] * vscale).astype(np.float32)) and len(np.unique(got)) > 30


def _slope(d, r, c, hs, vs, s):
    return TR.pyramid_sloped_terrain(r, c, hs, vs, 0.1 + 0.2 * d, platform_size=1.5)


def _stairs(d, r, c, hs, vs, s):
    return TR.pyramid_stairs_terrain(r, c, hs, vs, 0.31, 0.03 + 0.04 * d, platform_size=2.0)


@functools.lru_cache(maxsize=None)
def grid():
    """3 levels x 2 types of 4 m tiles at 0.1 m inside a 1 m border: 140 x 100 nodes, slopes and stairs."""
    return TR.TerrainGrid(LEVELS, TYPES, TILE, TILE, hscale=0.1, vscale=0.005, border_size=1.0, generators=[_slope, _stairs])


def _cfg(**kw):
    return R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), **kw)


def _yaw(n):
    return np.random.default_rng(6).uniform(-np.pi, np.pi, n)


def test_in_the_task_the_48_columns_and_everything_else_are_untouched():
    import torch
    n, ticks, g = 65, 30, grid()
    cfg = _cfg(episode_length_s=0.12, seed=5)                              # twelve ticks an episode: resets inside the window
    origin = g.tile_origins.reshape(-1, 2)[np.arange(n) % (LEVELS * TYPES)] + np.random.default_rng(2).uniform(-1.2, 1.2, (n, 2))
    actions = _dev(np.random.default_rng(3).uniform(-1, 1, (ticks, n, 12)).astype(np.float32))
    field, points = _field_of(g.terrain), HS.height_points()
    out = []
    for with_scan in (False, True):
        scan = HS.HeightScan(n, device=DEV) if with_scan else None
        task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), terrain=g.terrain, origin=origin, height_scan=scan)
        width = 240 if with_scan else 48
        assert task.num_obs == width and task.obs_buf.shape == (n, width) and task.height_scan is scan
        rec = [torch.zeros((ticks, n, k), dtype=torch.float32, device=DEV) for k in (width, 1, 1, 12, 13, 187)]
        first = task.reset()
        assert first.data_ptr() == task.obs_buf.data_ptr() and first.shape == (n, width)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")        # a torch call that waits for the device or copies to the host raises from here on
        try:
            for k in range(ticks):
                o, r, d, _ = task.step(actions[k])
                rec[0][k].copy_(o); rec[1][k, :, 0].copy_(r); rec[2][k, :, 0].copy_(d); rec[3][k].copy_(task.torques); rec[4][k].copy_(task.sim.root_states)
                if with_scan:
                    rec[5][k].copy_(task.measured_heights)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        if with_scan:
            assert o.data_ptr() == task.obs_buf.data_ptr() != task.task.obs_buf.data_ptr() and task.measured_heights.shape == (n, 187)
            assert torch.equal(task.task.obs_buf, task.obs_buf[:, :48])
        out.append([x.cpu().numpy() for x in rec] + [task.bridge.ctl.solver_record(), K.sim_origins(task.sim)])
    plain, wide = out
    assert same(plain[0], wide[0][:, :, :48])                              # the task's own columns, bit for bit
    for a, b, name in zip(plain[1:5] + plain[6:], wide[1:5] + wide[6:], ("rewards", "resets", "torques", "root states", "controller records", "origins")):
        assert np.array_equal(a, b, equal_nan=True), name
    assert plain[2].sum(0).min() >= 2                                      # every environment was reset inside the window
    for k in range(ticks):                                                 # the scan columns: the restatement on that tick's root states
        want = ref.scan(field, wide[4][k], wide[7], points, wide[0][k, :, :48])
        assert same(wide[0][k], want["wide"]) and same(wide[5][k], want["heights"]), k
    cols = wide[0][:, :, 48:235]
    assert (wide[0][:, :, 235:] == 0).all() and len(np.unique(cols)) > 100 and (np.abs(cols) < 5).any()


def test_with_a_curriculum_a_moved_robot_sees_its_new_tile_in_the_same_tick():
    import torch
    n, g = 65, grid()
    cfg = _cfg(seed=9)
    chosen = [0, 62, 64]
    cur = K.TerrainCurriculum(g, n, max_init_level=1, seed=5, device=DEV, episode_length_s=cfg.episode_length_s)
    scan = HS.HeightScan(n, device=DEV)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), curriculum=cur, height_scan=scan)
    assert task.num_obs == 240 and task.curriculum is cur
    actions = _dev(np.random.default_rng(3).uniform(-1, 1, (4, n, 12)).astype(np.float32))
    task.reset()
    for k in range(3):
        task.step(actions[k])
    before = K.sim_origins(task.sim)
    st = task.sim.get_state()
    st["f64"][chosen, 0] += 2.5                                            # beyond env_length / 2 = 2 m, feet and all
    st["f64"][np.ix_(chosen, [37, 40, 43, 46])] += 2.5
    task.sim.set_state(st)
    mask = torch.zeros(n, dtype=torch.long, device=DEV)
    mask[chosen] = 1
    task.reset_buf.bitwise_or_(mask)
    obs = task.step(actions[3])[0].cpu().numpy()
    after, root = K.sim_origins(task.sim), task.sim.root_states.cpu().numpy()
    new = g.tile_origins[cur.levels0[chosen] + 1, cur.types[chosen]]
    assert np.array_equal(after[chosen], new) and not np.array_equal(before[chosen], new)
    others = [i for i in range(n) if i not in chosen]
    assert np.array_equal(after[others], before[others])
    field, points = _field_of(g.terrain), HS.height_points()
    want = ref.scan(field, root, after, points, obs[:, :48])
    assert same(obs, want["wide"]) and same(task.measured_heights.cpu().numpy(), want["heights"])
    stale = ref.scan(field, root, before, points, obs[:, :48])             # the old tile would have read otherwise
    assert not np.array_equal(stale["heights"][chosen], want["heights"][chosen])


class _Recording:
    """The task with every observation it hands out kept (a clone on the device)."""

    def __init__(self, env):
        self.env, self.seen = env, []
        self.num_envs, self.num_obs, self.num_actions, self.device, self.cfg = env.num_envs, env.num_obs, env.num_actions, env.device, env.cfg
        self.curriculum, self.progress_buf = env.curriculum, env.progress_buf

    def reset(self):
        obs = self.env.reset()
        self.seen.append(obs.clone())
        return obs

    def step(self, actions):
        out = self.env.step(actions)
        self.seen.append(out[0].clone())
        return out


@pytest.mark.parametrize("update,normalize", [("torch", False), ("hip", False), ("torch", True), ("hip", True)])
def test_trainer_learns_on_the_wide_rows(update, normalize, tmp_path):
    import torch
    from rl_mpc_locomotion_amd import ppo as P
    from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
    n, g = 64, grid()
    cfg = _cfg(episode_length_s=0.05, seed=4)
    pcfg = P.PPOConfig(num_steps_per_env=8, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    cur = K.TerrainCurriculum(g, n, max_init_level=1, seed=2, device=DEV, episode_length_s=cfg.episode_length_s)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), curriculum=cur, height_scan=HS.HeightScan(n, device=DEV))
    env = _Recording(task)
    trainer = P.PPOTrainer(env, pcfg, seed=3, update=update, normalize_obs=normalize)
    ac, st = trainer.actor_critic, trainer.storage
    assert ac.num_obs == 240 and ac.actor[0].in_features == 240 and ac.critic[0].in_features == 240
    assert st.observations.shape == (8, n, 240)
    if normalize:
        assert trainer.obs_norm.num_obs == 240
    before = [p.detach().clone() for p in ac.parameters()]
    infos = trainer.learn(1)
    assert len(infos) == 1 and all(np.isfinite(v) for k, v in infos[0].items() if k != "terrain_level_by_type")
    assert any(not torch.equal(a, b) for a, b in zip(before, ac.parameters()))
    assert torch.isfinite(st.observations).all().item() and (st.observations[:, :, 235:] == 0).all().item()      # the pad: 0 before and after normalisation
    assert (task.obs_buf[:, 235:] == 0).all().item() and (trainer.obs[:, 235:] == 0).all().item()
    seen = torch.stack(env.seen)                                           # the reset's observation and the eight ticks'
    assert seen.shape == (9, n, 240) and (seen[:, :, 235:] == 0).all().item()
    if normalize:
        assert not torch.equal(trainer.obs, task.obs_buf) and not torch.equal(st.observations, seen[:8])
    else:                                                                  # the storage's columns are the environment's, all 240 of them
        assert torch.equal(st.observations, seen[:8]) and torch.equal(trainer.obs, task.obs_buf) and torch.equal(trainer.obs, seen[8])
    scans = st.observations[:, :, 48:235]
    assert len(torch.unique(scans)) > 50                                   # the storage holds the environment's scan columns, not a constant
    path = tmp_path / "ck.pt"
    trainer.save(path)
    policy = WeightPolicy.from_state_dict(torch.load(path)["model_state_dict"], device=DEV)
    assert policy.num_obs == 240 and policy.dims[0] == 240
    rows = st.observations.reshape(-1, 240).contiguous()
    assert torch.equal(ac.act_inference(rows), policy.step(rows, return_actions=True)[1])


def test_argument_errors_come_back_before_any_launch():
    import torch
    n, g = 8, grid()
    scan = HS.HeightScan(n, device=DEV)
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    root, obs = torch.zeros((n, 13), dtype=torch.float32, device=DEV), torch.zeros((n, 48), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*no sim bound"):
        scan.measure(root, obs)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*no terrain"):
        scan.bind(BatchedToySim(_robots(n), device=DEV))                   # a plane sim
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*9 robots"):
        scan.bind(_sim(n + 1, g.terrain, None))                            # another size
    scan.bind(_sim(n, g.terrain, None))
    L = HS.lib()
    assert L.mpc_hscan_run(scan._handle, root.data_ptr(), obs.data_ptr(), -1, obs.data_ptr() + 4096, None, None) == -1
    assert L.mpc_hscan_run(scan._handle, root.data_ptr(), None, 48, obs.data_ptr(), None, None) == -1
    assert L.mpc_hscan_run(scan._handle, root.data_ptr(), obs.data_ptr(), 48, obs.data_ptr(), None, None) == -1 and b"must not be" in L.mpc_hscan_last_error()
    assert L.mpc_hscan_run(scan._handle, None, obs.data_ptr(), 48, obs.data_ptr(), None, None) == -1
    for bad in (dict(root_states=root.double()), dict(root_states=root[:-1]), dict(obs_in=obs.double()), dict(obs_in=obs[:-1]), dict(obs_in=obs[:, ::2]),
                dict(out=torch.zeros((n, 239), dtype=torch.float32, device=DEV)), dict(heights=torch.zeros((n, 186), dtype=torch.float32, device=DEV))):
        with pytest.raises(ValueError):
            scan.measure(**{**dict(root_states=root, obs_in=obs), **bad})
    with pytest.raises(ValueError, match="terrain"):
        R.BatchedRLTask(_robots(n), [TROT] * n, device=DEV, height_scan=scan)
    with pytest.raises(ValueError, match="environments"):
        R.BatchedRLTask(_robots(n + 1), [TROT] * (n + 1), device=DEV, terrain=g.terrain, height_scan=scan)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*point 0"):
        HS.HeightScan(n, points_x=[np.nan], points_y=[0.0], device=DEV)
    assert scan.measure(root, obs).shape == (n, 240)                       # and the bound scan still runs
