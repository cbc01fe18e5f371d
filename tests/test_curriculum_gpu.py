"""The terrain curriculum on the MI355X (csrc/mpc_curriculum.h, rl_mpc_locomotion_amd.curriculum): the update kernel against the restatement of
tests/curriculum_ref.py on the crafted batch (levels, counters and origins EQUAL, sentinels untouched, reruns identical), the summary kernel against
numpy, and the hook in BatchedRLTask.step and PPOTrainer.learn: forced promotions land on the new tile and touch nobody else, nothing reaches the host,
a curriculum that decides nothing changes nothing, the records carry the levels."""
import functools

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, curriculum as K, rl_task as R, terrain as TR
from tests import curriculum_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
SIZES = (1, 63, 64, 65, 130)           # one lane, a wave less one, a full wave, one lane into the second workgroup, a third partial one
LEVELS, TYPES, TILE, EPISODE_S = 3, 2, 4.0, 20.0


def _slope(d, r, c, hs, vs, s):
    return TR.pyramid_sloped_terrain(r, c, hs, vs, 0.1 + 0.2 * d, platform_size=1.5)


def _stairs(d, r, c, hs, vs, s):
    return TR.pyramid_stairs_terrain(r, c, hs, vs, 0.31, 0.03 + 0.04 * d, platform_size=2.0)


@functools.lru_cache(maxsize=None)
def grid():
    """3 levels x 2 types of 4 m tiles at 0.1 m inside a 1 m border: 140 x 100 nodes.  Every tile's centre is a flat platform at a height of its own."""
    g = TR.TerrainGrid(LEVELS, TYPES, TILE, TILE, hscale=0.1, vscale=0.005, border_size=1.0, generators=[_slope, _stairs])
    assert (g.terrain.rows, g.terrain.cols) == (140, 100)
    tops = set()
    for i in range(LEVELS):
        for j in range(TYPES):
            ci, cj = g.terrain.cell(*g.tile_origins[i, j])[:2]
            blk = g.terrain.heights[ci - 4:ci + 5, cj - 4:cj + 5]
            assert blk.min() == blk.max() > 0                              # +-0.4 m around the centre: the stance's feet stand on it
            tops.add(int(blk[0, 0]))
    assert len(tops) == LEVELS * TYPES
    return g


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _robots(n):
    return [i % 3 for i in range(n)]


def _sim(n, origin, terrain="grid"):
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    yaw = np.random.default_rng(6).uniform(-np.pi, np.pi, n)
    if terrain is None:
        return BatchedToySim(_robots(n), yaw0=yaw, device=DEV)
    return BatchedToySim(_robots(n), yaw0=yaw, device=DEV, terrain=grid().terrain, origin=origin)


@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_equals_the_restatement_on_the_crafted_batch(n):
    import torch
    g, seed = grid(), 4321
    case = ref.crafted(n, LEVELS, TYPES, TILE, EPISODE_S)
    cur = K.TerrainCurriculum(g, n, seed=seed, device=DEV, episode_length_s=EPISODE_S, types=case["types"])
    assert cur.levels.dtype == torch.int32 and cur.levels.shape == (n,) and cur.levels.is_cuda and not cur.levels.any().item()
    sim = _sim(n, cur.origins0)
    assert np.array_equal(K.sim_origins(sim), cur.origins0)
    cur.bind(sim)
    view = K.sim_origin_view(sim)
    assert view.dtype == torch.float64 and view.shape == (n, 2) and np.array_equal(view.cpu().numpy(), cur.origins0)
    sent = np.tile(np.array(ref.SENTINEL_ORIGIN), (n, 1))
    reset, root, commands = _dev(case["reset"]), _dev(case["root"]), _dev(case["commands"])
    runs = []
    for _ in range(2):                                                     # the same start twice: bit-identical
        cur.levels.copy_(_dev(case["levels"])); cur.counts.zero_(); view.copy_(_dev(sent))
        cur.update(reset, root, commands)
        first = (cur.levels.cpu().numpy(), cur.counts.cpu().numpy(), K.sim_origins(sim))
        cur.update(reset, root, commands)                                  # and a second reset from where the first left: the counter keys the redraw
        runs.append(first + (cur.levels.cpu().numpy(), cur.counts.cpu().numpy(), K.sim_origins(sim)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    w1 = ref.update(case["reset"], case["root"], case["commands"], case["types"], g.tile_origins, case["levels"], np.zeros(n, np.int32), sent, TILE,
                    EPISODE_S, seed)
    w2 = ref.update(case["reset"], case["root"], case["commands"], case["types"], g.tile_origins, *w1[:3], TILE, EPISODE_S, seed)
    for got, want, name in zip(runs[0], w1[:3] + w2[:3], ("levels", "counts", "origins", "levels 2", "counts 2", "origins 2")):
        assert np.array_equal(got, want), name
    levels, counts, origins = runs[0][:3]
    idle = case["reset"] == 0
    assert (levels[idle] == ref.SENTINEL_LEVEL).all() and (counts[idle] == 0).all() and origins[idle].tobytes() == sent[idle].tobytes()
    assert (runs[0][3][idle] == ref.SENTINEL_LEVEL).all() and runs[0][5][idle].tobytes() == sent[idle].tobytes()
    for r in np.flatnonzero(~idle):
        want = case["expect"][r]
        if want is None:
            assert 0 <= levels[r] < LEVELS and levels[r] == ref.draw_level(seed, int(r), 1, LEVELS), r
        else:
            assert levels[r] == max(int(case["levels"][r]) + want, 0), r
    # the sim's own reset now stands the flagged robots on the new tiles
    if n >= ref.PATTERN:
        sim.reset_idx(_dev(np.where(idle, -1, np.arange(n)).astype(np.int32)))
        moved = np.flatnonzero(~idle)
        fresh = _sim(n, np.where(idle[:, None], cur.origins0, runs[0][5])).get_state()
        np.testing.assert_allclose(sim.get_state()["f64"][moved], fresh["f64"][moved], rtol=0, atol=1e-12)


@pytest.mark.parametrize("n", SIZES + (1025, 2049))
def test_summary_kernel_equals_numpy(n):
    import torch
    g = grid()
    cur = K.TerrainCurriculum(g, n, max_init_level=LEVELS - 1, seed=n, device=DEV)
    s = cur.summary()
    assert s.dtype == torch.float64 and s.shape == (2 + 2 * TYPES,) and s.data_ptr() == cur.summary().data_ptr()
    assert np.array_equal(s.cpu().numpy(), ref.summary(cur.levels0, cur.types, TYPES))
    if n == 1:
        assert s.cpu().numpy().tolist() == [1.0, float(cur.levels0[0]), 1.0, 0.0, float(cur.levels0[0]), 0.0]          # a type without members: mean 0.0
    else:
        assert len(np.unique(cur.levels0)) > 1 and set(cur.types.tolist()) == {0, 1}
    levels = np.random.default_rng(n).integers(0, LEVELS, n).astype(np.int32)
    cur.levels.copy_(_dev(levels))
    assert np.array_equal(cur.summary().cpu().numpy(), ref.summary(levels, cur.types, TYPES))
    one_type = K.TerrainCurriculum(g, n, max_init_level=LEVELS - 1, seed=n, device=DEV, types=np.ones(n, np.int32))
    assert np.array_equal(one_type.summary().cpu().numpy(), ref.summary(one_type.levels0, one_type.types, TYPES))


def _cfg(**kw):
    return R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), **kw)


def _task(n, cur, cfg):
    yaw = np.random.default_rng(6).uniform(-np.pi, np.pi, n)
    return R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=yaw, curriculum=cur)


@pytest.mark.parametrize("n", SIZES)
def test_forced_promotions_land_on_the_new_tile_and_touch_nobody_else(n):
    import torch
    g, cfg = grid(), _cfg(seed=9)
    chosen = [i for i in (0, 62, 64, 129) if i < n]
    others = [i for i in range(n) if i not in chosen]
    actions = _dev(np.random.default_rng(3).uniform(-1, 1, (6, n, 12)).astype(np.float32))
    mask = torch.zeros(n, dtype=torch.long, device=DEV)
    mask[chosen] = 1
    runs = []
    for moved in (False, True):
        cur = K.TerrainCurriculum(g, n, max_init_level=1, seed=5, device=DEV, episode_length_s=cfg.episode_length_s)
        task = _task(n, cur, cfg)
        assert task.curriculum is cur and task.sim.terrain is g.terrain and np.array_equal(task.sim.origin, cur.origins0)
        task.reset()
        assert np.array_equal(cur.levels.cpu().numpy(), cur.levels0) and (cur.counts == 1).all().item()       # the first tick resets everybody and moves nobody
        assert np.array_equal(K.sim_origins(task.sim), cur.origins0)
        for k in range(3):
            task.step(actions[k])
        if moved:
            st = task.sim.get_state()
            st["f64"][chosen, 0] += 2.5                                    # beyond env_length / 2 = 2 m, feet and all
            st["f64"][np.ix_(chosen, [37, 40, 43, 46])] += 2.5
            task.sim.set_state(st)
            assert (task.commands[chosen, :2].abs().sum(1) > 0).all().item()
            task.reset_buf.bitwise_or_(mask)
        obs = [task.step(actions[3])[0].clone()]
        after = task.sim.get_state()
        levels, origins = cur.levels.cpu().numpy(), K.sim_origins(task.sim)
        for k in (4, 5):
            obs.append(task.step(actions[k])[0].clone())
        end = task.sim.get_state()
        runs.append(dict(obs=torch.stack(obs).cpu().numpy(), after=after, end=end, levels=levels, origins=origins, record=task.bridge.ctl.solver_record(),
                         counts=cur.counts.cpu().numpy(), progress=task.progress_buf.cpu().numpy(), levels0=cur.levels0, types=cur.types))
    a, b = runs
    assert np.array_equal(a["levels"], a["levels0"]) and (a["counts"] == 1).all() and (a["progress"] == 6).all()      # nobody reset on its own in six ticks
    # the moved: one level up, on the new tile, standing as a fresh robot stands there
    assert np.array_equal(b["levels"][chosen], b["levels0"][chosen] + 1) and (b["counts"][chosen] == 2).all() and (b["progress"][chosen] == 2).all()
    new = g.tile_origins[b["levels0"][chosen] + 1, b["types"][chosen]]
    assert np.array_equal(b["origins"][chosen], new) and not np.array_equal(new, a["origins"][chosen])
    origin = a["origins"].copy()
    origin[chosen] = new
    fresh = _sim(n, origin)
    np.testing.assert_allclose(b["after"]["f64"][chosen], fresh.get_state()["f64"][chosen], rtol=0, atol=1e-12)
    ground, _ = fresh.terrain_query(_dev(new), normals=False)
    stance = _sim(n, None, terrain=None).get_state()["f64"][chosen, 2]    # the stance height: a fresh robot's base above its plane
    np.testing.assert_allclose(b["after"]["f64"][chosen, 2], ground.cpu().numpy() + stance, rtol=0, atol=1e-12)
    assert np.array_equal(ground.cpu().numpy(), g.terrain.height(new[:, 0], new[:, 1])) and len(set(ground.cpu().numpy().tolist())) == len({tuple(x) for x in new})
    # everybody else: bit for bit the run in which nobody was moved
    if others:
        assert np.array_equal(a["obs"][:, others], b["obs"][:, others])
        for key in ("after", "end"):
            assert np.array_equal(a[key]["f64"][others], b[key]["f64"][others]) and np.array_equal(a[key]["i32"][others], b[key]["i32"][others])
        assert np.array_equal(a["record"][others], b["record"][others])
        for key in ("levels", "origins", "counts", "progress"):
            assert np.array_equal(a[key][others], b[key][others]), key
    assert not np.array_equal(a["end"]["f64"][chosen], b["end"]["f64"][chosen])


def test_fifty_ticks_without_a_host_synchronisation():
    import torch
    n, g = 130, grid()
    cfg = _cfg(episode_length_s=0.2, seed=2)                               # twenty ticks an episode: resets, and with them promotions and demotions
    cur = K.TerrainCurriculum(g, n, max_init_level=1, seed=8, device=DEV, env_length=0.002, episode_length_s=cfg.episode_length_s)
    task = _task(n, cur, cfg)
    actions = _dev(np.random.default_rng(5).uniform(-1, 1, (50, n, 12)).astype(np.float32))
    summaries = torch.zeros((50, 2 + 2 * TYPES), dtype=torch.float64, device=DEV)
    task.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # a torch call that waits for the device or copies to the host raises from here on
    try:
        for k in range(50):
            task.step(actions[k])
            summaries[k].copy_(cur.summary())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    levels, counts, s = cur.levels.cpu().numpy(), cur.counts.cpu().numpy(), summaries.cpu().numpy()
    assert (counts >= 3).all() and levels.min() >= 0 and levels.max() < LEVELS
    assert np.array_equal(K.sim_origins(task.sim), g.tile_origins[levels, cur.types])
    assert np.array_equal(s[-1], ref.summary(levels, cur.types, TYPES)) and (s[:, 0] == n).all()
    assert len(np.unique(s[:, 1])) > 2                 # with a tile "length" of 2 mm the levels move: up, and past the top into the redraw


def test_a_curriculum_that_decides_nothing_changes_nothing():
    import torch
    n, g = 130, grid()
    cfg = _cfg(episode_length_s=0.3, seed=4)
    cur = K.TerrainCurriculum(g, n, max_init_level=LEVELS - 1, seed=1, device=DEV, env_length=1e9, episode_length_s=0.0)
    yaw = np.random.default_rng(6).uniform(-np.pi, np.pi, n)
    plain = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=yaw, terrain=g.terrain, origin=cur.origins0)
    hooked = _task(n, cur, cfg)
    assert plain.curriculum is None
    actions = _dev(np.random.default_rng(7).uniform(-1, 1, (100, n, 12)).astype(np.float32))
    out = []
    for task in (plain, hooked):
        rec = [torch.zeros((100, n, k), dtype=torch.float32, device=DEV) for k in (48, 1, 1, 12)]
        task.reset()
        for k in range(100):
            o, r, d, _ = task.step(actions[k])
            rec[0][k].copy_(o); rec[1][k, :, 0].copy_(r); rec[2][k, :, 0].copy_(d); rec[3][k].copy_(task.torques)
        st = task.sim.get_state()
        out.append([x.cpu().numpy() for x in rec] + [st["f64"], st["i32"], task.bridge.ctl.solver_record(), task.commands.cpu().numpy()])
    for x, y in zip(*out):
        assert np.array_equal(x, y, equal_nan=True)
    assert out[0][2].sum(0).min() >= 2                                     # every environment was reset, more than once
    assert np.array_equal(cur.levels.cpu().numpy(), cur.levels0) and (cur.counts.cpu().numpy() >= 3).all()
    assert np.array_equal(K.sim_origins(hooked.sim), cur.origins0) and len(np.unique(cur.levels0)) == LEVELS


KEYS = {"iter", "mean_reward", "done_rate", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate", "mean_episode_return", "mean_episode_length",
        "episodes_in_window", "episodes_finished", "timeouts_in_window"}


@pytest.mark.parametrize("update", ["torch", "hip"])
def test_trainer_records_carry_the_levels(update):
    from rl_mpc_locomotion_amd import ppo as P
    n, g = 64, grid()
    cfg = _cfg(episode_length_s=0.05, seed=4)
    pcfg = P.PPOConfig(num_steps_per_env=16, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    cur = K.TerrainCurriculum(g, n, max_init_level=1, seed=2, device=DEV, env_length=0.0002, episode_length_s=cfg.episode_length_s)
    infos = P.PPOTrainer(_task(n, cur, cfg), pcfg, seed=3, update=update).learn(1)
    assert len(infos) == 1 and set(infos[0]) == KEYS | {"mean_terrain_level", "terrain_level_by_type"}
    levels = cur.levels
    assert infos[0]["mean_terrain_level"] == levels.float().mean().item()
    by_type = [levels[_dev(cur.types == t)].float().mean().item() for t in range(TYPES)]
    assert infos[0]["terrain_level_by_type"] == by_type and not np.array_equal(levels.cpu().numpy(), cur.levels0)
    yaw = np.random.default_rng(6).uniform(-np.pi, np.pi, n)
    plain = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=yaw, terrain=g.terrain, origin=cur.origins0)
    infos = P.PPOTrainer(plain, pcfg, seed=3, update=update).learn(1)
    assert set(infos[0]) == KEYS


def test_argument_errors_come_back_before_any_launch():
    n, g = 8, grid()
    cur = K.TerrainCurriculum(g, n, device=DEV)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*no terrain"):
        cur.bind(_sim(n, None, terrain=None))                              # a plane sim
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*9 robots"):
        cur.bind(_sim(n + 1, None))                                        # another size
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*no sim bound"):
        cur.update(_dev(np.ones(n, np.int64)), _dev(np.zeros((n, 13), np.float32)), _dev(np.zeros((n, 3), np.float32)))
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*level of environment 3"):
        K.TerrainCurriculum(g, n, device=DEV, levels0=[0, 1, 2, 3, 0, 0, 0, 0])
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*type of environment 0"):
        K.TerrainCurriculum(g, n, device=DEV, types=[-1] * n)
    with pytest.raises(ValueError):
        K.TerrainCurriculum(g, n, max_init_level=LEVELS, device=DEV)
    with pytest.raises(ValueError, match="curriculum"):
        R.BatchedRLTask(_robots(n), [TROT] * n, device=DEV, terrain=g.terrain, curriculum=cur)
    with pytest.raises(ValueError, match="curriculum"):
        R.BatchedRLTask(_robots(n), [TROT] * n, device=DEV, origin=cur.origins0, curriculum=cur)
    with pytest.raises(ValueError):
        cur.update(_dev(np.ones(n, np.int32)), _dev(np.zeros((n, 13), np.float32)), _dev(np.zeros((n, 3), np.float32)))      # int32 flags
    sim = _sim(n, cur.origins0)
    cur.bind(sim)
    with pytest.raises(ValueError):
        cur.update(_dev(np.ones(n + 1, np.int64)), _dev(np.zeros((n, 13), np.float32)), _dev(np.zeros((n, 3), np.float32)))
