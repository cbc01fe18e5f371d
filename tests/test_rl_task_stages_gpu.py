"""BatchedRLTask.step's ``mark`` on the MI355X: a task stepped with a mark computes, byte for byte, what its twin stepped without one computes, and
the marks of a tick are exactly rl_task.STAGES filtered to the options the task has -- with every option on, and with none.  Rests on what the
noisy-against-clean test of tests/test_privileged_obs_gpu.py rests on: the generators are counter-based and two runs of the solver are deterministic."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import curriculum as K, domain_rand as D, episode_terms as E, height_scan as HS, privileged_obs as V, rl_task as R
from tests.test_height_scan_gpu import DEV, TROT, _cfg, _dev, _robots, _yaw, grid, same

pytestmark = pytest.mark.gpu
TICKS = 12
PLAIN = ("actions", "controller", "plant", "begin", "resets", "finish")
FIELDS = ("obs_buf", "rew_buf", "reset_buf", "timeout_buf", "progress_buf", "commands", "privileged_obs_buf", "measured_heights")


def _task(n, every_option):
    g = grid()
    cfg = _cfg(episode_length_s=0.08, seed=5)                              # 8 ticks an episode: resets, time-outs and command redraws inside the window
    assert cfg.max_episode_length == 8
    if not every_option:
        origin = g.tile_origins.reshape(-1, 2)[np.arange(n) % 6] + np.random.default_rng(2).uniform(-1.2, 1.2, (n, 2))
        return R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), terrain=g.terrain, origin=origin)
    scan = HS.HeightScan(n, points_x=(-0.4, -0.2, 0.0, 0.2, 0.4), points_y=(-0.2, 0.0, 0.2), device=DEV)      # 5 x 3
    dr = D.DomainRand(n, observations=D.NoiseSpec("gaussian", "additive", (0.0, 0.05)), actions=D.NoiseSpec("gaussian", "additive", (0.0, 0.02)),
                      push=D.PushSpec(interval_s=0.02, max_vel_xy=0.5), seed=3, device=DEV)
    et = E.EpisodeTerms(n, cfg, command_curriculum=E.CommandCurriculumSpec(1.5, x_range0=(-0.5, 0.5), threshold=0.0, update_every=1), device=DEV)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=_yaw(n), height_scan=scan, domain_rand=dr, episode_terms=et,
                           curriculum=K.TerrainCurriculum(g, n, max_init_level=1, seed=5, device=DEV, episode_length_s=cfg.episode_length_s),
                           privileged_obs=V.PrivilegedObs(n, device=DEV))
    assert dr.push_interval == 2 and task.measured_heights.shape == (n, 15)
    return task


def _fields(task):
    out = {k: getattr(task, k) for k in FIELDS if getattr(task, k, None) is not None}
    out["sim.root_states"], out["sim.dof_state"] = task.sim.root_states, task.sim.dof_state
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("every_option", (True, False), ids=("every_option", "no_option"))
@pytest.mark.parametrize("n", (3, 65))     # less than one wave; one wave into a second workgroup of the one-wave-per-environment kernels
def test_a_marked_step_computes_what_an_unmarked_one_does_and_marks_its_stages(n, every_option):
    plain, marked = _task(n, every_option), _task(n, every_option)
    want = R.STAGES if every_option else PLAIN
    assert [s for s in R.STAGES if s in want] == list(want)
    actions = _dev(np.random.default_rng(3).uniform(-1.5, 1.5, (TICKS, n, 12)).astype(np.float32))      # beyond clip_actions: the clamp has work
    plain.reset()
    marked.reset()
    seen, resets, time_outs = [], 0, 0
    for k in range(TICKS):
        plain.step(actions[k])
        out = marked.step(actions[k], mark=seen.append)
        assert tuple(seen) == tuple(want), k
        seen.clear()
        a, b = _fields(plain), _fields(marked)
        assert list(a) == list(b) and len(a) == (10 if every_option else 8)
        for name in a:
            assert same(a[name], b[name]), (k, name)
        assert out[0].data_ptr() == marked.obs_buf.data_ptr() and out[3]["time_outs"].data_ptr() == marked.timeout_buf.data_ptr()
        resets, time_outs = resets + int(b["reset_buf"].sum()), time_outs + int(b["timeout_buf"].sum())
    assert resets >= n and time_outs >= 1                                   # the window held resets and time-outs
    if every_option:
        assert marked.domain_rand.launches == plain.domain_rand.launches == {"observations": TICKS + 1, "actions": TICKS + 1, "push": (TICKS + 1) // 2}
        assert marked.common_step_counter == plain.common_step_counter == TICKS + 1
