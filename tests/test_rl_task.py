"""The RL task's post-physics half (csrc/rl_task.h, include/mpc_task.h, rl_mpc_locomotion_amd.rl_task) against the reference's own functions
(tests/golden/rl_task_{aliengo,a1,go1}.npz, minted by tests/golden/make_golden_rl_task.py), on the CPU: the header is compiled with g++ into a
small shim and driven through ctypes.

Tolerances are derived, not measured from the code under test.  An observation that is a copy, or one or two correctly rounded float32 operations on
float32 inputs (scaled commands, (dof_pos - default) * scale, dof_vel * scale, the clip), has one possible value: bit-identical.  The six rotated
velocities and the reward are chains of ~20 float32 operations (and an exp) whose association torch does not pin, so they are held to 4 x the
reference's own float32-vs-float64 gap on the same rows, which the fixture records (about 1e-6 and 6e-9).  Every integer buffer is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, rl_task as R
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mpc_task.h")
HIPCC = "/opt/rocm/bin/hipcc"
ROBOTS = ("aliengo", "a1", "go1")
ROT = slice(3, 9)                      # body-frame linear and angular velocity
EXACT = np.r_[0:3, 9:48]               # everything else

SHIM = r"""
#include "rl_task.h"
using namespace rltask;
extern "C" {
void shim_begin(const Config *c, int n, long long *progress, long long *reset, long long *timeout, int *episode, int *ids, float *commands) {
  for (int r = 0; r < n; ++r) {
    float cmd[3];
    ids[r] = begin_env(*c, r, progress[r], reset[r], timeout[r], episode[r], cmd);
    if (ids[r] >= 0) for (int a = 0; a < 3; ++a) commands[3 * r + a] = cmd[a];
  }
}
void shim_finish(const Config *c, int n, const float *root, const float *dof, const float *commands, const float *actions, const float *torques,
                 const float *cf, int bodies, int base, const int *knee, const int *hip, const unsigned char *fell, const long long *progress,
                 float *obs, float *rew, long long *reset) {
  for (int r = 0; r < n; ++r) {
    observe(*c, root + 13 * r, dof + 24 * r, commands + 3 * r, actions + 12 * r, obs + 48 * r);
    Contacts k{false, false, 0};
    if (cf) k = contacts_from_forces(cf + (long)r * 3 * bodies, base, knee, hip);
    if (fell) k.base = k.base || fell[r] != 0;
    bool rs;
    rew[r] = reward_reset(*c, root + 13 * r, commands + 3 * r, torques + 12 * r, k, progress[r], rs);
    reset[r] = rs ? 1 : 0;
  }
}
void shim_uniform(unsigned long long seed, int env0, int n_env, int episode0, int n_episode, int axis, float *out) {
  for (int e = 0; e < n_env; ++e)
    for (int p = 0; p < n_episode; ++p) out[(long)e * n_episode + p] = uniform01(seed, env0 + e, episode0 + p, axis);
}
void shim_sample(const Config *c, int env, int episode, float *out) { sample_commands(*c, env, episode, out); }
}
"""


class ShimConfig(C.Structure):         # rltask::Config
    _fields_ = [("scales", C.c_float * 4), ("rew", C.c_float * 6), ("cmd_lo", C.c_float * 3), ("cmd_hi", C.c_float * 3), ("clip_obs", C.c_float),
                ("default_dof_pos", C.c_float * 12), ("max_episode_length", C.c_longlong), ("seed", C.c_ulonglong)]


def shim_config(cfg):
    """TaskConfig -> rltask::Config, with the roundings mpc_task_create applies (double -> float32)."""
    s = cfg._struct()
    c = ShimConfig()
    c.scales[:] = [s.lin_vel_scale, s.ang_vel_scale, s.dof_pos_scale, s.dof_vel_scale]
    c.rew[:] = list(s.rew_scale)
    c.cmd_lo[:] = [s.command_range[a][0] for a in range(3)]
    c.cmd_hi[:] = [s.command_range[a][1] for a in range(3)]
    c.clip_obs = s.clip_observations
    c.default_dof_pos[:] = list(s.default_dof_pos)
    c.max_episode_length, c.seed = s.max_episode_length, s.seed
    return c


def batch_config():
    """The configuration the batch half of the fixtures was minted with (the yaml's commented alternative scales, knee collision -0.25)."""
    return R.TaskConfig(lin_vel_scale=2.0, ang_vel_scale=0.25, dof_pos_scale=1.0, dof_vel_scale=0.05, rew_collision=-0.25)


def sequence_config(seed=0):
    """The yaml's own values, the episode shortened to 40 ticks."""
    return R.TaskConfig(episode_length_s=0.4, seed=seed)


_GOLD = {}


def gold(robot):
    if robot not in _GOLD:
        g = np.load(os.path.join(ROOT, "tests", "golden", f"rl_task_{robot}.npz"))
        _GOLD[robot] = {k: g[k] for k in g.files}
        for a in _GOLD[robot].values():
            a.setflags(write=False)
    return _GOLD[robot]


def check_outputs(obs, rew, reset, g_obs, g_rew, g_reset, gap_rot, gap_rew, clip, what):
    """obs / rew / reset of the code under test against the reference's, under the rules at the head of this file.  g_obs may be unclipped."""
    want = np.clip(g_obs, -clip, clip)
    d_rot = float(np.abs(obs[:, ROT].astype(np.float64) - want[:, ROT]).max())
    d_rew = float(np.abs(rew.astype(np.float64) - g_rew).max())
    print(f"{what}: rotated velocities {d_rot:.3e} (bound {4 * gap_rot:.3e}), reward {d_rew:.3e} (bound {4 * gap_rew:.3e})")
    assert np.array_equal(obs[:, EXACT], want[:, EXACT]), f"{what}: a copied / single-operation observation differs"
    assert np.array_equal(reset.astype(bool), g_reset.astype(bool)), f"{what}: reset flags differ"
    assert d_rot <= 4 * gap_rot, f"{what}: rotated velocities off by {d_rot:.3e} > {4 * gap_rot:.3e}"
    assert d_rew <= 4 * gap_rew, f"{what}: reward off by {d_rew:.3e} > {4 * gap_rew:.3e}"
    assert np.abs(obs).max() <= clip


def compact_ids(ids):
    """An id array of begin (r or -1 per environment) as the reference's compact `env_ids`, padded with -1."""
    n = len(ids)
    assert all(ids[i] in (-1, i) for i in range(n))
    out = np.full(n, -1, np.int32)
    hit = ids[ids >= 0]
    out[:len(hit)] = hit
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("rl_task_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    for f in (L.shim_begin, L.shim_finish, L.shim_uniform, L.shim_sample):
        f.restype = None
    vp, ci = C.c_void_p, C.c_int
    L.shim_begin.argtypes = [vp, ci] + [vp] * 6
    L.shim_finish.argtypes = [vp, ci] + [vp] * 6 + [ci, ci] + [vp] * 7
    L.shim_uniform.argtypes = [C.c_ulonglong, ci, ci, ci, ci, ci, vp]
    L.shim_sample.argtypes = [vp, ci, ci, vp]
    return L


def host_finish(L, cfg, root, dof, commands, actions, torques, progress, contact=None, idx=None, fell=None):
    n = len(root)
    c = shim_config(cfg)
    a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
    root, dof, commands, actions, torques = (a(x, np.float32) for x in (root, dof, commands, actions, torques))
    progress = a(progress, np.int64)
    obs, rew, reset = np.zeros((n, 48), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64)
    cf = bodies = base = knee = hip = None
    if contact is not None:
        cf = a(contact, np.float32)
        bodies, base, knee, hip = cf.shape[1], int(idx[0]), a(idx[1], np.int32), a(idx[2], np.int32)
    fl = None if fell is None else a(fell, np.uint8)
    p = lambda x: None if x is None else x.ctypes.data
    L.shim_finish(C.addressof(c), n, p(root), p(dof), p(commands), p(actions), p(torques), p(cf), bodies or 0, base or 0, p(knee), p(hip), p(fl), p(progress),
                  p(obs), p(rew), p(reset))
    return obs, rew, reset


@pytest.mark.parametrize("robot", ROBOTS)
def test_batch_matches_the_reference_functions(shim, robot):
    g = gold(robot)
    # the fixture's own input conditions: what makes this comparison worth something
    assert g["b_cond_contact_margin"] >= 0.4 and g["b_cond_positive_reward"] >= 0.5 and g["b_cond_clamped"] > 0.02
    assert min(g["b_cond_base"], g["b_cond_knee"], g["b_cond_hip"], g["b_cond_timeout"], g["b_cond_no_reset"]) >= 0.02
    assert not (g["b_episode"] == g["b_max_len"]).any() and np.abs(g["b_obs"]).max() > 5.0
    cfg = batch_config()
    assert cfg.max_episode_length == int(g["b_max_len"]) and np.allclose(cfg.reward_scales(), g["b_rew_scales"], rtol=1e-15, atol=0)
    obs, rew, reset = host_finish(shim, cfg, g["b_root"], g["b_dof"], g["b_commands"], g["b_actions"], g["b_torques"], g["b_episode"], g["b_contact"],
                                  (g["base_index"], g["knee_indices"], g["hip_indices"]))
    check_outputs(obs, rew, reset, g["b_obs"], g["b_rew"], g["b_reset"], float(g["b_gap_rot"]), float(g["b_gap_rew"]), float(g["clip"]), f"{robot} batch")
    # the float64 recomputation is the same distance away as the float32 one is from it, give or take: nothing is hidden in the choice of reference
    assert np.abs(rew.astype(np.float64) - g["b_rew64"]).max() <= 5 * float(g["b_gap_rew"])
    assert np.abs(obs[:, ROT].astype(np.float64) - np.clip(g["b_rot64"], -5, 5)).max() <= 5 * float(g["b_gap_rot"])


def replay_sequence(g, cfg, begin, finish):
    """The 120-tick sequence of the fixture through begin / finish callables (host shim or device kernels); commands are taken from the golden
    after each begin, because the command generator is not torch's."""
    n = g["s_progress"].shape[1]
    lo, hi = np.array(g["command_ranges"], np.float32).T
    resets = 0
    for k in range(g["s_progress"].shape[0]):
        before = None if k == 0 else g["s_commands"][k - 1]
        progress, timeout, ids, commands = begin()
        assert np.array_equal(progress, g["s_progress"][k]), f"tick {k}: progress_buf"
        assert np.array_equal(timeout, g["s_timeout"][k]), f"tick {k}: timeout_buf"
        assert np.array_equal(compact_ids(ids), g["s_ids"][k]), f"tick {k}: reset ids"
        hit = ids >= 0
        resets += int(hit.sum())
        assert (commands[hit] >= lo).all() and (commands[hit] <= hi).all(), f"tick {k}: drawn commands outside their ranges"
        if before is not None:
            assert np.array_equal(commands[~hit], before[~hit]), f"tick {k}: begin touched the commands of an environment that is not reset"
        obs, rew, reset = finish(k, g["s_commands"][k])
        check_outputs(obs, rew, reset, g["s_obs"][k], g["s_rew"][k], g["s_reset"][k], float(g["s_gap_rot"]), float(g["s_gap_rew"]), float(g["clip"]), f"tick {k}")
    assert resets == int(g["s_cond_resets"]) >= n + 4


@pytest.mark.parametrize("robot", ROBOTS)
def test_sequence_matches_vec_task_step(shim, robot):
    g = gold(robot)
    assert g["s_cond_contact_margin"] >= 0.4 and g["s_cond_timeouts"] >= 2 and g["s_progress"].max() == g["s_max_len"] + 1
    cfg = sequence_config(seed=3)
    assert cfg.max_episode_length == int(g["s_max_len"]) == 40
    c = shim_config(cfg)
    n = g["s_progress"].shape[1]
    progress, reset, timeout = np.zeros(n, np.int64), np.ones(n, np.int64), np.zeros(n, np.int64)      # vec_task.py:240-246
    episode, ids, commands = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros((n, 3), np.float32)
    idx = (g["base_index"], g["knee_indices"], g["hip_indices"])

    def begin():
        shim.shim_begin(C.addressof(c), n, *(x.ctypes.data for x in (progress, reset, timeout, episode, ids, commands)))
        return progress.copy(), timeout.copy(), ids.copy(), commands.copy()

    def finish(k, cmd):
        commands[:] = cmd
        obs, rew, rs = host_finish(shim, cfg, g["s_root"][k], g["s_dof"][k], commands, g["s_actions"][k], g["s_torques"][k], progress, g["s_contact"][k], idx)
        reset[:] = rs
        return obs, rew, rs

    replay_sequence(g, cfg, begin, finish)
    assert (episode >= 1).all() and episode.sum() == int(g["s_cond_resets"])


def test_fell_mask_is_base_contact(shim):
    g = gold("aliengo")
    n = len(g["b_root"])
    cfg = batch_config()
    idx = (int(g["base_index"]), g["knee_indices"], g["hip_indices"])
    nrm = np.linalg.norm(g["b_contact"].astype(np.float64), axis=2)
    fell = nrm[:, idx[0]] > 1
    only_base = np.zeros_like(g["b_contact"])
    only_base[:, idx[0]] = g["b_contact"][:, idx[0]]
    args = (g["b_root"], g["b_dof"], g["b_commands"], g["b_actions"], g["b_torques"], g["b_episode"])
    a = host_finish(shim, cfg, *args, contact=only_base, idx=idx)
    b = host_finish(shim, cfg, *args, fell=fell)
    both = host_finish(shim, cfg, *args, contact=only_base, idx=idx, fell=fell)
    none = host_finish(shim, cfg, *args)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(a, both):
        assert np.array_equal(x, y)
    assert fell.sum() >= 8 and (a[2][fell] == 1).all() and np.array_equal(none[2].astype(bool), g["b_episode"] > g["b_max_len"])


def test_command_sampler(shim):
    cfg = R.TaskConfig(seed=11)
    c, c2 = shim_config(cfg), shim_config(R.TaskConfig(seed=12))
    lo, hi = np.array(c.cmd_lo[:]), np.array(c.cmd_hi[:])

    def draw(cc, env, ep):
        out = np.zeros(3, np.float32)
        shim.shim_sample(C.addressof(cc), env, ep, out.ctypes.data)
        return out
    base = draw(c, 5, 1)
    assert np.array_equal(base, draw(c, 5, 1))                                   # identical for equal (seed, env, episode)
    assert not np.array_equal(base, draw(c, 5, 2)) and not np.array_equal(base, draw(c, 6, 1)) and not np.array_equal(base, draw(c2, 5, 1))
    assert len({base[0], base[1] / hi[1] * hi[0], base[2]}) == 3                 # the three axes are three draws
    N = 100_000
    sd_mean, sd_var = np.sqrt(1 / 12 / N), np.sqrt((1 / 80 - 1 / 144) / N)       # of the mean and the variance of N uniform(0, 1) draws
    for axis in range(3):
        for shape in ((N, 1), (1, N), (317, 317)):                               # across environments, across episodes, both
            u = np.zeros(shape[0] * shape[1], np.float32)
            shim.shim_uniform(cfg.seed, 0, shape[0], 1, shape[1], axis, u.ctypes.data)
            u = u[:N].astype(np.float64)
            assert u.min() >= 0.0 and u.max() < 1.0
            assert abs(u.mean() - 0.5) <= 5 * sd_mean and abs(u.var() - 1 / 12) <= 5 * sd_var, (axis, shape, u.mean(), u.var())
            assert len(np.unique(u)) > 0.99 * N                                  # (24-bit values: ~0.3 % collide by chance)
    cmds = np.stack([draw(c, e, 1 + e % 7) for e in range(2000)])
    assert (cmds >= lo).all() and (cmds <= hi).all()
    span = cmds.max(0) - cmds.min(0)
    assert (span > 0.95 * (hi - lo)).all()
    fixed = R.TaskConfig(command_x_range=(0.5, 0.5), command_y_range=(0.0, 0.0), command_yaw_range=(-0.25, -0.25))
    assert np.array_equal(draw(shim_config(fixed), 9, 4), np.array([0.5, 0.0, -0.25], np.float32))


def test_task_config_restates_the_yaml():
    g = gold("aliengo")
    cfg = R.TaskConfig()
    assert cfg.max_episode_length == 2000 and cfg.clip_observations == float(g["clip"]) == 5.0 and cfg.clip_actions == 1.0 and cfg.dt == float(g["dt"])
    assert np.array_equal(np.array([cfg.command_x_range, cfg.command_y_range, cfg.command_yaw_range]), g["command_ranges"])
    assert np.array_equal(np.array(cfg.default_dof_pos, np.float32), g["default_dof_pos"])
    assert (cfg.lin_vel_scale, cfg.ang_vel_scale, cfg.dof_pos_scale, cfg.dof_vel_scale) == (1.0, 1.0, 1.0, 1.0)
    want = dict(lin_vel_xy=1.0 * 0.01, lin_vel_z=-4.0 * 0.01, ang_vel_xy=-0.05 * 0.01, ang_vel_z=0.5 * 0.01, torque=-0.000025 * 0.01, collision=0.0)
    assert cfg.reward_scales() == [want[k] for k in R.REWARD_TERMS]


def test_abi_symbols_and_argument_checks():
    names = sorted(set(re.findall(r"\b(mpc_task_[a-z_]+)\s*\(", open(HEADER).read())))
    assert names == sorted(R.SYMBOLS) and not set(names) & set(_lib.SYMBOLS)
    L = R.lib()
    for s in R.SYMBOLS:
        assert getattr(L, s).argtypes is not None, s
    h = C.c_void_p()
    good = R.TaskConfig()._struct()
    E_ARG = -1

    def bad(**kw):
        c = R.TaskConfig(**kw)._struct()
        return L.mpc_task_create(C.byref(h), 8, C.addressof(c))
    assert L.mpc_task_create(None, 8, C.addressof(good)) == E_ARG
    assert L.mpc_task_create(C.byref(h), 0, C.addressof(good)) == E_ARG
    assert L.mpc_task_create(C.byref(h), 8, None) == E_ARG
    assert bad(command_x_range=(1.0, -1.0)) == E_ARG and b"min > max" in L.mpc_task_last_error()
    assert bad(clip_observations=0.0) == E_ARG and b"clip_observations" in L.mpc_task_last_error()
    assert bad(episode_length_s=0.0) == E_ARG and b"max_episode_length" in L.mpc_task_last_error()
    assert bad(lin_vel_scale=float("nan")) == E_ARG and bad(rew_torque=float("inf")) == E_ARG
    assert not h.value                                                           # nothing was created
    assert L.mpc_task_begin(None, None) == E_ARG and L.mpc_task_buffers(None, None) == E_ARG
    assert L.mpc_task_finish(None, None, None, None, None, None, 0, 0, None, None, None, None) == E_ARG
    L.mpc_task_destroy(None)


def test_classes_raise_without_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from rl_mpc_locomotion_amd import BatchedRLTask, TaskPostPhysics
    with pytest.raises(_lib.MpcLibraryError):
        BatchedRLTask([0, 0], [0, 0])
    with pytest.raises(_lib.MpcLibraryError):
        TaskPostPhysics(2)


def test_kernels_compile_for_gfx950_without_scratch_or_buffer_access(tmp_path):
    out = tmp_path / "mpc_task.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "mpc_task.hip"),
                    "-o", str(out)], check=True)
    asm = out.read_text()
    for kernel in ("task_begin_kernel", "task_finish_kernel"):
        assert re.search(r"^_Z\w*%s\w*:" % kernel, asm, re.M), kernel
    assert len(re.findall(r"\.amdhsa_private_segment_fixed_size 0\b", asm)) == 2
    assert not re.search(r"^\s+(scratch_|buffer_)", asm, re.M)
