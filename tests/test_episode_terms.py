"""The per-term episode sums and the command curriculum on the CPU (csrc/episode_terms.h, csrc/mpc_episode_terms.h,
rl_mpc_locomotion_amd.episode_terms): the header compiled with g++ into a small shim.  reward_terms against rltask::reward_reset on the inputs of
tests/golden/rl_task_*.npz -- bit for bit, every sample, every contact variant --, the close / decide / resample chain against the restatement of
tests/episode_terms_ref.py -- sums, ticks, counts, ranges, window accumulators and commands EQUAL --, the decision's edges, the draws, the spec's
validation, the ABI's symbols and argument checks, and the kernels' scratch and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, curriculum, domain_rand, episode, episode_terms as E, height_scan, obs_norm, ppo as P, rl_task, terrain, toy_sim
from tests import episode_terms_ref as ref
from tests.helpers import ROOT
from tests.test_rl_task import ROBOTS, batch_config, gold, sequence_config, shim_config

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HEADER = os.path.join(CSRC, "mpc_episode_terms.h")
HIPCC = "/opt/rocm/bin/hipcc"
SIZES = (1, 63, 64, 65, 130)

SHIM = r"""
#include "episode_terms.h"
using namespace epterms;
using rltask::Config;
using rltask::Contacts;
extern "C" {
int shim_layout(int *out) {
  const int v[] = {kTerms, kBlock, kPartial, (int)kCommandAxis, kGlobRanges, kGlobWindow, kGlobWidenings, kGlobLen, kSumClosed, kSumTerms, kSumLo, kSumHi,
                   kSumWidenings, kSumEpisodeS, kSummaryLen, (int)sizeof(Curriculum)};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
  return (int)(sizeof(v) / sizeof(v[0]));
}
// the six terms, their clipped left-to-right sum, and what reward_reset returns on the same inputs
void shim_terms(const Config *c, int n, const float *root, const float *commands, const float *torques, const float *cf, int bodies, int base,
                const int *knee, const int *hip, const unsigned char *fell, float *terms, float *from_terms, float *rew) {
  for (int r = 0; r < n; ++r) {
    Contacts k{false, false, 0};
    if (cf) k = rltask::contacts_from_forces(cf + (long)r * 3 * bodies, base, knee, hip);
    if (fell) k.base = k.base || fell[r] != 0;
    reward_terms(*c, root + 13 * r, commands + 3 * r, torques + 12 * r, k, terms + kTerms * r);
    from_terms[r] = reward_from_terms(terms + kTerms * r);
    bool rs;
    rew[r] = rltask::reward_reset(*c, root + 13 * r, commands + 3 * r, torques + 12 * r, k, 0, rs);
  }
}
void shim_accumulate(int n, const float *terms, float *sums, int *ticks) {
  for (int r = 0; r < n; ++r) accumulate_env(terms + kTerms * r, sums + kTerms * r, ticks[r]);
}
// the three launches of close_and_resample, as the kernels make them
void shim_close_and_resample(int n, const int *ids, float *sums, int *ticks, int *counts, double *glob, float *commands, const Curriculum *k,
                             int resample, unsigned long long seed, int stage, double *S) {
  const int blocks = (n + kBlock - 1) / kBlock;
  double *partials = new double[(size_t)blocks * kPartial];
  for (int b = 0; b < blocks; ++b) {
    const int first = b * kBlock, count = n - first < kBlock ? n - first : kBlock;
    int closed[kBlock];
    for (int e = 0; e < count; ++e) closed[e] = ids[first + e] >= 0 && closes(ids[first + e], ticks[first + e], sums + (size_t)(first + e) * kTerms) ? 1 : 0;
    for (int j = 0; j < kPartial; ++j) partials[(size_t)b * kPartial + j] = block_partial_word(count, closed, sums + (size_t)first * kTerms, kTerms, j);
    for (int e = 0; e < count; ++e) {
      if (ids[first + e] < 0) continue;
      for (int i = 0; i < kTerms; ++i) sums[(size_t)(first + e) * kTerms + i] = 0.0f;
      ticks[first + e] = 0;
      counts[first + e] += 1;
    }
  }
  for (int j = 0; j < kPartial; ++j) {
    double acc = 0.0;
    for (int base = 0; base < blocks; base += stage) acc = join_word(acc, blocks - base < stage ? blocks - base : stage, partials + (size_t)base * kPartial, j);
    S[j] = acc;
  }
  delete[] partials;
  join_tail(*k, S, glob);
  if (resample)
    for (int r = 0; r < n; ++r)
      if (ids[r] >= 0) resample_env(seed, r, counts[r], glob + kGlobRanges, commands + 3 * r);
}
void shim_resample(unsigned long long seed, int env, int count, const double *ranges, float *out) { resample_env(seed, env, count, ranges, out); }
}
"""


class ShimCurriculum(C.Structure):     # epterms::Curriculum
    _fields_ = [("enabled", C.c_int), ("tick", C.c_longlong), ("update_every", C.c_longlong), ("max_episode_length", C.c_double), ("threshold", C.c_double),
                ("scale", C.c_double), ("step", C.c_double), ("max_curriculum", C.c_double)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("episode_terms_shim")
    src, so = d / "episode_terms_shim.cpp", d / "episode_terms_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    vp, ci, ull = C.c_void_p, C.c_int, C.c_ulonglong
    L.shim_layout.argtypes = [vp]
    L.shim_terms.argtypes, L.shim_terms.restype = [vp, ci] + [vp] * 4 + [ci, ci] + [vp] * 6, None
    L.shim_accumulate.argtypes, L.shim_accumulate.restype = [ci, vp, vp, vp], None
    L.shim_close_and_resample.argtypes, L.shim_close_and_resample.restype = [ci] + [vp] * 7 + [ci, ull, ci, vp], None
    L.shim_resample.argtypes, L.shim_resample.restype = [ull, ci, ci, vp, vp], None
    return L


def test_layouts_agree(shim):
    out = np.zeros(32, np.int32)
    k = shim.shim_layout(out.ctypes.data)
    assert out[:k].tolist() == [ref.TERMS, ref.BLOCK, 8, ref.COMMAND_AXIS, ref.G_RANGES, ref.G_WINDOW, ref.G_WIDENINGS, ref.STATE_LEN, E.S_CLOSED, E.S_TERMS,
                                E.S_LO, E.S_HI, E.S_WIDENINGS, E.S_EPISODE_S, E.SUMMARY_LEN, C.sizeof(ShimCurriculum)]
    assert (E.G_RANGES, E.G_WINDOW, E.G_WIDENINGS, E.STATE_LEN) == (ref.G_RANGES, ref.G_WINDOW, ref.G_WIDENINGS, ref.STATE_LEN)
    assert E.NUM_TERMS == ref.TERMS == len(rl_task.REWARD_TERMS) and rl_task.REWARD_TERMS[ref.LIN_VEL_XY] == "lin_vel_xy"


def host_terms(L, cfg, root, commands, torques, contact=None, idx=None, fell=None):
    n = len(root)
    c = shim_config(cfg)
    a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
    root, commands, torques = (a(x, np.float32) for x in (root, commands, torques))
    terms, from_terms, rew = np.zeros((n, 6), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    cf = bodies = base = knee = hip = None
    if contact is not None:
        cf = a(contact, np.float32)
        bodies, base, knee, hip = cf.shape[1], int(idx[0]), a(idx[1], np.int32), a(idx[2], np.int32)
    fl = None if fell is None else a(fell, np.uint8)
    p = lambda x: None if x is None else x.ctypes.data
    L.shim_terms(C.addressof(c), n, p(root), p(commands), p(torques), p(cf), bodies or 0, base or 0, p(knee), p(hip), p(fl), p(terms), p(from_terms), p(rew))
    return terms, from_terms, rew


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_terms_add_up_to_the_reward_bit_for_bit(shim, robot):
    g = gold(robot)
    idx = (g["base_index"], g["knee_indices"], g["hip_indices"])
    S = g["s_root"].shape
    cases = [(batch_config(), g["b_root"], g["b_commands"], g["b_torques"], g["b_contact"]),
             (sequence_config(seed=3), g["s_root"].reshape(-1, 13), g["s_commands"].reshape(-1, 3), g["s_torques"].reshape(-1, 12),
              g["s_contact"].reshape((S[0] * S[1],) + g["s_contact"].shape[2:]))]
    seen_clip = seen_positive = knees = 0
    for cfg, root, commands, torques, contact in cases:
        n = len(root)
        fell = np.linalg.norm(contact.astype(np.float64), axis=2)[:, int(idx[0])] > 1
        for variant in (dict(contact=contact, idx=idx), dict(fell=fell), dict(contact=contact, idx=idx, fell=fell), dict()):
            terms, from_terms, rew = host_terms(shim, cfg, root, commands, torques, **variant)
            assert from_terms.tobytes() == rew.tobytes(), (robot, sorted(variant))
            # the same sum in numpy float32, one rounding per addition
            total = terms[:, 0]
            for i in range(1, 6):
                total = (total + terms[:, i]).astype(np.float32)
            assert np.maximum(total, np.float32(0)).tobytes() == rew.tobytes()
            seen_clip += int((total < 0).sum())
            seen_positive += int((total > 0).sum())
            knees += int((terms[:, 5] != 0).sum())
            scales = np.array(cfg.reward_scales(), np.float32)
            assert (np.sign(terms) * np.sign(scales) >= 0).all()              # every term has its scale's sign (or is zero)
        assert n >= 100
    assert seen_clip > 0 and seen_positive > 0 and knees > 0               # the clip bites somewhere, and the collision term is exercised


def test_accumulate_is_one_float32_add_per_term_and_tick(shim):
    rng = np.random.default_rng(2)
    n = 70
    sums, ticks = np.zeros((n, 6), np.float32), np.zeros(n, np.int32)
    want = np.zeros((n, 6), np.float32)
    for k in range(40):
        terms = (rng.standard_normal((n, 6)) * 10.0 ** rng.integers(-5, 2, (n, 6))).astype(np.float32)
        shim.shim_accumulate(n, terms.ctypes.data, sums.ctypes.data, ticks.ctypes.data)
        want = (want + terms).astype(np.float32)
    assert sums.tobytes() == want.tobytes() and (ticks == 40).all()
    assert not np.array_equal(want, np.sum([0], dtype=np.float32))         # (something was summed)


SPEC = dict(update_every=1, max_episode_length=100, threshold=0.8, scale=0.01, step=0.5, max_curriculum=2.0)
RANGES = ((-2.5, 2.5), (-1.0, 1.0), (-0.75, 0.25))


def shim_spec(spec, tick, enabled=True):
    k = ShimCurriculum()
    if spec is None:
        k.enabled, k.tick, k.update_every = 0, tick, 1
        return k
    k.enabled, k.tick, k.update_every = int(enabled), tick, spec["update_every"]
    k.max_episode_length, k.threshold, k.scale = float(spec["max_episode_length"]), spec["threshold"], float(np.float32(spec["scale"]))
    k.step, k.max_curriculum = spec["step"], spec["max_curriculum"]
    return k


def host_chain(L, case, state, tick, spec, seed, enabled=True, stage=256):
    sums, ticks, counts, commands = (case[k].copy() for k in ("sums", "ticks", "counts", "commands"))
    state = state.copy()
    k = shim_spec(spec, tick, enabled)
    S = np.zeros(8)
    L.shim_close_and_resample(len(case["ids"]), case["ids"].ctypes.data, sums.ctypes.data, ticks.ctypes.data, counts.ctypes.data, state.ctypes.data,
                              commands.ctypes.data, C.addressof(k), int(spec is not None), seed, stage, S.ctypes.data)
    return sums, ticks, counts, state, commands, S[:7]


def equal(got, want, what):
    for g, w, name in zip(got, want, ("sums", "ticks", "counts", "state", "commands", "S")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", ref.PATTERNS)
def test_host_build_equals_the_restatement_on_the_crafted_batch(shim, n, pattern):
    seed = 777
    case = ref.crafted(n, pattern)
    marked = case["marked"]
    for spec, x0 in ((SPEC, (-0.5, 1.0)), (None, None)):
        state = ref.state0(RANGES, x0)
        state[ref.G_WINDOW:ref.G_WINDOW + 7] = np.arange(7) * 0.125 + 3.0     # a window that already holds something
        got = host_chain(shim, case, state, 5, spec, seed)
        want = ref.close_and_resample(case["ids"], case["sums"], case["ticks"], case["counts"], state, case["commands"], 5, spec, seed)
        equal(got, want, (n, pattern, spec is not None))
        sums, ticks, counts, new_state, commands, S = got
        closed = marked & (case["ticks"] > 0) & np.isfinite(case["sums"]).all(1)
        assert S[0] == closed.sum() and np.isfinite(S).all()
        if pattern == "mix" and n >= 63:
            assert (marked & (case["ticks"] > 0)).sum() > closed.sum()         # the episodes with a NaN or an infinite sum closed nothing
        # environments that are not marked keep their sentinels; marked ones are zeroed and counted
        assert (sums[~marked] == ref.SENTINEL_SUM).all() and (ticks[~marked] == ref.SENTINEL_TICKS).all() and (counts[~marked] == ref.SENTINEL_COUNT).all()
        assert (commands[~marked] == ref.SENTINEL_COMMAND).all()
        assert not sums[marked].any() and not ticks[marked].any() and np.array_equal(counts[marked], case["counts"][marked] + 1)
        if spec is None:
            assert (commands == ref.SENTINEL_COMMAND).all() and np.array_equal(new_state[:6], state[:6]) and new_state[ref.G_WIDENINGS] == 0
        else:
            rg = new_state[:6].reshape(3, 2).astype(np.float32)
            assert (commands[marked] >= rg[:, 0]).all() and (commands[marked] <= rg[:, 1]).all()
            assert np.array_equal(new_state[2:6], state[2:6])                  # the y and yaw ranges stay
        if pattern in ("nobody", "everybody_fresh"):
            assert S[0] == 0 and not S.any() and np.array_equal(new_state[ref.G_WINDOW:], state[ref.G_WINDOW:]) and np.array_equal(new_state[:2], state[:2])
        if pattern == "one_per_block":
            assert marked.sum() == -(-n // 64)
    # the order is the rule's: a plain float64 sum over all closed environments differs somewhere across the sizes, so EQUAL means something
    S = ref.reduce_closed(case["ids"], case["sums"], case["ticks"])
    if pattern == "everybody" and n == 130:
        other = case["sums"].astype(np.float64)[::-1].sum(0)
        assert not np.array_equal(other, S[1:])


def test_the_join_stages_do_not_change_the_sum(shim):
    n = 64 * 9 + 5
    case = ref.crafted(n, "mix")
    state = ref.state0(RANGES, (-0.5, 0.5))
    want = ref.close_and_resample(case["ids"], case["sums"], case["ticks"], case["counts"], state, case["commands"], 3, SPEC, 9)
    for stage in (1, 4, 256):
        equal(host_chain(shim, case, state, 3, SPEC, 9, stage=stage), want, stage)


def _one_closing(value, n=3):
    """n environments, environment 1 closing an episode whose tracking sum is `value`"""
    ids = np.array([-1, 1, -1][:n], np.int32)
    sums = np.zeros((n, 6), np.float32)
    sums[1, 0] = value
    return dict(ids=ids, sums=sums, ticks=np.array([4, 9, 4][:n], np.int32), counts=np.zeros(n, np.int32), commands=np.zeros((n, 3), np.float32))


def test_decision_edges(shim):
    seed = 1
    spec = dict(SPEC, update_every=10)
    bar = spec["threshold"] * float(np.float32(spec["scale"])) * spec["max_episode_length"]          # the tracking sum at which mean / length == threshold x scale
    above, below = np.float32(bar), np.float32(bar)
    while float(above) / spec["max_episode_length"] <= spec["threshold"] * float(np.float32(spec["scale"])):
        above = np.nextafter(above, np.float32(np.inf))
    while float(below) / spec["max_episode_length"] > spec["threshold"] * float(np.float32(spec["scale"])):
        below = np.nextafter(below, np.float32(-np.inf))
    assert np.nextafter(below, np.float32(np.inf)) == above                # one float32 ulp apart
    state = ref.state0(RANGES, (-0.5, 0.5))

    def run(case, tick, st=state, enabled=True, sp=spec):
        got = host_chain(shim, case, st, tick, sp, seed, enabled=enabled)
        equal(got, ref.close_and_resample(case["ids"], case["sums"], case["ticks"], case["counts"], st, case["commands"], tick, sp, seed, enabled=enabled),
              (tick, enabled))
        return got[3]
    st = run(_one_closing(above), 20)
    assert st[:2].tolist() == [-1.0, 1.0] and st[ref.G_WIDENINGS] == 1     # just above: widened
    st = run(_one_closing(below), 20)
    assert st[:2].tolist() == [-0.5, 0.5] and st[ref.G_WIDENINGS] == 0     # just below (and exactly at the bar): not
    nothing = _one_closing(above)
    nothing["ticks"][1] = 0                                                # marked, but its sums hold no tick: nothing closed
    st = run(nothing, 20)
    assert st[:2].tolist() == [-0.5, 0.5] and st[ref.G_WINDOW] == 0
    nobody = _one_closing(above)
    nobody["ids"][:] = -1
    assert run(nobody, 20)[:2].tolist() == [-0.5, 0.5]
    st = run(_one_closing(above), 21)                                      # tick % update_every != 0: closed and counted, not decided
    assert st[:2].tolist() == [-0.5, 0.5] and st[ref.G_WINDOW] == 1 and st[ref.G_WINDOW + 1] == float(above)
    st = run(_one_closing(above), 20, enabled=False)                       # curriculum_enabled = False: the same
    assert st[:2].tolist() == [-0.5, 0.5] and st[ref.G_WINDOW] == 1
    # repeated widenings saturate at +-max_curriculum (2.0), each side on its own
    st = ref.state0(RANGES, (-0.5, 1.0))
    seen = []
    for k in range(6):
        st = run(_one_closing(above), 10 * k, st=st)
        seen.append(st[:2].tolist())
    assert seen == [[-1.0, 1.5], [-1.5, 2.0], [-2.0, 2.0], [-2.0, 2.0], [-2.0, 2.0], [-2.0, 2.0]] and st[ref.G_WIDENINGS] == 6
    assert st[ref.G_WINDOW] == 6 and st[ref.G_WINDOW + 1] == 6 * float(above)
    # a step that is no multiple of the room left: clipped, not overshot
    st = run(_one_closing(above), 0, st=ref.state0(RANGES, (-1.8, 0.0)), sp=dict(spec, step=0.3))
    assert st[:2].tolist() == [-2.0, 0.3]


def test_draws_do_not_depend_on_who_else_resets(shim):
    n, seed = 130, 31
    base = ref.crafted(n, "everybody")
    state = ref.state0(RANGES, (-1.0, 1.0))
    spec = dict(SPEC, threshold=1e9)                                       # never widens: the ranges are the same in both runs
    everybody = host_chain(shim, base, state, 1, spec, seed)[4]
    alone = {k: v.copy() for k, v in base.items()}
    keep = np.zeros(n, bool)
    keep[[0, 63, 64, 129]] = True
    alone["ids"] = np.where(keep, np.arange(n), -1).astype(np.int32)
    few = host_chain(shim, alone, state, 1, spec, seed)[4]
    assert np.array_equal(few[keep], everybody[keep]) and (few[~keep] == ref.SENTINEL_COMMAND).all()
    assert len(np.unique(everybody[:, 0])) > 100                           # environments draw different commands,
    again = {k: v.copy() for k, v in base.items()}
    again["counts"] = base["counts"] + 1
    assert not np.array_equal(host_chain(shim, again, state, 1, spec, seed)[4], everybody)        # and a later resample another one
    for r in (0, 64, 129):
        assert np.array_equal(everybody[r], ref.resample(seed, r, int(base["counts"][r]) + 1, state[:6].reshape(3, 2)))


def test_commands_lie_inside_the_ranges_hi_included(shim):
    out = np.zeros(3, np.float32)
    ranges = np.array([[-0.3, 0.7], [0.1, 0.1], [-1e-3, 2.5]])
    lo, hi = ranges.astype(np.float32).T
    draws = []
    for env in range(60):
        for count in range(1, 60):
            shim.shim_resample(5, env, count, ranges.ctypes.data, out.ctypes.data)
            assert np.array_equal(out, ref.resample(5, env, count, ranges))
            draws.append(out.copy())
    draws = np.array(draws)
    assert (draws >= lo).all() and (draws <= hi).all() and (draws[:, 1] == hi[1]).all()
    span = hi - lo
    assert (draws[:, 0].min() < lo[0] + 0.01 * span[0]) and (draws[:, 0].max() > hi[0] - 0.01 * span[0])       # the whole range is used
    # the fminf: lo + (hi - lo) u can round above hi for u just below 1; such a range exists and the result is hi, never beyond
    f = np.float32
    u = f(16777215.0) * f(1.0 / 16777216.0)
    hit = [(a, b) for a, b in ((f(-0.3), f(0.7)), (f(0.1), f(0.3)), (f(-1.7), f(0.9)), (f(1e-3), f(2.5)), (f(-2.5), f(2.5))) if f(a + f(f(b - a) * u)) > b]
    for a, b in hit:
        assert min(f(a + f(f(b - a) * u)), b) == b
    # the three axes are streams of their own, and none is a stream sample_commands or the terrain curriculum uses
    from tests.curriculum_ref import uniform01
    u = np.array([[float(uniform01(3, e, 1, a)) for e in range(200)] for a in range(7)])
    assert all(not np.array_equal(u[a], u[b]) for a in range(7) for b in range(a))


def test_spec_validation_is_host_side():
    cfg = rl_task.TaskConfig(episode_length_s=2.0)
    assert E.CommandCurriculumSpec(2.5).resolved(cfg) == (-2.5, 2.5, 200)
    assert E.CommandCurriculumSpec(1.5, x_range0=(-0.5, 0.5), update_every=1).resolved(cfg) == (-0.5, 0.5, 1)
    assert E.CommandCurriculumSpec(1.0, x_range0=(0.0, 1.0)).resolved(cfg)[:2] == (0.0, 1.0)
    for kw, text in ((dict(max_curriculum=2.0), "max_curriculum"), (dict(max_curriculum=1.0, x_range0=(0.2, 0.5)), "lo <= 0 <= hi"),
                     (dict(max_curriculum=1.0, x_range0=(-0.5, -0.1)), "lo <= 0 <= hi"), (dict(max_curriculum=0.4, x_range0=(-0.5, 0.3)), "max_curriculum"),
                     (dict(max_curriculum=1.0, x_range0=(-0.5, 0.5), step=0.0), "step"), (dict(max_curriculum=1.0, x_range0=(-0.5, 0.5), step=-0.5), "step"),
                     (dict(max_curriculum=float("nan"), x_range0=(-0.5, 0.5)), "finite"), (dict(max_curriculum=1.0, x_range0=(-0.5, 0.5), update_every=0), "update_every"),
                     (dict(max_curriculum=1.0, x_range0=(-0.5, 0.5, 0.1)), "x_range0")):
        with pytest.raises(ValueError, match=text):
            E.CommandCurriculumSpec(**kw).resolved(cfg)
    # EpisodeTerms validates the spec before it asks for a device
    with pytest.raises(ValueError, match="max_curriculum"):
        E.EpisodeTerms(8, cfg, command_curriculum=E.CommandCurriculumSpec(0.1))
    with pytest.raises(ValueError, match="n must"):
        E.EpisodeTerms(0, cfg)


def test_record_of_a_summary():
    values = [4.0, 8.0, -2.0, 0.0, 1.0, -0.5, 0.0, -1.0, 1.5, 3.0, 2.0]
    assert E.EpisodeTerms.record(values) == {"rew_lin_vel_xy": 1.0, "rew_lin_vel_z": -0.25, "rew_ang_vel_xy": 0.0, "rew_ang_vel_z": 0.125, "rew_torque": -0.0625,
                                             "rew_collision": 0.0, "max_command_x": 1.5, "min_command_x": -1.0, "command_widenings": 3}
    empty = E.EpisodeTerms.record([0.0] * 7 + [-0.5, 0.5, 0.0, 20.0])
    assert all(empty["rew_" + t] == 0.0 for t in rl_task.REWARD_TERMS) and empty["max_command_x"] == 0.5
    state = ref.state0(RANGES, (-1.0, 1.5))
    state[ref.G_WINDOW:ref.G_WINDOW + 7], state[ref.G_WIDENINGS] = values[:7], 3
    assert ref.summary(state, 2.0).tolist() == values


def test_abi_symbols_are_the_headers_and_nobody_elses():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(E.SYMBOLS) and len(names) == 8
    others = (set(_lib.SYMBOLS) | set(P.SYMBOLS) | set(P.UPDATE_SYMBOLS) | set(rl_task.SYMBOLS) | set(toy_sim.SYMBOLS) | set(terrain.SYMBOLS)
              | set(episode.SYMBOLS) | set(obs_norm.SYMBOLS) | set(curriculum.SYMBOLS) | set(height_scan.SYMBOLS) | set(domain_rand.SYMBOLS))
    assert not set(names) & others
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        assert "mpc_episode_terms_" not in open(os.path.join(ROOT, "include", h)).read(), h
    protos = re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(mpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert sorted(p[1] for p in protos) == names
    raw = C.CDLL(_lib.LIB_PATH)
    L = E.lib()
    for ret, name, params in protos:
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert len(f.argtypes) == (0 if params.strip() in ("", "void") else params.count(",") + 1), name
        assert (f.restype is None) == (" ".join(ret.split()) == "void"), name
    assert "episode_terms" in re.search(r"^UOBJS\s*:=.*$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(0)
    assert re.search(r"MPC_EPISODE_TERMS_SUMMARY = (\d+), MPC_EPISODE_TERMS_STATE = (\d+)", text).groups() == (str(E.SUMMARY_LEN), str(E.STATE_LEN))


def test_bad_arguments_are_refused_without_a_gpu():
    L = E.lib()
    E_ARG = -1
    h = C.c_void_p()
    good = rl_task.TaskConfig()._struct()

    def create(out=C.byref(h), n=4, cfg=good, ep=20.0, cur=1, lo=-0.5, hi=0.5, step=0.5, thr=0.8, mx=1.5, every=100):
        return L.mpc_episode_terms_create(out, n, None if cfg is None else C.addressof(cfg), ep, cur, lo, hi, step, thr, mx, every)

    nan_scale = rl_task.TaskConfig()._struct(); nan_scale.rew_scale[2] = float("nan")
    swapped = rl_task.TaskConfig()._struct(); swapped.command_range[1][0], swapped.command_range[1][1] = 1.0, -1.0
    no_len = rl_task.TaskConfig()._struct(); no_len.max_episode_length = 0
    for kw, text in (({"out": None}, b"null"), ({"cfg": None}, b"null"), ({"n": 0}, b"n must"), ({"n": -3}, b"n must"), ({"cfg": nan_scale}, b"not finite"),
                     ({"cfg": swapped}, b"min > max"), ({"cfg": no_len}, b"max_episode_length"), ({"ep": 0.0}, b"episode_length_s"),
                     ({"ep": float("nan")}, b"episode_length_s"), ({"ep": float("inf")}, b"episode_length_s"), ({"lo": 0.1}, b"lo <= 0 <= hi"),
                     ({"hi": -0.1}, b"lo <= 0 <= hi"), ({"lo": float("nan")}, b"lo <= 0 <= hi"), ({"mx": 0.4}, b"max_curriculum"),
                     ({"mx": float("inf")}, b"max_curriculum"), ({"step": 0.0}, b"step"), ({"step": float("nan")}, b"step"), ({"thr": float("nan")}, b"threshold"),
                     ({"every": 0}, b"update_every")):
        assert create(**kw) == E_ARG, kw
        msg = L.mpc_episode_terms_last_error()
        assert b"mpc_episode_terms_create" in msg and text in msg, (kw, msg)
    assert not h.value
    p = 0x1000
    assert L.mpc_episode_terms_close_and_resample(None, p, p, 0, 1, None) == E_ARG and b"null" in L.mpc_episode_terms_last_error()
    assert L.mpc_episode_terms_accumulate(None, p, p, p, p, p, None) == E_ARG and L.mpc_episode_terms_summary(None, p, None) == E_ARG
    assert L.mpc_episode_terms_new_window(None, None) == E_ARG and L.mpc_episode_terms_arrays(None, *[C.byref(C.c_void_p()) for _ in range(4)]) == E_ARG
    L.mpc_episode_terms_destroy(None)


def test_classes_raise_without_a_gpu_and_the_task_refuses_another_size(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.MpcLibraryError):
        E.EpisodeTerms(8)
    with pytest.raises(_lib.MpcLibraryError):
        rl_mpc_locomotion_amd.EpisodeTerms(8, command_curriculum=rl_mpc_locomotion_amd.CommandCurriculumSpec(2.5))

    class Fake:                                                            # (the argument check comes before anything touches the device)
        n = 8
    with pytest.raises(ValueError, match="episode terms hold 8"):
        rl_task.BatchedRLTask([0] * 4, [0] * 4, episode_terms=Fake())
    with pytest.raises(_lib.MpcLibraryError):
        rl_task.BatchedRLTask([0] * 8, [0] * 8, episode_terms=Fake())


def test_kernels_compile_for_gfx950_without_scratch_and_with_the_staging_as_the_only_lds(tmp_path):
    out = tmp_path / "mpc_episode_terms.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "mpc_episode_terms.hip"), "-o", str(out)], check=True, capture_output=True, text=True)
    found = {}
    for name, scratch, lds in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S):
        found[name] = (int(scratch), int(lds))
    close = 64 * 7 * 4 + 64 * 4                                            # a wave's float32 sums in rows of 7 words, and its closed flags
    join = 256 * 8 * 8 + 8 * 8                                             # 256 staged partial rows, and the joined row
    for kernel, want in (("terms_close_kernel", (0, close)), ("terms_join_kernel", (0, join)), ("terms_resample_kernel", (0, 0)),
                         ("terms_accumulate_kernel", (0, 0)), ("terms_summary_kernel", (0, 0))):
        hit = [v for k, v in found.items() if kernel in k]
        assert hit == [want], (kernel, found)
    assert len(found) == 5
