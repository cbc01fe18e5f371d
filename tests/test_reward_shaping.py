"""The reward shaping terms on the CPU (csrc/reward_shaping.h, csrc/mpc_reward_shaping.h, rl_mpc_locomotion_amd.reward_shaping): the header compiled
with g++ into a small shim and compared with the restatement of tests/reward_shaping_ref.py -- terms, reward, history, sums, ticks, close and window
EQUAL --, the crafted rows one by one, the spec's validation, the ABI's symbols and argument checks, the task's refusals, the trainer's rider, a
sanitized stand-alone program, and the kernels' registers, scratch and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, episode_terms, privileged_obs, reward_shaping as RS, rl_task, toy_sim
from tests import reward_shaping_ref as ref
from tests.helpers import ROOT
from tests.reward_shaping_ref import F, same
from tests.test_rl_task import shim_config

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HEADER = os.path.join(CSRC, "mpc_reward_shaping.h")
HIPCC = "/opt/rocm/bin/hipcc"
GXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC]
CFG = rl_task.TaskConfig(episode_length_s=ref.MAX_EPISODE_LENGTH * ref.DT, dt=ref.DT, rew_collision=-0.25)
TARGET_H, TARGET_AIR = 0.31, 0.5

SHIM = r"""
#include "reward_shaping.h"
using namespace rshape;
using rltask::Config;
extern "C" {
int shim_layout(int *out) {
  const int v[] = {kTerms, kBlock, kPartial, kWords, kLanes, kMaxPoints, kSumClosed, kSumTerms, kSumEpisodeS, kSummaryLen, (int)sizeof(Spec), (int)sizeof(Env),
                   kOrientation, kBaseHeight, kDofVel, kDofAcc, kActionRate, kFeetAirTime, kStandStill, kTermination, epterms::kPartial, epterms::kTerms};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
  return (int)(sizeof(v) / sizeof(v[0]));
}
// one tick of n environments as the run kernel makes it; state arrays as the C ABI's.  task6 [n][6] receives rltask::reward_terms, from6 [n] their
// clipped sum by rltask::reward_from_terms
void shim_run(const Config *c, const Spec *k, int n, const float *root, const float *dof, const float *actions, const float *commands, const float *torques,
              const unsigned char *fell, const int *ids, const long long *reset, const long long *progress, const int *contact, const float *heights, int P,
              float *last_actions, float *last_dof_vel, float *air_time, int *last_contact, float *sums, int *ticks, float *rew, float *terms, float *task6,
              float *from6) {
  for (int r = 0; r < n; ++r) {
    Env env;
    for (int i = 0; i < kDof; ++i) { env.last_actions[i] = last_actions[r * kDof + i]; env.last_dof_vel[i] = last_dof_vel[r * kDof + i]; }
    for (int l = 0; l < kLegs; ++l) { env.air_time[l] = air_time[r * kLegs + l]; env.last_contact[l] = last_contact[r * kLegs + l]; }
    for (int i = 0; i < kTerms; ++i) env.sums[i] = sums[r * kTerms + i];
    env.ticks = ticks[r];
    float t[kTaskTerms], e[kTerms];
    rltask::reward_terms(*c, root + 13 * r, commands + 3 * r, torques + 12 * r, rltask::contacts_from_fell(fell && fell[r] != 0), t);
    const float hbar = k->scale[kBaseHeight] != 0.0f ? height_mean(root[13 * r + 2], heights ? heights + (size_t)r * P : nullptr, P) : 0.0f;
    tick_terms(*c, *k, root + 13 * r, dof + 24 * r, actions + 12 * r, commands + 3 * r, ids[r], reset[r], progress[r], contact + 4 * r, hbar, env, e);
    rew[r] = reward_from(*k, t, e);
    accumulate_env(e, env.sums, env.ticks);
    for (int i = 0; i < kDof; ++i) { last_actions[r * kDof + i] = env.last_actions[i]; last_dof_vel[r * kDof + i] = env.last_dof_vel[i]; }
    for (int l = 0; l < kLegs; ++l) { air_time[r * kLegs + l] = env.air_time[l]; last_contact[r * kLegs + l] = env.last_contact[l]; }
    for (int i = 0; i < kTerms; ++i) { sums[r * kTerms + i] = env.sums[i]; terms[r * kTerms + i] = e[i]; }
    ticks[r] = env.ticks;
    for (int i = 0; i < kTaskTerms; ++i) task6[r * kTaskTerms + i] = t[i];
    from6[r] = rltask::reward_from_terms(t);
  }
}
// the two launches of mpc_shaping_close, as the kernels make them: `stage` block partials per pass of the join
void shim_close(int n, const int *ids, float *sums, int *ticks, double *window, int stage, double *S) {
  const int blocks = (n + kBlock - 1) / kBlock;
  double *partials = new double[(size_t)blocks * kPartial];
  for (int b = 0; b < blocks; ++b) {
    const int first = b * kBlock, count = n - first < kBlock ? n - first : kBlock;
    int closed[kBlock];
    for (int e = 0; e < count; ++e) closed[e] = closes(ids[first + e], ticks[first + e], sums + (size_t)(first + e) * kTerms) ? 1 : 0;
    for (int j = 0; j < kPartial; ++j) partials[(size_t)b * kPartial + j] = block_partial_word(count, closed, sums + (size_t)first * kTerms, kTerms, j);
    for (int e = 0; e < count; ++e) {
      if (ids[first + e] < 0) continue;
      for (int i = 0; i < kTerms; ++i) sums[(size_t)(first + e) * kTerms + i] = 0.0f;
      ticks[first + e] = 0;
    }
  }
  for (int j = 0; j < kWords; ++j) {
    double acc = 0.0;
    for (int base = 0; base < blocks; base += stage) acc = join_word(acc, blocks - base < stage ? blocks - base : stage, partials + (size_t)base * kPartial, j);
    S[j] = acc;
    window[j] = window[j] + acc;
  }
  delete[] partials;
}
float shim_height_mean(float root_z, const float *heights, int P) { return height_mean(root_z, heights, P); }
// episode_terms.h's own six-term words through the generalised forms: what tests/test_episode_terms.py's shim keeps getting
double shim_epterms_partial(int count, const int *closed, const float *sums, int stride, int j) { return epterms::block_partial_word(count, closed, sums, stride, j); }
double shim_epterms_join(double acc, int blocks, const double *partials, int j) { return epterms::join_word(acc, blocks, partials, j); }
}
"""

# the stand-alone program of the sanitizer run: chained ticks from a file into heap blocks of exactly their sizes, the results to a file
MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
template <class T> static std::vector<T> take(FILE *f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "short read\n"); exit(3); }
  return v;
}
template <class T> static void put(FILE *o, const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), o); }
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int runs = take<int>(f, 1)[0];
  for (int run = 0; run < runs; ++run) {
    const std::vector<int> q = take<int>(f, 3);                                 // n, P, ticks
    const int n = q[0], P = q[1], ticks = q[2];
    const std::vector<Config> c = take<Config>(f, 1);
    const std::vector<Spec> k = take<Spec>(f, 1);
    std::vector<float> la((size_t)n * 12, 0.0f), lv((size_t)n * 12, 0.0f), air((size_t)n * 4, 0.0f), sums((size_t)n * 8, 0.0f);
    std::vector<int> lc((size_t)n * 4, 0), tk((size_t)n, 0);
    std::vector<double> window(kWords, 0.0), S(kWords, 0.0);
    for (int t = 0; t < ticks; ++t) {
      const std::vector<int> ids = take<int>(f, n);
      const std::vector<float> root = take<float>(f, (size_t)n * 13), dof = take<float>(f, (size_t)n * 24), actions = take<float>(f, (size_t)n * 12),
                               commands = take<float>(f, (size_t)n * 3), torques = take<float>(f, (size_t)n * 12);
      const std::vector<unsigned char> fell = take<unsigned char>(f, n);
      const std::vector<long long> reset = take<long long>(f, n), progress = take<long long>(f, n);
      const std::vector<int> contact = take<int>(f, (size_t)n * 4);
      const std::vector<float> heights = take<float>(f, (size_t)n * P);
      std::vector<float> rew(n), terms((size_t)n * 8), task6((size_t)n * 6), from6(n);
      shim_close(n, ids.data(), sums.data(), tk.data(), window.data(), 256, S.data());
      shim_run(c.data(), k.data(), n, root.data(), dof.data(), actions.data(), commands.data(), torques.data(), fell.data(), ids.data(), reset.data(),
               progress.data(), contact.data(), P ? heights.data() : nullptr, P, la.data(), lv.data(), air.data(), lc.data(), sums.data(), tk.data(),
               rew.data(), terms.data(), task6.data(), from6.data());
      put(o, rew); put(o, terms);
    }
    put(o, la); put(o, lv); put(o, air); put(o, lc); put(o, sums); put(o, tk); put(o, window);
  }
  fclose(f);
  fclose(o);
  return 0;
}
"""


class ShimSpec(C.Structure):           # rshape::Spec
    _fields_ = [("scale", C.c_float * 8), ("base_height_target", C.c_float), ("air_time_target", C.c_float), ("dt", C.c_float)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("reward_shaping_shim")
    src, so = d / "reward_shaping_shim.cpp", d / "reward_shaping_shim.so"
    src.write_text(SHIM)
    subprocess.run(GXX + ["-fPIC", "-shared", str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    vp, ci, cf, cd = C.c_void_p, C.c_int, C.c_float, C.c_double
    L.shim_layout.argtypes = [vp]
    L.shim_run.argtypes, L.shim_run.restype = [vp, vp, ci] + [vp] * 11 + [ci] + [vp] * 10, None
    L.shim_close.argtypes, L.shim_close.restype = [ci, vp, vp, vp, vp, ci, vp], None
    L.shim_height_mean.argtypes, L.shim_height_mean.restype = [cf, vp, ci], cf
    L.shim_epterms_partial.argtypes, L.shim_epterms_partial.restype = [ci, vp, vp, ci, ci], cd
    L.shim_epterms_join.argtypes, L.shim_epterms_join.restype = [cd, ci, vp, ci], cd
    return L


def shim_spec(per_second, target_h=TARGET_H, target_air=TARGET_AIR, dt=ref.DT):
    k = ShimSpec()
    k.scale[:] = [float(v) for v in ref.scales_of(per_second, dt)]
    k.base_height_target, k.air_time_target, k.dt = target_h, target_air, dt
    return k


class Host:
    """The header's state and its two calls through the shim, shaped like ref.Shaping."""

    def __init__(self, L, n, per_second, cfg=CFG, **spec):
        self.L, self.n, self.c, self.k = L, n, shim_config(cfg), shim_spec(per_second, **spec)
        self.last_actions, self.last_dof_vel = np.zeros((n, 12), F), np.zeros((n, 12), F)
        self.air_time, self.last_contact = np.zeros((n, 4), F), np.zeros((n, 4), np.int32)
        self.sums, self.ticks, self.window = np.zeros((n, 8), F), np.zeros(n, np.int32), np.zeros(9)

    state = ref.Shaping.state

    def close(self, ids, stage=256):
        S = np.zeros(9)
        self.L.shim_close(self.n, ids.ctypes.data, self.sums.ctypes.data, self.ticks.ctypes.data, self.window.ctypes.data, stage, S.ctypes.data)
        return S

    def run(self, b, ids):
        """(e, rew, task6, from6) of one tick on the batch b"""
        n = self.n
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        root, dof, actions, commands, torques = (a(b[k], F) for k in ("root", "dof", "actions", "commands", "torques"))
        fell, reset, progress, contact = a(b["fell"], np.uint8), a(b["reset"], np.int64), a(b["progress"], np.int64), a(b["contact"], np.int32)
        heights = None if b["heights"] is None else a(b["heights"], F)
        rew, terms, task6, from6 = np.zeros(n, F), np.zeros((n, 8), F), np.zeros((n, 6), F), np.zeros(n, F)
        self.L.shim_run(C.addressof(self.c), C.addressof(self.k), n, root.ctypes.data, dof.ctypes.data, actions.ctypes.data, commands.ctypes.data, torques.ctypes.data,
                        fell.ctypes.data, ids.ctypes.data, reset.ctypes.data, progress.ctypes.data, contact.ctypes.data, None if heights is None else heights.ctypes.data,
                        0 if heights is None else heights.shape[1], self.last_actions.ctypes.data, self.last_dof_vel.ctypes.data, self.air_time.ctypes.data,
                        self.last_contact.ctypes.data, self.sums.ctypes.data, self.ticks.ctypes.data, rew.ctypes.data, terms.ctypes.data, task6.ctypes.data,
                        from6.ctypes.data)
        return terms, rew, task6, from6


def restatement(n, per_second, cfg=CFG, target_h=TARGET_H, target_air=TARGET_AIR):
    return ref.Shaping(n, ref.scales_of(per_second, cfg.dt), target_h, target_air, cfg.dt, cfg.default_dof_pos, cfg.max_episode_length)


def chain(n, P, seed, ticks=6, maker=ref.crafted_tick):
    """`ticks` chained ticks: (ids, batch) each; every environment is marked on the first (the task's first tick resets all), some on the third and
    the fifth."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(ticks):
        ids = ref.marks(n, "all" if t == 0 else "some" if t in (2, 4) else "none")
        out.append((ids, (maker if t % 2 == 0 else ref.random_tick)(n, P, rng, t)))
    return out


def assert_states_equal(host, want, what):
    for name, w in want.state().items():
        g = host.state()[name]
        assert same(g, w), (what, name)


def run_chain(host, want, ticks, what):
    """Both through the same ticks; everything EQUAL after each; returns the per-tick (e, rew, marked, batch)."""
    seen = []
    for t, (ids, b) in enumerate(ticks):
        S, S_want = host.close(ids), want.close(ids)
        assert S.tobytes() == S_want.tobytes(), (what, t, "S")
        e, rew, task6, from6 = host.run(b, ids)
        e_want, rew_want = want.run(b["root"], b["dof"], b["actions"], b["commands"], ids, b["reset"], b["progress"], b["contact"], b["heights"], task6)
        assert same(e, e_want), (what, t, "terms", np.argwhere(~(e == e_want)))
        assert same(rew, rew_want), (what, t, "rew")
        assert_states_equal(host, want, (what, t))
        seen.append((e, rew, ids >= 0, b, task6, from6))
    return seen


def test_layouts_agree(shim):
    out = np.zeros(32, np.int32)
    k = shim.shim_layout(out.ctypes.data)
    assert out[:k].tolist() == [8, ref.BLOCK, 16, ref.WINDOW_LEN, ref.LANES, RS.MAX_POINTS, RS.S_CLOSED, RS.S_TERMS, RS.S_EPISODE_S, RS.SUMMARY_LEN, C.sizeof(ShimSpec),
                                (12 + 12 + 4 + 4 + 8 + 1) * 4, *range(8), 8, 6]
    assert RS.SHAPING_TERMS == ref.TERMS == ("orientation", "base_height", "dof_vel", "dof_acc", "action_rate", "feet_air_time", "stand_still", "termination")
    assert RS.NUM_TERMS == 8 and RS.WINDOW_LEN == ref.WINDOW_LEN and len(rl_task.REWARD_TERMS) == 6 and len(rl_task.STAGES) == 13


@pytest.mark.parametrize("n,P", [(65, P) for P in ref.POINTS] + [(n, 187) for n in ref.SIZES if n != 65] + [(130, 0)])
def test_six_chained_ticks_equal_the_restatement(shim, n, P):
    host, want = Host(shim, n, ref.ALL_ON), restatement(n, ref.ALL_ON)
    seen = run_chain(host, want, chain(n, P, 100 * n + P), (n, P))
    e = np.stack([s[0] for s in seen])
    marked = np.stack([s[2] for s in seen])
    assert (e[marked][:, [ref.DOF_ACC, ref.ACTION_RATE, ref.FEET_AIR_TIME]] == 0).all()               # a reset tick pays none of the history's terms
    assert (host.ticks == np.where(ref.marks(n, "some") >= 0, 2, 6)).all()
    if n >= 63:
        for i, name in enumerate(ref.TERMS):
            assert (e[:, :, i] != 0).any(), name                                                       # every term is exercised,
        assert (e[~marked][:, ref.DOF_ACC] != 0).all() and host.window[0] == 2 * (ref.marks(n, "some") >= 0).sum()       # and the episodes closed twice
        rew = np.stack([s[1] for s in seen])
        assert (rew > 0).any() and (rew < 0).any()                                                     # the clip bites, and termination reaches below it


def test_command_norms_on_both_sides_of_a_tenth(shim):
    n = 24
    rng = np.random.default_rng(4)
    b = ref.crafted_tick(n, 0, rng)
    mv = ref.moving(b["commands"])
    case = np.arange(n) % 12
    assert not mv[case == 0].any() and mv[case == 2].all() and mv[case == 3].all() and not mv[case == 4].any()
    at = b["commands"][case == 1]
    assert (at[:, 0] == F(0.1)).all() and (mv[case == 1] == (np.sqrt(at[:, 0] * at[:, 0]) > F(0.1))).all()      # at the float32 nearest 0.1: whatever sqrtf gives
    host, want = Host(shim, n, ref.ALL_ON), restatement(n, ref.ALL_ON)
    ids = ref.marks(n, "none")
    for k, contact in enumerate((np.zeros((n, 4), np.int32), np.ones((n, 4), np.int32))):      # all feet up, then all down: the second tick sees them land
        (e, rew, marked, _, _, _), = run_chain(host, want, [(ids, dict(b, contact=contact))], k)
    assert (e[~mv, ref.FEET_AIR_TIME] == 0).all() and (e[mv, ref.FEET_AIR_TIME] != 0).all()
    assert (e[mv, ref.STAND_STILL] == 0).all() and (e[~mv, ref.STAND_STILL] != 0).all()


def test_a_foot_that_lands_above_and_below_the_target(shim):
    seq = ref.landing_sequence(TARGET_AIR)
    host, want = Host(shim, 1, ref.ALL_ON), restatement(1, ref.ALL_ON)
    rng = np.random.default_rng(9)
    paid = []
    for t, contact in enumerate(seq):
        b = ref.random_tick(1, 0, rng)
        b["commands"][:] = (0.5, 0.0, 0.0)
        b["contact"] = contact[None].copy()
        (e, _, _, _, _, _), = run_chain(host, want, [(ref.marks(1, "all" if t == 0 else "none"), b)], t)
        paid.append(float(e[0, ref.FEET_AIR_TIME]))
    paid = np.array(paid)
    scale = float(ref.scales_of(ref.ALL_ON, ref.DT)[ref.FEET_AIR_TIME])
    landings = np.flatnonzero(paid)
    assert len(landings) == 2 and paid[landings[0]] < 0 < paid[landings[1]]     # the short flight first (below the target), the long one later (above)
    short, long_ = landings - 2                 # dt's in air_time when the landing is seen: the lift-off tick still has last_contact set and counts nothing
    for ticks_up, got in ((short, paid[landings[0]]), (long_, paid[landings[1]])):
        air = F(0)
        for _ in range(ticks_up):
            air = F(air + F(ref.DT))
        assert got == float(F(F(air - F(TARGET_AIR)) * F(scale)))
    assert host.air_time[0, 3] > 0 and host.air_time[0, 2] == 0 and host.air_time[0, 0] == 0        # the foot that never lands keeps counting


def test_termination_is_a_fall_and_not_a_time_out(shim):
    n = 24
    b = ref.crafted_tick(n, 0, np.random.default_rng(5))
    host, want = Host(shim, n, ref.ALL_ON), restatement(n, ref.ALL_ON)
    (e, rew, _, _, _, _), = run_chain(host, want, [(ref.marks(n, "all"), b)], 0)
    case = np.arange(n) % 12
    scale = ref.scales_of(ref.ALL_ON, ref.DT)[ref.TERMINATION]
    assert (e[case == 5, ref.TERMINATION] == 0).all() and (e[case == 7, ref.TERMINATION] == 0).all()      # a fall on the time-out tick is a time-out
    assert (e[case == 6, ref.TERMINATION] == scale).all() and (rew[case == 6] < 0).all()                  # a fall before it is charged, below the clip
    assert ((b["reset"] != 0) == (b["fell"] | (b["progress"] > ref.MAX_EPISODE_LENGTH))).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_state_that_blew_up(shim, bad):
    n, P = 70, 65
    first, second = ref.blown_up_ticks(n, P, bad)
    hit, off = ref.BLOWN, ref.BLOWN_OFF
    none, everybody = ref.marks(n, "none"), ref.marks(n, "all")
    for scales, live in ((off, False), (ref.ALL_ON, True)):
        host, want = Host(shim, n, scales), restatement(n, scales)
        run_chain(host, want, [(everybody, first)], "first")
        (e, rew, _, _, task6, _), = run_chain(host, want, [(none, second)], ("second", live))
        if not live:                                                           # the affected terms are off: nothing of them reaches the reward or the sums
            assert np.isfinite(e).all() and np.isfinite(rew[[5, 7, 9]]).all() and np.isfinite(host.sums).all()
            assert (e[:, [ref.ORIENTATION, ref.BASE_HEIGHT, ref.DOF_VEL, ref.DOF_ACC]] == 0).all()
        else:                                                                  # live: the term is what the arithmetic gives, and the reward what fmaxf gives
            for r, i in hit.items():
                assert not np.isfinite(e[r, i]), (r, i)
            # rows 5, 7, 9 leave the task's own six terms finite: the sum under the clip is NaN or -inf (a penalised +inf), fmaxf gives 0, termination follows
            assert (rew[[5, 7, 9]] == (F(0) + e[:, ref.TERMINATION])[[5, 7, 9]]).all() and np.isfinite(task6[[5, 7, 9]]).all()
            assert not np.isfinite(host.sums[[3, 5, 7, 9]]).all(1).any()
            S = host.close(everybody)
            assert same(S, want.close(everybody)) and S[0] == n - 4 and np.isfinite(S).all() and not host.sums.any()       # such an episode closes nothing


@pytest.mark.parametrize("n", ref.SIZES)
@pytest.mark.parametrize("pattern", ["none", "some", "all"])
def test_close_and_window_equal_the_restatement(shim, n, pattern):
    rng = np.random.default_rng(7 * n)
    host, want = Host(shim, n, ref.ALL_ON), restatement(n, ref.ALL_ON)
    mag = F(10.0) ** rng.integers(-6, 4, (n, 8)).astype(F)
    sums = (rng.standard_normal((n, 8)).astype(F) * mag).astype(F)
    ticks = rng.integers(0, 3, n).astype(np.int32) * rng.integers(1, 900, n).astype(np.int32)      # a third holds no tick
    if n >= 63:
        sums[5, 2], sums[17, 7], sums[40, 0] = np.nan, np.inf, -np.inf
    window = np.arange(9) * 0.125 + 3.0                                        # a window that already holds something
    for obj in (host, want):
        obj.sums, obj.ticks, obj.window = sums.copy(), ticks.copy(), window.copy()
    ids = ref.marks(n, pattern)
    marked = ids >= 0
    S = host.close(ids)
    assert S.tobytes() == want.close(ids).tobytes() and np.isfinite(S).all()
    assert_states_equal(host, want, (n, pattern))
    with np.errstate(all="ignore"):
        closed = marked & (ticks > 0) & np.isfinite(sums).all(1)
    assert S[0] == closed.sum() and (host.window == window + S).all()
    assert same(host.sums[~marked], sums[~marked]) and (host.ticks[~marked] == ticks[~marked]).all() and not host.sums[marked].any() and not host.ticks[marked].any()
    if pattern == "none":
        assert not S.any()
    if pattern == "all" and n == 130:                                          # the order is the rule's: a plain sum in another order differs, so EQUAL means something
        assert not np.array_equal(sums[closed].astype(np.float64)[::-1].sum(0), S[1:])
    for stage in (1, 4):                                                       # the join's staging does not change the sum
        again = Host(shim, n, ref.ALL_ON)
        again.sums, again.ticks, again.window = sums.copy(), ticks.copy(), window.copy()
        assert again.close(ids, stage=stage).tobytes() == S.tobytes()


def test_all_scales_zero_is_the_tasks_reward(shim):
    n, P = 130, 187
    host = Host(shim, n, [0.0] * 8)
    for t, (ids, b) in enumerate(chain(n, P, 3)):
        host.close(ids)
        e, rew, task6, from6 = host.run(b, ids)
        assert (rew == from6).all() and rew.tobytes() == from6.tobytes() and not e.any() and not host.sums.any()
    assert (host.ticks > 0).all() and host.air_time.any() and host.last_actions.any()      # the history is kept whatever the scales are


@pytest.mark.parametrize("P", ref.POINTS + (2, 128, 208))
def test_height_mean_order(shim, P):
    rng = np.random.default_rng(P)
    z = rng.standard_normal(40).astype(F)
    h = (rng.standard_normal((40, max(P, 1))) * 10.0 ** rng.integers(-3, 2, (40, max(P, 1)))).astype(F)[:, :P]
    want = ref.height_mean(z, h if P else None)
    got = np.array([shim.shim_height_mean(float(z[r]), np.ascontiguousarray(h[r]).ctypes.data if P else None, P) for r in range(40)], F)
    assert got.tobytes() == want.tobytes()
    if P == 0:
        assert got.tobytes() == z.tobytes()
    if P == 187:                                                               # the order is the rule's: numpy's own mean differs somewhere
        assert not np.array_equal((z[:, None] - h).mean(1, dtype=F), want)


def test_the_six_term_reduction_keeps_its_words(shim):
    """episode_terms.h's block_partial_word / join_word now forward to the generalised forms: the same words as the written-out rule."""
    rng = np.random.default_rng(1)
    count, stride = 64, 7
    closed = (rng.random(count) < 0.6).astype(np.int32)
    sums = (rng.standard_normal((count, stride)) * 10.0 ** rng.integers(-5, 4, (count, stride))).astype(F)
    for j in range(8):
        acc = 0.0
        if j <= 6:
            for e in range(count):
                if closed[e]:
                    acc = acc + (1.0 if j == 0 else float(sums[e, j - 1]))
        assert shim.shim_epterms_partial(count, closed.ctypes.data, sums.ctypes.data, stride, j) == acc
    partials = rng.standard_normal((9, 8))
    for j in range(8):
        acc = 0.5
        for b in range(9):
            acc = acc + float(partials[b, j])
        assert shim.shim_epterms_join(0.5, 9, partials.ctypes.data, j) == acc


def test_spec_validation_is_host_side(monkeypatch):
    spec = RS.ShapingSpec(orientation=-0.2, termination=-200.0)
    assert spec.validate() is spec and spec.air_time_target == 0.5 and spec.base_height == 0.0
    assert spec.scales(0.01) == [-0.2 * 0.01, 0, 0, 0, 0, 0, 0, -200.0 * 0.01]
    assert RS.ShapingSpec().scales(0.005) == [0.0] * 8
    for kw, text in ((dict(dof_acc=float("nan")), "finite"), (dict(base_height_target=float("inf")), "finite"), (dict(air_time_target=float("nan")), "finite"),
                     (dict(air_time_target=-0.1), "air_time_target")):
        with pytest.raises(ValueError, match=text):
            RS.ShapingSpec(**kw).validate()
        with pytest.raises(ValueError, match=text):                           # RewardShaping validates the spec before it asks for a device
            RS.RewardShaping(8, RS.ShapingSpec(**kw))
    with pytest.raises(ValueError, match="n must"):
        RS.RewardShaping(0)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.MpcLibraryError):
        rl_mpc_locomotion_amd.RewardShaping(8, rl_mpc_locomotion_amd.ShapingSpec(orientation=-1.0))


def test_record_of_a_summary():
    values = [4.0, 8.0, -2.0, 0.0, 1.0, -0.5, 0.0, -1.0, 16.0, 2.0]
    assert RS.RewardShaping.record(values) == {"rew_orientation": 1.0, "rew_base_height": -0.25, "rew_dof_vel": 0.0, "rew_dof_acc": 0.125, "rew_action_rate": -0.0625,
                                               "rew_feet_air_time": 0.0, "rew_stand_still": -0.125, "rew_termination": 2.0}
    empty = RS.RewardShaping.record([0.0] * 9 + [20.0])
    assert list(empty) == ["rew_" + t for t in RS.SHAPING_TERMS] and not any(empty.values())
    assert ref.summary(np.array(values[:9]), 2.0).tolist() == values


def test_abi_symbols_are_the_headers_and_nobody_elses():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(RS.SYMBOLS) and len(names) == 9
    others = set(_lib.SYMBOLS) | set(rl_task.SYMBOLS) | set(toy_sim.SYMBOLS) | set(episode_terms.SYMBOLS) | set(privileged_obs.SYMBOLS)
    assert not set(names) & others
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        assert "mpc_shaping_" not in open(os.path.join(ROOT, "include", h)).read(), h
    protos = re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(mpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert sorted(p[1] for p in protos) == names
    raw = C.CDLL(_lib.LIB_PATH)
    L = RS.lib()
    for ret, name, params in protos:
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert len(f.argtypes) == (0 if params.strip() in ("", "void") else params.count(",") + 1), name
        assert (f.restype is None) == (" ".join(ret.split()) == "void"), name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "reward_shaping" in re.search(r"^UOBJS\s*:=.*$", make, re.M).group(0) and re.search(r"^#\s+reward_shaping .*contraction", make, re.M | re.S)
    assert re.search(r"MPC_SHAPING_TERMS = (\d+), MPC_SHAPING_SUMMARY = (\d+), MPC_SHAPING_MAX_POINTS = (\d+)", text).groups() == (
        str(RS.NUM_TERMS), str(RS.SUMMARY_LEN), str(RS.MAX_POINTS))


def test_bad_arguments_are_refused_without_a_gpu():
    L = RS.lib()
    E_ARG = -1
    h = C.c_void_p()
    good = CFG._struct()
    zeros = (C.c_double * 8)()

    def create(out=C.byref(h), n=4, cfg=good, scales=zeros, hgt=0.3, air=0.5, dt=0.01, ep=20.0):
        return L.mpc_shaping_create(out, n, None if cfg is None else C.addressof(cfg), None if scales is None else C.addressof(scales), hgt, air, dt, ep)

    nan_scale = CFG._struct(); nan_scale.rew_scale[2] = float("nan")
    swapped = CFG._struct(); swapped.command_range[1][0], swapped.command_range[1][1] = 1.0, -1.0
    no_len = CFG._struct(); no_len.max_episode_length = 0
    bad_pos = CFG._struct(); bad_pos.default_dof_pos[7] = float("inf")
    bad_scales = (C.c_double * 8)(); bad_scales[3] = float("nan")
    for kw, text in (({"out": None}, b"null"), ({"cfg": None}, b"null"), ({"scales": None}, b"null"), ({"n": 0}, b"n must"), ({"n": -3}, b"n must"),
                     ({"cfg": nan_scale}, b"not finite"), ({"cfg": swapped}, b"min > max"), ({"cfg": no_len}, b"max_episode_length"),
                     ({"cfg": bad_pos}, b"default_dof_pos"), ({"scales": bad_scales}, b"shaping scale"), ({"hgt": float("nan")}, b"base_height_target"),
                     ({"air": -0.5}, b"air_time_target"), ({"air": float("inf")}, b"air_time_target"), ({"dt": 0.0}, b"dt must"), ({"dt": float("nan")}, b"dt must"),
                     ({"ep": 0.0}, b"episode_length_s"), ({"ep": float("inf")}, b"episode_length_s")):
        assert create(**kw) == E_ARG, kw
        msg = L.mpc_shaping_last_error()
        assert b"mpc_shaping_create" in msg and text in msg, (kw, msg)
    assert not h.value
    p = 0x1000
    assert L.mpc_shaping_bind(None, p) == E_ARG and b"null handle" in L.mpc_shaping_last_error()
    assert L.mpc_shaping_close(None, p, None) == E_ARG and b"mpc_shaping_close: null" in L.mpc_shaping_last_error()
    assert L.mpc_shaping_run(None, *[p] * 10, 1, p, p, None) == E_ARG and b"mpc_shaping_run: null" in L.mpc_shaping_last_error()
    assert L.mpc_shaping_summary(None, p, None) == E_ARG and L.mpc_shaping_new_window(None, None) == E_ARG
    assert L.mpc_shaping_arrays(None, *[C.byref(C.c_void_p()) for _ in range(7)]) == E_ARG and b"mpc_shaping_arrays" in L.mpc_shaping_last_error()
    L.mpc_shaping_destroy(None)


def test_the_task_refuses_before_the_device_is_touched(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "need_gpu", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(_lib.MpcLibraryError("device asked for")))

    class Fake:
        def __init__(self, n, cfg=None, **spec):
            self.n, self.spec, self.cfg = n, RS.ShapingSpec(**spec), cfg if cfg is not None else rl_task.TaskConfig()

    class Scan:                                                               # (a height scan as the validation pass sees it)
        n, obs_clip = 4, 5.0
    with pytest.raises(ValueError, match="reward shaping holds 8"):
        rl_task.BatchedRLTask([0] * 4, [0] * 4, reward_shaping=Fake(8))
    for other in (rl_task.TaskConfig(dt=0.005), rl_task.TaskConfig(rew_torque=-1e-4), rl_task.TaskConfig(episode_length_s=10.0)):
        with pytest.raises(ValueError, match="another TaskConfig"):            # the unit's dt, scales and episode length are the task's or it is refused
            rl_task.BatchedRLTask([0] * 4, [0] * 4, reward_shaping=Fake(4, cfg=other))
        with pytest.raises(_lib.MpcLibraryError, match="device asked for"):
            rl_task.BatchedRLTask([0] * 4, [0] * 4, cfg=other, reward_shaping=Fake(4, cfg=other))
    with pytest.raises(TypeError):                                             # cfg is keyword-only: a positional third argument is the device
        RS.RewardShaping(4, RS.ShapingSpec(), None, rl_task.TaskConfig())
    for where in (dict(terrain=object()), dict(curriculum=type("Cur", (), {"n": 4, "terrain": None, "origins0": None})())):
        with pytest.raises(ValueError, match="base_height"):
            rl_task.BatchedRLTask([0] * 4, [0] * 4, reward_shaping=Fake(4, base_height=-1.0), **where)
        with pytest.raises(_lib.MpcLibraryError, match="device asked for"):    # the same term over a scan, and other terms without one, are accepted
            rl_task.BatchedRLTask([0] * 4, [0] * 4, reward_shaping=Fake(4, base_height=-1.0), height_scan=Scan(), **where)
        calls.clear()
        with pytest.raises(_lib.MpcLibraryError, match="device asked for"):
            rl_task.BatchedRLTask([0] * 4, [0] * 4, reward_shaping=Fake(4, orientation=-1.0), **where)
    with pytest.raises(_lib.MpcLibraryError, match="device asked for"):        # on the plane the base height is root_z: no scan needed
        rl_task.BatchedRLTask([0] * 4, [0] * 4, reward_shaping=Fake(4, base_height=-1.0))


def test_the_trainers_rider():
    from rl_mpc_locomotion_amd import ppo

    class Shaping:
        windows = 0

        def summary(self):
            return torch.tensor([2.0, 4.0, 0, 0, 0, 0, 0, 0, -8.0, 2.0], dtype=torch.float64)
        record = staticmethod(RS.RewardShaping.record)

        def new_window(self):
            self.windows += 1

    class Trainer:
        alg = type("Alg", (), {"lr_device": None, "learning_rate": 1e-3})()
        curriculum = episode_terms = None
        episode_stats = type("Stats", (), {"summary": torch.zeros(8, dtype=torch.float64)})()
        _scalars = torch.zeros(5, dtype=torch.float64)
    plain = ppo._read_riders(ppo._riders(Trainer()))
    assert "reward_shaping" not in plain                                       # a trainer without the attribute reads as before
    Trainer.reward_shaping = Shaping()
    record = ppo._read_riders(ppo._riders(Trainer()))
    assert list(record)[:len(plain)] == list(plain) and list(record)[-1] == "reward_shaping"
    assert record["reward_shaping"]["rew_orientation"] == 1.0 and record["reward_shaping"]["rew_termination"] == -2.0 and len(record["reward_shaping"]) == 8
    assert Trainer.reward_shaping.windows == 1


def chain_bytes(ticks, n, P, cfg, spec):
    out = [np.array([n, P, len(ticks)], np.int32).tobytes(), bytes(cfg), bytes(spec)]
    for ids, b in ticks:
        out += [ids.tobytes(), *(np.ascontiguousarray(b[k], F).tobytes() for k in ("root", "dof", "actions", "commands", "torques")),
                np.ascontiguousarray(b["fell"], np.uint8).tobytes(), np.ascontiguousarray(b["reset"], np.int64).tobytes(),
                np.ascontiguousarray(b["progress"], np.int64).tobytes(), np.ascontiguousarray(b["contact"], np.int32).tobytes(),
                b"" if b["heights"] is None else np.ascontiguousarray(b["heights"], F).tobytes()]
    return b"".join(out)


def test_sanitized_stand_alone_program_runs_the_chains_clean(shim, tmp_path):
    """Host code only: a program with its own main, built with -fsanitize=address,undefined, run as a child process."""
    src, exe = tmp_path / "reward_shaping_main.cpp", tmp_path / "reward_shaping_main"
    src.write_text(SHIM + MAIN)
    subprocess.run(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(src), "-o", str(exe)], check=True)
    runs = [(n, P, chain(n, P, 100 * n + P)) for n, P in ((1, 0), (63, 1), (65, 187), (130, 65))]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(runs)], np.int32).tobytes())
        for n, P, ticks in runs:
            f.write(chain_bytes(ticks, n, P, shim_config(CFG), shim_spec(ref.ALL_ON)))
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for n, P, ticks in runs:
        host = Host(shim, n, ref.ALL_ON)
        want = []
        for ids, b in ticks:
            host.close(ids)
            e, rew, _, _ = host.run(b, ids)
            want += [rew, e]
        want += [host.last_actions, host.last_dof_vel, host.air_time, host.last_contact, host.sums, host.ticks, host.window]
        for w in want:
            assert raw[at:at + w.nbytes] == w.tobytes(), (n, P)
            at += w.nbytes
    assert at == len(raw)


def test_kernels_compile_for_gfx950_without_scratch(tmp_path, capsys):
    out = tmp_path / "mpc_reward_shaping.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "mpc_reward_shaping.hip"), "-o", str(out)], check=True, capture_output=True, text=True)
    found = {}
    for name, sgpr, vgpr, scratch, lds in re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                                                     r.stderr, re.S):
        found[name] = dict(sgprs=int(sgpr), vgprs=int(vgpr), scratch=int(scratch), lds=int(lds))
    with capsys.disabled():
        for name, v in found.items():
            print(f"\n  {name}: {v}", end="")
    close = 64 * 9 * 4 + 64 * 4                                            # a wave's float32 sums in rows of 9 words, and its closed flags
    join = 256 * 16 * 8                                                    # 256 staged partial rows
    for kernel, lds in (("shaping_close_kernel", close), ("shaping_join_kernel", join), ("shaping_run_kernel", 16 * 4), ("shaping_summary_kernel", 0)):
        hit = [v for k, v in found.items() if kernel in k]
        assert len(hit) == 1 and hit[0]["scratch"] == 0 and hit[0]["lds"] == lds, (kernel, found)
    assert len(found) == 4
    text = open(os.path.join(CSRC, "mpc_reward_shaping.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", text) and "hipFuncSetAttribute" not in text
