"""The contact terms on the CPU (csrc/contact_terms.h, csrc/mpc_contact_terms.h, rl_mpc_locomotion_amd.contact_terms): the header compiled with g++ into
a small shim and compared with the restatement of tests/contact_terms_ref.py -- terms, reward, sums, ticks, close, window and the widened row EQUAL --,
the hand-made rows one by one, the spec's validation, the ABI's symbols and argument checks, the task's refusals, the trainer's rider, the sanitized
stand-alone refusals program, and the kernels' scratch and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, contact_terms as CT, episode_terms, friction, privileged_obs, reward_shaping, rl_task, toy_sim
from tests import contact_terms_ref as ref
from tests.contact_terms_ref import F, NEAR, same
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HEADER = os.path.join(CSRC, "mpc_contact_terms.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC]
CFG = rl_task.TaskConfig(episode_length_s=0.3, dt=ref.DT)
FORCE_SCALE, MU_CLIP, CLIP_OBS = 0.01, 2.0, 5.0
E_ARG = -1

SHIM = r"""
#include "contact_terms.h"
using namespace cterms;
extern "C" {
int shim_layout(int *out) {
  const int v[] = {kTerms, kBlock, kPartial, kWords, kColumns, kSumClosed, kSumTerms, kSumEpisodeS, kSummaryLen, (int)sizeof(Spec), (int)sizeof(Shaping),
                   kFeetSlip, kFeetContactForces, kFeetStumble, kShapingTerms, kShapingTermination, kTaskTerms, kLegs};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
  return (int)(sizeof(v) / sizeof(v[0]));
}
// one tick of n environments as the run kernel makes it, the task's six terms [n][6] and the shaping unit's eight [n][8] (g->live) given
void shim_run(const Spec *k, const Shaping *g, int n, const float *force, const float *slip, const int *ids, const float *task6, const float *shaping,
              float *sums, int *ticks, float *rew, float *terms) {
  for (int r = 0; r < n; ++r) {
    float e[kTerms], se[kShapingTerms];
    for (int i = 0; i < kShapingTerms; ++i) se[i] = g->live ? shaping[r * kShapingTerms + i] : 0.0f;
    tick_terms(*k, force + 12 * r, slip + 4 * r, ids[r], e);
    rew[r] = reward_from(*k, *g, chain_from(*g, task6 + 6 * r, se), e, se);
    accumulate_env(e, sums + kTerms * r, ticks[r]);
    for (int i = 0; i < kTerms; ++i) terms[r * kTerms + i] = e[i];
  }
}
// the two launches of mpc_contact_close, as the kernels make them: `stage` block partials per pass of the join
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
// the row widening, column by column as the kernel's words are made
void shim_extend(const Spec *k, int n, int Wp, const float *priv, const double *mu, const float *force, float *out) {
  for (int r = 0; r < n; ++r) {
    for (int j = 0; j < Wp; ++j) out[(size_t)r * (Wp + kColumns) + j] = priv[(size_t)r * Wp + j];
    for (int j = 0; j < kColumns; ++j) out[(size_t)r * (Wp + kColumns) + Wp + j] = column(*k, mu[r], force + 12 * r, j);
  }
}
}
"""


class ShimSpec(C.Structure):           # cterms::Spec
    _fields_ = [("scale", C.c_float * 3), ("max_contact_force", C.c_float), ("dt", C.c_float), ("force_scale", C.c_float), ("mu_clip", C.c_float),
                ("clip_obs", C.c_float)]


class ShimShaping(C.Structure):        # cterms::Shaping
    _fields_ = [("live", C.c_int), ("scale", C.c_float * 8)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("contact_terms_shim")
    src, so = d / "contact_terms_shim.cpp", d / "contact_terms_shim.so"
    src.write_text(SHIM)
    subprocess.run(GXX + ["-fPIC", "-shared", str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    vp, ci = C.c_void_p, C.c_int
    L.shim_layout.argtypes = [vp]
    L.shim_run.argtypes, L.shim_run.restype = [vp, vp, ci] + [vp] * 9, None
    L.shim_close.argtypes, L.shim_close.restype = [ci, vp, vp, vp, vp, ci, vp], None
    L.shim_extend.argtypes, L.shim_extend.restype = [vp, ci, ci, vp, vp, vp, vp], None
    return L


def shim_spec(per_second, max_force=ref.MAX_FORCE, dt=ref.DT, mu_clip=MU_CLIP):
    k = ShimSpec()
    k.scale[:] = [float(v) for v in ref.scales_of(per_second, dt)]
    k.max_contact_force, k.dt, k.force_scale, k.mu_clip, k.clip_obs = max_force, dt, FORCE_SCALE, mu_clip, CLIP_OBS
    return k


def shim_shaping(per_second, dt=ref.DT):
    g = ShimShaping()
    if per_second is not None:
        g.live = 1
        g.scale[:] = [float(v) for v in ref.scales_of(per_second, dt)]
    return g


class Host:
    """The header's state and its two calls through the shim, shaped like ref.Contact."""

    def __init__(self, L, n, per_second, shaping=None, **spec):
        self.L, self.n, self.k, self.g = L, n, shim_spec(per_second, **spec), shim_shaping(shaping)
        self.sums, self.ticks, self.window = np.zeros((n, 3), F), np.zeros(n, np.int32), np.zeros(4)

    state = ref.Contact.state

    def close(self, ids, stage=256):
        S = np.zeros(4)
        self.L.shim_close(self.n, ids.ctypes.data, self.sums.ctypes.data, self.ticks.ctypes.data, self.window.ctypes.data, stage, S.ctypes.data)
        return S

    def run(self, force, slip, ids, task6, shaping_terms=None):
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        force, slip, ids, task6 = a(force, F), a(slip, F), a(ids, np.int32), a(task6, F)
        se = None if shaping_terms is None else a(shaping_terms, F)
        rew, terms = np.zeros(self.n, F), np.zeros((self.n, 3), F)
        self.L.shim_run(C.addressof(self.k), C.addressof(self.g), self.n, force.ctypes.data, slip.ctypes.data, ids.ctypes.data, task6.ctypes.data,
                        None if se is None else se.ctypes.data, self.sums.ctypes.data, self.ticks.ctypes.data, rew.ctypes.data, terms.ctypes.data)
        return terms, rew


def restatement(n, per_second, max_force=ref.MAX_FORCE, dt=ref.DT):
    return ref.Contact(n, ref.scales_of(per_second, dt), max_force, dt)


def assert_state(host, want, what):
    for name, w in want.state().items():
        assert same(host.state()[name], w), (what, name)


def test_layouts_agree(shim):
    out = (C.c_int * 32)()
    k = shim.shim_layout(out)
    assert list(out[:k]) == [3, 64, 8, 4, 16, CT.S_CLOSED, CT.S_TERMS, CT.S_EPISODE_S, CT.SUMMARY_LEN, C.sizeof(ShimSpec), C.sizeof(ShimShaping), 0, 1, 2, 8, 7, 6, 4]
    assert CT.CONTACT_TERMS == ref.TERMS == ("feet_slip", "feet_contact_forces", "feet_stumble") and CT.NUM_TERMS == ref.NT == 3
    assert CT.COLUMNS == ref.COLUMNS == 16 and CT.WINDOW_LEN == ref.WINDOW_LEN == 4 and CT.NUM_SHAPING_TERMS == reward_shaping.NUM_TERMS == 8
    assert reward_shaping.SHAPING_TERMS.index("termination") == ref.SHAPING_TERMINATION
    assert len(reward_shaping.SHAPING_TERMS) == 8 and len(rl_task.REWARD_TERMS) == 6 and len(rl_task.STAGES) == 13


@pytest.mark.parametrize("shaping", [None, ref.SHAPING_ON, ref.SHAPING_NO_TERMINATION], ids=["plain", "shaped", "shaped_no_termination"])
@pytest.mark.parametrize("scales", ref.SUBSETS, ids=lambda s: "".join("1" if v else "0" for v in s))
def test_six_chained_ticks_equal_the_restatement(shim, scales, shaping):
    """Every subset of live scales, without and with shaping terms (termination live and off), n = 65: terms, reward, sums, ticks and window."""
    n = 65
    host, want = Host(shim, n, scales, shaping), restatement(n, scales)
    rng = np.random.default_rng(17)
    g = None if shaping is None else ref.scales_of(shaping, ref.DT)
    clipped = paid = 0
    for t, (ids, b) in enumerate(ref.chain(n, 500 + n)):
        se = None if shaping is None else ref.shaping_tick(n, rng)
        assert same(host.close(ids), want.close(ids)), t
        e, rew = host.run(b["force"], b["slip"], ids, b["task6"], se)
        e_want, rew_want = want.run(b["force"], b["slip"], ids, b["task6"], g, se)
        assert same(e, e_want), (t, "terms", np.argwhere(~(e == e_want)))
        assert same(rew, rew_want), (t, "rew")
        assert_state(host, want, t)
        assert not e[ids >= 0].any()                                          # a marked tick pays nothing
        for i in range(3):
            assert (e[:, i] != 0).any() == (scales[i] != 0 and not (ids >= 0).all()), (t, i)
        plain = ref.reward((0, 0, 0), b["task6"], e, g, se)
        if not any(scales):
            assert rew.tobytes() == plain.tobytes()                            # all three off: the reward of the step without the unit
        clipped += int((rew == (0 if g is None or g[7] == 0 else se[:, 7])).sum())
        paid += int((rew > 0).sum())
    assert clipped > 0 and paid > 0                                            # both sides of the clip
    # nothing closes on the tick that resets everybody first; the resets of two consecutive ticks all do, an environment in both of them twice
    assert want.window[0] == (ref.marks(n, "some", 2) >= 0).sum() + (ref.marks(n, "some", 3) >= 0).sum() > 0
    assert ((ref.marks(n, "some", 2) >= 0) & (ref.marks(n, "some", 3) >= 0)).any()


def test_the_hand_made_rows_one_by_one(shim):
    """The limits from both sides: a leg exactly at max_contact_force and one ulp above, a tangential force exactly 5 |Fz| and one ulp above, zero
    rows, a foot that slid and lifted."""
    force, slip = ref.crafted_rows()
    n = len(force)
    k = ref.scales_of(ref.ALL_ON, ref.DT)
    host = Host(shim, n, ref.ALL_ON)
    none = np.full(n, -1, np.int32)
    e, rew = host.run(force, slip, none, np.zeros((n, 6), F))
    assert same(e, ref.terms_of(k, ref.MAX_FORCE, ref.DT, force, slip, none))
    assert not e[0].any()                                                      # zero rows
    above = NEAR(ref.FMAX, F(np.inf))
    assert np.sqrt(ref.FMAX * ref.FMAX) == ref.FMAX and np.sqrt(above * above) == above        # the norms of (0, 0, m) are m at both of them
    assert e[1, 1] == 0 and e[2, 1] == (above - ref.FMAX) * k[1] < 0           # exactly at the limit pays nothing, one ulp above pays that ulp
    t_at, t_above = np.sqrt(F(15) * F(15)), np.sqrt(NEAR(F(15), F(np.inf)) * NEAR(F(15), F(np.inf)))
    assert t_at == F(5) * F(3) < t_above                                       # the tangential norms: exactly 5 |Fz|, and one ulp above it
    assert e[3, 2] == 0 and e[4, 2] == k[2] and e[8, 2] == 0 and e[7, 2] == k[2]               # exactly on the cone of 5 is no stumble, one ulp outside is
    dt = F(ref.DT)
    v = [F(s) / dt for s in slip[5]]
    assert e[5, 0] == ((((F(0) + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]) * k[0] < 0
    m = [np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) for f in force[5]]
    assert e[5, 1] == ((((F(0) + (m[0] - ref.FMAX)) + (m[1] - ref.FMAX)) + (m[2] - ref.FMAX)) + (m[3] - ref.FMAX)) * k[1] < 0
    assert e[6, 0] == ((F(0.007) / dt) * (F(0.007) / dt)) * k[0] < 0 and not force[6].any()     # no contact filter: the foot that lifted still counts
    assert same(rew, np.zeros(n, F))                                           # penalties alone: the clip holds the reward at 0
    marked = np.arange(n, dtype=np.int32)
    e, _ = Host(shim, n, ref.ALL_ON).run(force, slip, marked, np.zeros((n, 6), F))
    assert e.tobytes() == np.zeros((n, 3), F).tobytes()                        # the tick that performs the reset: +0 everywhere


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_force_or_a_slide_that_blew_up(shim, bad):
    """Rows 1 and 2 carry `bad` in a force component and in a slide.  With the terms off nothing reaches the reward.  With them on: fmaxf and the
    comparison swallow a NaN force (contact_terms.h says so), an inf force and a NaN or inf slide reach their terms, the reward is fmaxf's 0 and the
    close of everybody leaves those episodes out."""
    n = 6
    rng = np.random.default_rng(4)
    b = ref.random_tick(n, rng)
    b["task6"][:] = (0.01, 0, 0, 0.004, 0, 0)                                  # a reward above the clip
    b["force"][:], b["slip"][:] = (3.0, -2.0, 40.0), 0.0
    b["force"][1, 2, 0], b["slip"][2, 3] = bad, bad
    none, everybody = np.full(n, -1, np.int32), np.arange(n, dtype=np.int32)
    for scales, live in ((ref.SUBSETS[0], False), (ref.ALL_ON, True)):
        host, want = Host(shim, n, scales), restatement(n, scales)
        host.close(everybody), want.close(everybody)
        e, rew = host.run(b["force"], b["slip"], none, b["task6"])
        e_want, rew_want = want.run(b["force"], b["slip"], none, b["task6"])
        assert same(e, e_want) and same(rew, rew_want)
        assert_state(host, want, live)
        if not live:
            assert not e.any() and (rew == rew[0]).all() and rew[0] > 0 and np.isfinite(host.sums).all()
        else:
            assert np.isfinite(e[1]).all() == bool(np.isnan(bad))              # a NaN force is swallowed by fmaxf, an inf one is not
            assert not np.isfinite(e[2, 0]) and rew[2] == 0 and rew[0] > 0
            assert rew[1] == (rew[0] if np.isnan(bad) else 0)
        S = host.close(everybody)
        assert same(S, want.close(everybody))
        broken = 0 if not live else (1 if np.isnan(bad) else 2)
        assert S[0] == n - broken and np.isfinite(host.window).all() and not host.sums.any() and not host.ticks.any()


@pytest.mark.parametrize("n", ref.SIZES)
def test_close_and_join_equal_the_loop_restatement(shim, n):
    """Sums of mixed size, sign and a few non-finite rows, closed by every pattern, with the join staged 1, 2 and 256 partials at a time."""
    for pattern in ("none", "some", "all"):
        rng = np.random.default_rng(n + len(pattern))
        sums = (rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-6, 3, (n, 3))).astype(F)
        sums[rng.random(n) < 0.1, 1] = np.nan
        sums[rng.random(n) < 0.05, 0] = -np.inf
        ticks = rng.integers(0, 3, n).astype(np.int32)
        ids = ref.marks(n, pattern)
        for stage in (1, 2, 256):
            host, want = Host(shim, n, ref.ALL_ON), restatement(n, ref.ALL_ON)
            host.sums, host.ticks, want.sums, want.ticks = sums.copy(), ticks.copy(), sums.copy(), ticks.copy()
            host.window[:] = want.window[:] = (3.0, -1.5, 0.25, -7.0)
            assert same(host.close(ids, stage), want.close(ids)), (pattern, stage)
            assert_state(host, want, (pattern, stage))
        assert same(host.sums[ids < 0], sums[ids < 0]) and not host.sums[ids >= 0].any() and not host.ticks[ids >= 0].any()


@pytest.mark.parametrize("n,wp", [(1, 64), (65, 240), (130, 256)])
def test_the_widened_row_equals_the_restatement(shim, n, wp):
    rng = np.random.default_rng(wp)
    priv = rng.standard_normal((n, wp)).astype(F)
    priv[0, :4] = (np.nan, -0.0, np.inf, 1e-42)                                # copied bit for bit, whatever the words are
    force = (rng.standard_normal((n, 4, 3)) * [60, 60, 300]).astype(F)       # beyond the clip on both sides at force_scale 0.01
    force[0, 0] = (500.0, -500.0, np.nextafter(F(500), F(np.inf)))
    mu = np.resize(np.array([0.0, 0.4, MU_CLIP, np.inf, 1.9999999, 2.5]), n)
    out = np.full((n, wp + 16), 7.0, F)
    k = shim_spec(ref.ALL_ON)
    shim.shim_extend(C.addressof(k), n, wp, priv.ctypes.data, mu.ctypes.data, force.ctypes.data, out.ctypes.data)
    want = ref.extend(priv, mu, force, FORCE_SCALE, MU_CLIP, CLIP_OBS)
    assert out.tobytes()[:16] == want.tobytes()[:16] and same(out, want) and out[:, :wp].tobytes() == priv.tobytes()
    assert out[0, wp] == 0 and (out[:, wp] <= F(MU_CLIP)).all() and not out[:, wp + 13:].any()
    assert out[0, wp + 1] == 5 and out[0, wp + 2] == -5 and out[0, wp + 3] == 5 and (np.abs(out[:, wp + 1:wp + 13]) < 5).any()
    if n > 3:
        assert out[1, wp] == F(0.4) and out[2, wp] == F(MU_CLIP) and out[3, wp] == F(MU_CLIP)


def test_spec_validation_is_host_side(monkeypatch):
    monkeypatch.setattr(_lib, "need_gpu", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    S = CT.ContactSpec
    d = S()
    assert (d.feet_slip, d.feet_contact_forces, d.feet_stumble, d.max_contact_force, d.force_scale, d.mu_clip) == (0.0, 0.0, 0.0, 100.0, 0.01, 2.0)
    assert S(max_contact_force=0.0).validate().scales(0.01) == [0.0, 0.0, 0.0]
    assert S(feet_slip=-0.4, feet_stumble=3.0).scales(0.005) == [-0.4 * 0.005, 0.0, 3.0 * 0.005]
    for bad, msg in ((S(feet_slip=float("nan")), "finite"), (S(feet_stumble=float("inf")), "finite"), (S(max_contact_force=float("inf")), "finite"),
                     (S(max_contact_force=-1.0), "max_contact_force"), (S(force_scale=0.0), "> 0"), (S(mu_clip=-2.0), "> 0"), (S(mu_clip=float("inf")), "finite")):
        with pytest.raises(ValueError, match=msg):
            bad.validate()
        with pytest.raises(ValueError, match=msg):
            CT.ContactTerms(4, bad)
    with pytest.raises(ValueError, match="at least 1"):
        CT.ContactTerms(0)
    unit = CT.ContactTerms(4, S(feet_slip=-1.0), cfg=CFG, privileged=True)      # host memory only until bind
    assert unit.privileged and unit.cfg is CFG and unit.sums is None and unit.width(80) == 96
    with pytest.raises(TypeError):                                             # cfg is keyword-only: a positional third argument is the device
        CT.ContactTerms(4, S(), None, CFG)


def test_record_of_a_summary():
    values = [4.0, 8.0, -2.0, 0.0, 2.0]
    assert CT.ContactTerms.record(values) == {"rew_feet_slip": 1.0, "rew_feet_contact_forces": -0.25, "rew_feet_stumble": 0.0}
    empty = CT.ContactTerms.record([0.0] * 4 + [20.0])
    assert list(empty) == ["rew_" + t for t in CT.CONTACT_TERMS] and not any(empty.values())
    assert ref.summary(np.array(values[:4]), 2.0).tolist() == values


def _names(path, pattern=r"\b(mpc_[a-z0-9_]+)\s*\("):
    return sorted(set(re.findall(pattern, re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))))


def test_abi_symbols_are_the_headers_and_nobody_elses():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = _names(HEADER)
    assert names == sorted(CT.SYMBOLS) and len(names) == 10
    others = (set(_lib.SYMBOLS) | set(rl_task.SYMBOLS) | set(toy_sim.SYMBOLS) | set(episode_terms.SYMBOLS) | set(privileged_obs.SYMBOLS) |
              set(reward_shaping.SYMBOLS) | set(friction.SYMBOLS))
    assert not set(names) & others
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        assert "mpc_contact_" not in open(os.path.join(ROOT, "include", h)).read(), h
    # the neighbours keep their entry points, and their kernels
    assert len(_names(os.path.join(CSRC, "mpc_friction.h"))) == 10 and len(_names(os.path.join(CSRC, "mpc_reward_shaping.h"))) == 9
    assert len(_names(os.path.join(CSRC, "mpc_friction.hip"), r"\bvoid\s+(\w+_kernel)\s*\(")) == 3
    assert len(_names(os.path.join(CSRC, "mpc_privileged_obs.hip"), r"\bvoid\s+(\w+_kernel)\s*\(")) == 2
    protos = re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(mpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert sorted(p[1] for p in protos) == names
    raw = C.CDLL(_lib.LIB_PATH)
    L = CT.lib()
    for ret, name, params in protos:
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert len(f.argtypes) == (0 if params.strip() in ("", "void") else params.count(",") + 1), name
        assert (f.restype is None) == (" ".join(ret.split()) == "void"), name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "contact_terms" in re.search(r"^UOBJS\s*:=.*$", make, re.M).group(0) and re.search(r"^#\s+contact_terms .*contraction", make, re.M | re.S)
    assert re.search(r"MPC_CONTACT_TERMS = (\d+), MPC_CONTACT_SUMMARY = (\d+), MPC_CONTACT_COLUMNS = (\d+), MPC_CONTACT_SHAPING_TERMS = (\d+)", text).groups() == (
        str(CT.NUM_TERMS), str(CT.SUMMARY_LEN), str(CT.COLUMNS), str(CT.NUM_SHAPING_TERMS))


def test_bad_arguments_are_refused_without_a_gpu():
    L = CT.lib()
    err = L.mpc_contact_last_error
    h = C.c_void_p()
    good = CFG._struct()
    scales = (C.c_double * 3)(-0.004, -0.0002, -0.015)

    def create(out=C.byref(h), n=4, cfg=good, scales=scales, fmax=100.0, fs=0.01, mc=2.0, dt=0.01, ep=20.0):
        return L.mpc_contact_create(out, n, None if cfg is None else C.addressof(cfg), None if scales is None else C.addressof(scales), fmax, fs, mc, dt, ep)

    nan_scale = CFG._struct(); nan_scale.rew_scale[2] = float("nan")
    swapped = CFG._struct(); swapped.command_range[1][0], swapped.command_range[1][1] = 1.0, -1.0
    no_len = CFG._struct(); no_len.max_episode_length = 0
    bad_clip = CFG._struct(); bad_clip.clip_observations = float("nan")
    bad_scales = (C.c_double * 3)(); bad_scales[1] = float("inf")
    for kw, text in (({"out": None}, b"null"), ({"cfg": None}, b"null"), ({"scales": None}, b"null"), ({"n": 0}, b"n must"), ({"n": -3}, b"n must"),
                     ({"cfg": nan_scale}, b"not finite"), ({"cfg": swapped}, b"min > max"), ({"cfg": no_len}, b"max_episode_length"),
                     ({"cfg": bad_clip}, b"clip_observations"), ({"scales": bad_scales}, b"contact scale"), ({"fmax": -1.0}, b"max_contact_force"),
                     ({"fmax": float("nan")}, b"max_contact_force"), ({"fs": 0.0}, b"force_scale"), ({"fs": float("inf")}, b"force_scale"),
                     ({"mc": 0.0}, b"mu_clip"), ({"mc": float("nan")}, b"mu_clip"), ({"dt": 0.0}, b"dt must"), ({"dt": float("nan")}, b"dt must"),
                     ({"ep": 0.0}, b"episode_length_s"), ({"ep": float("inf")}, b"episode_length_s")):
        assert create(**kw) == E_ARG, kw
        assert b"mpc_contact_create" in err() and text in err(), (kw, err())
    assert not h.value
    assert create() == 0 and h.value                                           # a host-only handle
    p, q, odd = 0x10000, 0x80000, 0x10004
    shaping = (C.c_double * 8)(*([-0.001] * 8))
    assert L.mpc_contact_bind(None, p) == E_ARG and b"null handle" in err()
    assert L.mpc_contact_bind(h, None) == E_ARG and b"null sim" in err()
    assert L.mpc_contact_close(None, p, None) == E_ARG and b"mpc_contact_close: null" in err()
    assert L.mpc_contact_close(h, p, None) == E_ARG and b"no sim bound" in err()
    assert L.mpc_contact_run(None, p, p, p, None, p, None, None, p, None, None) == E_ARG and b"mpc_contact_run: null" in err()
    assert L.mpc_contact_run(h, p, p, None, None, p, None, None, p, None, None) == E_ARG and b"mpc_contact_run: null" in err()
    assert L.mpc_contact_run(h, p, p, p, None, p, q, None, p, None, None) == E_ARG and b"goes with shaping_scales" in err()
    assert L.mpc_contact_run(h, p, p, p, None, p, None, shaping, p, None, None) == E_ARG and b"goes with shaping_scales" in err()
    assert L.mpc_contact_run(h, p, p, p, None, p, q, shaping, p, q, None) == E_ARG and b"must not be d_shaping_terms" in err()
    assert L.mpc_contact_run(h, p, p, p, None, p, q, shaping, p, None, None) == E_ARG and b"no sim bound" in err()
    assert L.mpc_contact_extend(None, p, 64, q, None) == E_ARG and L.mpc_contact_extend(h, None, 64, q, None) == E_ARG and b"null" in err()
    for wp in (0, 8, 63, 65, 72, -16, 65552):
        assert L.mpc_contact_extend(h, p, wp, q, None) == E_ARG and b"multiple of 16" in err(), wp
    assert L.mpc_contact_extend(h, odd, 64, q, None) == E_ARG and b"16-byte aligned" in err()
    assert L.mpc_contact_extend(h, p, 64, odd + 0x4000, None) == E_ARG and b"16-byte aligned" in err()
    assert L.mpc_contact_extend(h, p, 64, p, None) == E_ARG and b"distinct" in err()
    assert L.mpc_contact_extend(h, p, 64, p + 4 * (4 * 64 - 4), None) == E_ARG and b"distinct" in err()
    assert L.mpc_contact_extend(h, p, 64, p + 4 * 4 * 64, None) == E_ARG and b"no sim bound" in err()
    assert L.mpc_contact_summary(h, None, None) == E_ARG and L.mpc_contact_summary(h, p, None) == E_ARG and b"no sim bound" in err()
    assert L.mpc_contact_new_window(None, None) == E_ARG and L.mpc_contact_new_window(h, None) == E_ARG and b"no sim bound" in err()
    assert L.mpc_contact_arrays(h, *[C.byref(C.c_void_p()) for _ in range(3)]) == E_ARG and b"no sim bound" in err()
    L.mpc_contact_destroy(h)
    L.mpc_contact_destroy(None)


def test_the_task_refuses_before_the_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "need_gpu", lambda *a, **k: (_ for _ in ()).throw(_lib.MpcLibraryError("device asked for")))
    T, S = CT.ContactTerms, CT.ContactSpec(feet_slip=-0.1)
    fr = lambda n=4: friction.Friction(n, mu=0.2)

    class Priv:                                                               # (privileged observations as the validation pass sees them)
        n, plant = 4, False
    with pytest.raises(ValueError, match="the contact terms hold 8 environments, robot_type 4"):
        rl_task.BatchedRLTask([0] * 4, [0] * 4, friction=fr(), contact_terms=T(8, S))
    for other in (rl_task.TaskConfig(dt=0.005), rl_task.TaskConfig(clip_observations=4.0), rl_task.TaskConfig(episode_length_s=10.0)):
        with pytest.raises(ValueError, match="contact_terms was made under another TaskConfig"):
            rl_task.BatchedRLTask([0] * 4, [0] * 4, friction=fr(), contact_terms=T(4, S, cfg=other))
        with pytest.raises(_lib.MpcLibraryError, match="device asked for"):
            rl_task.BatchedRLTask([0] * 4, [0] * 4, cfg=other, friction=fr(), contact_terms=T(4, S, cfg=other))
    with pytest.raises(ValueError, match="give friction="):
        rl_task.BatchedRLTask([0] * 4, [0] * 4, contact_terms=T(4, S))
    with pytest.raises(ValueError, match="privileged=True"):
        rl_task.BatchedRLTask([0] * 4, [0] * 4, friction=fr(), contact_terms=T(4, S, privileged=True))
    with pytest.raises(_lib.MpcLibraryError, match="device asked for"):        # with the row to widen it passes the refusal pass
        rl_task.BatchedRLTask([0] * 4, [0] * 4, friction=fr(), privileged_obs=Priv(), contact_terms=T(4, S, privileged=True))
    with pytest.raises(_lib.MpcLibraryError, match="device asked for"):
        rl_task.BatchedRLTask([0] * 4, [0] * 4, friction=fr(), contact_terms=T(4, S))

    class Sim:
        _handle, n, device = None, 4, None
    with pytest.raises(_lib.MpcLibraryError, match="device asked for"):        # the class itself needs the device from bind on
        T(4, S).bind(Sim())


def test_the_trainers_rider():
    from rl_mpc_locomotion_amd import ppo

    class Unit:
        windows = 0

        def __init__(self, values, record):
            self.values, self.record = values, record

        def summary(self):
            return torch.tensor(self.values, dtype=torch.float64)

        def new_window(self):
            self.windows += 1

    class Trainer:
        alg = type("Alg", (), {"lr_device": None, "learning_rate": 1e-3})()
        curriculum = episode_terms = None
        episode_stats = type("Stats", (), {"summary": torch.zeros(8, dtype=torch.float64)})()
        _scalars = torch.zeros(5, dtype=torch.float64)
        reward_shaping = Unit([2.0, 4.0, 0, 0, 0, 0, 0, 0, -8.0, 2.0], reward_shaping.RewardShaping.record)
    plain = ppo._read_riders(ppo._riders(Trainer()))
    assert "contact_terms" not in plain and list(plain)[-1] == "reward_shaping"  # a trainer without the attribute reads as before
    Trainer.contact_terms = Unit([2.0, -4.0, 0.0, 6.0, 2.0], CT.ContactTerms.record)
    record = ppo._read_riders(ppo._riders(Trainer()))
    assert list(record)[:len(plain)] == list(plain) and list(record)[-1] == "contact_terms" and record["reward_shaping"] == plain["reward_shaping"]
    assert record["contact_terms"] == {"rew_feet_slip": -1.0, "rew_feet_contact_forces": 0.0, "rew_feet_stumble": 1.5}
    assert Trainer.contact_terms.windows == 1 and Trainer.reward_shaping.windows == 2


def test_refusals_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/contact_terms_refusals_main.cpp, a stand-alone program over the unit's host paths, built with AddressSanitizer and UBSan on the host code
    and run directly: every create refusal, every argument check of a handle that has no sim, the binds that are refused."""
    exe = tmp_path / "contact_terms_refusals"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-x", "hip",
                    os.path.join(ROOT, "tools", "contact_terms_refusals_main.cpp"), os.path.join(CSRC, "mpc_contact_terms.hip"), "-o", str(exe)], check=True, cwd=CSRC)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_kernels_compile_for_gfx950_without_scratch(tmp_path, capsys):
    out = tmp_path / "mpc_contact_terms.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "mpc_contact_terms.hip"), "-o", str(out)], check=True, capture_output=True, text=True)
    found = {}
    for name, sgpr, vgpr, scratch, lds in re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                                                     r.stderr, re.S):
        found[name] = dict(sgprs=int(sgpr), vgprs=int(vgpr), scratch=int(scratch), lds=int(lds))
    with capsys.disabled():
        for name, v in found.items():
            print(f"\n  {name}: {v}", end="")
    close = 64 * 3 * 4 + 64 * 4                                            # a wave's float32 sums in rows of 3 words, and its closed flags
    join = 256 * 8 * 8                                                     # 256 staged partial rows
    for kernel, lds in (("contact_close_kernel", close), ("contact_join_kernel", join), ("contact_run_kernel", 0), ("contact_extend_kernel", 0),
                        ("contact_summary_kernel", 0)):
        hit = [v for k, v in found.items() if kernel in k]
        assert len(hit) == 1 and hit[0]["scratch"] == 0 and hit[0]["lds"] == lds, (kernel, found)
    assert len(found) == 5                                                     # exactly its named kernels
    text = open(os.path.join(CSRC, "mpc_contact_terms.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", text) and "hipFuncSetAttribute" not in text and "LdsLimit" not in text
