"""The Coulomb friction of the toy plant (csrc/toy_sim.h's Coulomb contact, csrc/friction.h, rl_mpc_locomotion_amd.friction) on the CPU: the headers
are compiled with g++ into a small shim and driven through ctypes, against the numpy restatements tests/toy_friction.py and tests/friction_ref.py.

Tolerances are tests/test_toy_sim.py's (1e-9 for pos, quat, q and anchor; 1e-7 for v, w and qd); the force agrees within 1e-9 * max(1 N, |f|) and
the slip within 1e-12 m.  The tests assert about their own inputs that both branches of the cone test are reached and that no decision is a tie
(|ftn - lim| <= 1e-9 * max(1, ftn)), so a disagreement cannot hide behind one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, friction as FR, terrain as TR
from rl_mpc_locomotion_amd.quadruped import ROBOT_TABLE64
from tests import friction_ref as fref, toy_friction as TF
from tests.helpers import ROOT
from tests.plant_rand_ref import POS_LIKE, VEL_LIKE, from_record, to_record
from tests.toy_sim import SIDE, leg_fk_jac, quat_to_rot

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "closed_loop_h10.npz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
E_ARG = -1
TOL_POS, TOL_VEL, TOL_FORCE, TOL_SLIP, TIE = 1e-9, 1e-7, 1e-9, 1e-12, 1e-9
MUS = (0.0, 0.2, 0.4, 1.0)
CASES = ("aliengo_trot_flat", "aliengo_trot_slope", "go1_trot_flat")

SHIM = r"""
#include "friction.h"
#include "toy_sim.h"
using namespace toysim;
struct Field { const short *h; int rows, cols; double hscale, vscale, x0, y0; };
static HeightField field(const Field *t, double ox, double oy) { return HeightField{t->h, t->rows, t->cols, t->hscale, t->vscale, t->x0, t->y0, ox, oy}; }
static void out(const Coulomb &c, double *force, double *slip) {
  for (int l = 0; l < 4; ++l) { slip[l] = c.slip[l]; for (int i = 0; i < 3; ++i) force[3 * l + i] = c.force[l][i]; }
}
extern "C" {
void shim_init(const double *row, double yaw0, double gx, double gy, double *f, int *k) {
  Params P; params_from_row(P, row);
  State s; toy_init(s, P, yaw0, gx, gy);
  pack(s, f, k, 1);
}
// mu null: the plain toy_step; else toy_step_friction with the neutral plant record
void shim_step(const double *row, double gx, double gy, double dt, const double *tau, const double *mu, double *f, int *k, double *force, double *slip) {
  Params P; params_from_row(P, row);
  State s; unpack(s, f, k, 1);
  if (mu) { Coulomb c; c.mu = *mu; toy_step_friction(s, P, tau, dt, Plane{gx, gy}, 0.0, 1.0, kGravZ, c); out(c, force, slip); }
  else toy_step(s, P, tau, dt, gx, gy);
  pack(s, f, k, 1);
}
void shim_step_field(const double *row, const Field *t, double ox, double oy, double dt, const double *tau, const double *mu, double *f, int *k, double *force,
                     double *slip) {
  Params P; params_from_row(P, row);
  State s; unpack(s, f, k, 1);
  if (mu) { Coulomb c; c.mu = *mu; toy_step_friction(s, P, tau, dt, field(t, ox, oy), 0.0, 1.0, kGravZ, c); out(c, force, slip); }
  else toy_step(s, P, tau, dt, field(t, ox, oy));
  pack(s, f, k, 1);
}
void shim_draw(int k, const int *env, unsigned long long seed, const unsigned *e, float lo, float hi, int buckets, float *mu) {
  for (int i = 0; i < k; ++i) mu[i] = friction::draw_mu(seed, (uint32_t)env[i], e[i], lo, hi, buckets);
}
int shim_range_ok(float lo, float hi, int buckets) { return friction::range_error(lo, hi, buckets) == nullptr; }
}
"""


class Field(C.Structure):
    _fields_ = [("h", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("hscale", C.c_double), ("vscale", C.c_double), ("x0", C.c_double),
                ("y0", C.c_double)]


def field_of(t):
    return Field(t.heights.ctypes.data, t.rows, t.cols, t.hscale, t.vscale, t.x0, t.y0)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("friction_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    vp, cd, ci, cf = C.c_void_p, C.c_double, C.c_int, C.c_float
    L.shim_init.argtypes, L.shim_init.restype = [vp, cd, cd, cd, vp, vp], None
    L.shim_step.argtypes, L.shim_step.restype = [vp, cd, cd, cd, vp, vp, vp, vp, vp, vp], None
    L.shim_step_field.argtypes, L.shim_step_field.restype = [vp, vp, cd, cd, cd, vp, vp, vp, vp, vp, vp], None
    L.shim_draw.argtypes, L.shim_draw.restype = [ci, vp, C.c_ulonglong, vp, cf, cf, ci, vp], None
    L.shim_range_ok.argtypes, L.shim_range_ok.restype = [cf, cf, ci], ci
    return L


def _row(rt):
    return np.ascontiguousarray(ROBOT_TABLE64[rt], dtype=np.float64)


def header_step(shim, rt, ground, tau, mu, f, k, dt=0.01):
    """One step of the header on record (f, k) in place; ground ("plane", gx, gy) or ("field", Field, ox, oy); mu None: the plain toy_step.
    Returns (force [4, 3], slip [4])."""
    tau64 = np.ascontiguousarray(tau, dtype=np.float64).reshape(12)
    m = None if mu is None else np.array([mu], np.float64)
    mp = None if m is None else m.ctypes.data
    force, slip = np.full((4, 3), np.nan), np.full(4, np.nan)
    if ground[0] == "plane":
        shim.shim_step(_row(rt).ctypes.data, ground[1], ground[2], dt, tau64.ctypes.data, mp, f.ctypes.data, k.ctypes.data, force.ctypes.data, slip.ctypes.data)
    else:
        shim.shim_step_field(_row(rt).ctypes.data, C.addressof(ground[1]), ground[2], ground[3], dt, tau64.ctypes.data, mp, f.ctypes.data, k.ctypes.data,
                             force.ctypes.data, slip.ctypes.data)
    return force, slip


def compare(what, f, k, force, slip, model):
    """The header's record, force and slip after one step against the model's: the module's tolerances."""
    rf, rk = to_record(model)
    assert np.array_equal(k, rk), f"{what}: contact / lift / fell {k.tolist()} against the model's {rk.tolist()}"
    dpos, dvel = float(np.abs(f[POS_LIKE] - rf[POS_LIKE]).max()), float(np.abs(f[VEL_LIKE] - rf[VEL_LIKE]).max())
    assert dpos <= TOL_POS, f"{what}: |dpos, dquat, dq, danchor| {dpos:.3e}"
    assert dvel <= TOL_VEL, f"{what}: |dv, dw, dqd| {dvel:.3e}"
    fmag = np.maximum(1.0, np.sqrt((model.force ** 2).sum(1)))
    dforce = float((np.abs(force - model.force).max(1) / fmag).max())
    assert dforce <= TOL_FORCE, f"{what}: force differs by {dforce:.3e} of max(1 N, |f|)"
    dslip = float(np.abs(slip - model.slip).max())
    assert dslip <= TOL_SLIP, f"{what}: slip differs by {dslip:.3e} m"
    return dpos, dvel, dforce, dslip


def no_tie(what, log):
    """No decision of the cone test within 1e-9 of its threshold.  A leg with exactly zero torques is no decision: its f, ftn and lim are exact zeros in
    every IEEE implementation and 0 > 0 is false in all of them (the controller commands such legs on its first ticks)."""
    for l, ftn, lim, slid, *_, pushes in log:
        if not pushes:
            assert ftn == 0.0 and lim == 0.0 and not slid
            continue
        assert not abs(ftn - lim) <= TIE * max(1.0, ftn), f"{what}: leg {l} decides on ftn {ftn!r} against lim {lim!r}"


# ---- 1. mu = inf is the old plant -------------------------------------------------------------------------------------------------------------------
def test_mu_inf_is_the_old_plant_bit_for_bit(shim):
    g = np.load(GOLD)
    names = sorted({key.split("/")[0] for key in g.files})
    assert len(names) == 6
    compared = 0
    for name in names:
        meta, tau = g[name + "/meta"], g[name + "/torque"]
        rt, ground = int(meta[0]), ("plane", float(meta[3]), float(meta[4]))
        f = np.zeros(49); k = np.zeros(9, np.int32)
        shim.shim_init(_row(rt).ctypes.data, float(meta[5]), ground[1], ground[2], f.ctypes.data, k.ctypes.data)
        ff, kf = f.copy(), k.copy()
        for tick in range(int(meta[6])):
            if k[8]:
                break
            if tick % 25 == 0:          # the unclamped f of the last substep: the model's at mu = inf, which logs that no foot slid
                m = from_record(TF.ToyFrictionRobot(ROBOT_TABLE64[rt], yaw0=float(meta[5]), slope=ground[1:]), f, k)
                log = []
                m.step(tau[tick], log=log)
                assert not any(e[3] for e in log)
            header_step(shim, rt, ground, tau[tick], None, f, k)
            force, slip = header_step(shim, rt, ground, tau[tick], np.inf, ff, kf)
            assert np.array_equal(f, ff) and np.array_equal(k, kf), f"{name}, tick {tick}"
            assert (slip == 0).all() and np.isfinite(force).all()
            assert ((force == 0).all(1) | (k[:4] != 0)).all()          # (a leg in the air has no force)
            if tick % 25 == 0:
                fmag = np.maximum(1.0, np.sqrt((m.force ** 2).sum(1)))
                assert (np.abs(force - m.force).max(1) <= TOL_FORCE * fmag).all(), f"{name}, tick {tick}"
                compared += int((m.force != 0).any(1).sum())
    assert compared >= 100


# ---- 2. the header against the numpy model, single steps in closed loop ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def closed_loop(shim):
    """Every (case, mu): the model in closed loop with the emulated controller for at most 100 ticks, ending at the first fall; every tick the
    header starts from the model's state.  Returns the rows (case, mu, tick, n, header force, header slip, header anchors, log) and the counts."""
    from tests.emu import emu
    g = np.load(GOLD)
    rows, slipping, sticking, worst = [], 0, 0, np.zeros(4)
    for name in CASES:
        meta = g[name + "/meta"]
        rt, ground = int(meta[0]), ("plane", float(meta[3]), float(meta[4]))
        for mu in MUS:
            ctrl = emu.EmuLocomotion([rt], [int(meta[1])], flat_ground=bool(meta[2]), nthreads=1)
            model = TF.ToyFrictionRobot(ROBOT_TABLE64[rt], yaw0=float(meta[5]), slope=ground[1:], mu=mu)
            n = model._tick_normal()
            for tick in range(100):
                if model.fell:
                    break
                dof, body = model.observe()
                tau = ctrl.run(dof[None], body[None], g[name + "/cmd"][None])[0]
                f, k = to_record(model)
                force, slip = header_step(shim, rt, ground, tau, mu, f, k)
                log = []
                model.step(tau, log=log)
                what = f"{name}, mu {mu}, tick {tick}"
                no_tie(what, log)
                worst = np.maximum(worst, compare(what, f, k, force, slip, model))
                slipping += sum(e[3] for e in log)
                sticking += sum(not e[3] and e[8] for e in log)
                rows.append((name, mu, tick, n, force, slip, f[37:49].reshape(4, 3).copy(), log, ground))
    print(f"{len(rows)} steps: {slipping} slipping and {sticking} sticking leg-substeps; worst |dpos| {worst[0]:.2e}, |dvel| {worst[1]:.2e}, "
          f"force {worst[2]:.2e}, slip {worst[3]:.2e} m")
    return rows, slipping, sticking


def test_header_equals_the_numpy_model_in_closed_loop(closed_loop):
    rows, slipping, sticking = closed_loop                                      # (the comparisons ran, and asserted, in the fixture)
    assert {(r[0], r[1]) for r in rows} == {(c, m) for c in CASES for m in MUS}
    assert slipping >= 20 and sticking >= 100


# ---- 3. properties ------------------------------------------------------------------------------------------------------------------------------------
def test_forces_stay_in_the_cone_and_slides_follow_the_rule(closed_loop):
    rows, _, _ = closed_loop
    nonzero = slides = 0
    for name, mu, tick, n, force, slip, anchors, log, ground in rows:
        what = f"{name}, mu {mu}, tick {tick}"
        for l in range(4):
            f = force[l]
            if not f.any():
                continue
            nonzero += 1
            fn = f @ n
            ft = f - fn * n
            assert fn >= 0.0, what
            if mu == 0.0:
                # the header's force is fn * n + 0 * t = fn * n exactly; on the flat plane n = (0, 0, 1) and x, y are exactly zero, on the slope
                # THIS decomposition's own subtraction leaves a rounding of a few ulp of |f|, which a bound of 0 * fn cannot hold
                if ground[1] == 0.0 and ground[2] == 0.0:
                    assert f[0] == 0.0 and f[1] == 0.0, what
                else:
                    assert np.sqrt(ft @ ft) <= 4 * np.finfo(np.float64).eps * np.sqrt(f @ f), what
            else:
                assert np.sqrt(ft @ ft) <= mu * fn * (1 + 1e-12), f"{what}: leg {l} |ft| {np.sqrt(ft @ ft)!r}, mu fn {mu * fn!r}"
        # the model's slides: the anchor moves along -t by exactly d and stays on the ground; the header's anchors are the model's (test 2)
        for l, ftn, lim, slid, before, t, d, after, _ in log:
            if not slid:
                continue
            slides += 1
            assert d > 0 and d == 0.0025 * ((ftn - lim) / TF.SLIP_DAMP)
            assert after[0] == before[0] - d * t[0] and after[1] == before[1] - d * t[1]
            assert after[2] == ground[1] * after[0] + ground[2] * after[1]
        for l in range(4):                                                       # the header's anchors lie on the plane, to the tolerance of its own product sum
            a = anchors[l]
            assert abs(a[2] - (ground[1] * a[0] + ground[2] * a[1])) <= 1e-15 * max(1.0, abs(a[0]) + abs(a[1]))
    print(f"{nonzero} nonzero force rows, {slides} slides")
    assert nonzero >= 1000 and slides >= 20


def _pushing_torque(m, f_world):
    """The joint torques with which every leg of m pushes the body with f_world: tau = -J^T R^T f."""
    R = quat_to_rot(m.quat)
    return np.stack([-leg_fk_jac(m.q[l], SIDE[l], m.abad, m.hip, m.knee)[1].T @ (R.T @ f_world) for l in range(4)])


def test_a_slide_on_a_height_field_lands_on_the_field_and_can_cross_a_cell_diagonal(shim):
    # tests/toy_terrain.py's surface field at a fifteenth of its amplitude (+-0.02 m on the 0.1 m grid: every stance is within reach); x0 == y0
    t = TR.Terrain(np.random.default_rng(64048).integers(-4, 5, (64, 48)).astype(np.int16), 0.1, 0.005, -1.7, -1.7)
    fd = field_of(t)
    rt, mu = 0, 0.2
    crossed = slid = 0
    # an anchor's local x, y do not depend on the origin, and with x0 == y0 a cell's diagonal is where x - y (field frame) is a multiple of the grid:
    # the origin puts one leg's anchor `gap` to the side of a diagonal from which the push below slides it across (about 3e-4 m of x - y per substep)
    local = TF.ToyFrictionTerrainRobot(ROBOT_TABLE64[rt], t, (1.45, 1.45), yaw0=0.3).anchor
    for i, (leg, gap) in enumerate((l, gap) for l in range(4) for gap in (1e-4, 5e-4, 2e-2)):
        origin = (1.45, 1.45 + (local[leg, 0] - local[leg, 1]) - gap)
        m = TF.ToyFrictionTerrainRobot(ROBOT_TABLE64[rt], t, origin, yaw0=0.3, mu=mu)
        assert m.ik_residual < 1e-9
        tau = _pushing_torque(m, np.array([30.0, -10.0, 60.0]))
        f, k = to_record(m)
        force, slip = header_step(shim, rt, ("field", fd, origin[0], origin[1]), tau, mu, f, k)
        log = []
        m.step(tau, log=log)
        what = f"origin {i}"
        no_tie(what, log)
        compare(what, f, k, force, slip, m)
        anchors = f[37:49].reshape(4, 3)
        for l in range(4):
            if k[l]:
                assert anchors[l, 2] == t.height(float(anchors[l, 0]), float(anchors[l, 1]), origin), what          # the header's anchor, the field's height there
        for l, ftn, lim, s, before, tt, d, after, _ in log:
            if not s:
                continue
            slid += 1
            assert after[0] == before[0] - d * tt[0] and after[1] == before[1] - d * tt[1] and after[2] == m.ground(after)
            up0, up1 = m.ground_normal(before)[2], m.ground_normal(after)[2]
            ij0, ij1 = t.cell(float(before[0]), float(before[1]), origin)[:2], t.cell(float(after[0]), float(after[1]), origin)[:2]
            crossed += int(up0 != up1 and tuple(ij0) == tuple(ij1))
    print(f"{slid} slides on the field, {crossed} across a cell diagonal")
    assert slid >= 24 and crossed >= 4


def test_mu_zero_on_the_flat_plane_gives_a_purely_normal_force(shim):
    m = TF.ToyFrictionRobot(ROBOT_TABLE64[2], yaw0=0.7, mu=0.0)
    tau = _pushing_torque(m, np.array([25.0, 15.0, 40.0]))
    f, k = to_record(m)
    force, slip = header_step(shim, 2, ("plane", 0.0, 0.0), tau, 0.0, f, k)
    m.step(tau)
    assert (force[:, :2] == 0).all() and (force[:, 2] > 30).all() and (slip > 0).all()
    assert (m.force[:, :2] == 0).all() and np.abs(slip - m.slip).max() <= TOL_SLIP


# ---- 4. the draw ------------------------------------------------------------------------------------------------------------------------------------------
def host_draw(shim, env, seed, e, lo, hi, buckets):
    env = np.ascontiguousarray(env, dtype=np.int32)
    e = np.ascontiguousarray(np.broadcast_to(np.asarray(e, dtype=np.uint32), env.shape))
    mu = np.full(len(env), np.nan, np.float32)
    shim.shim_draw(len(env), env.ctypes.data, seed, e.ctypes.data, lo, hi, buckets, mu.ctypes.data)
    return mu


@pytest.mark.parametrize("buckets", [0, 2, 64])
@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
def test_draws_equal_the_restatement_bit_for_bit(shim, seed, buckets):
    env = np.arange(257)
    lo, hi = 0.5, 1.25
    for e in (0, 1, 2):
        mu = host_draw(shim, env, seed, e, lo, hi, buckets)
        assert mu.tobytes() == fref.draw_mu(seed, env, e, lo, hi, buckets).tobytes()
        assert (mu >= np.float32(lo)).all() and (mu <= np.float32(hi)).all()
        if buckets:
            levels = np.float32(lo) + (np.float32(hi) - np.float32(lo)) * np.arange(buckets, dtype=np.float32) / np.float32(buckets - 1)
            assert np.isin(mu, np.minimum(levels, np.float32(hi))).all() and len(np.unique(mu)) == min(buckets, len(np.unique(mu)))
            assert len(np.unique(mu)) >= min(buckets, 40)
        else:
            assert len(np.unique(mu)) > 250
    a, b = host_draw(shim, env, seed, 0, lo, hi, buckets), host_draw(shim, env, seed, 1, lo, hi, buckets)
    assert not np.array_equal(a, b)


def test_draw_edge_cases(shim):
    env = np.arange(257)
    for buckets in (0, 2, 64):
        assert (host_draw(shim, env, 3, 1, 0.75, 0.75, buckets) == np.float32(0.75)).all()                  # lo == hi gives exactly lo
        assert (host_draw(shim, env, 3, 1, 0.0, 0.0, buckets) == 0).all()
    # a draw depends on (seed, environment, draw index) alone: not on the batch it is made in
    small, large = host_draw(shim, np.arange(64), 3, 2, 0.5, 1.25, 64), host_draw(shim, env, 3, 2, 0.5, 1.25, 64)
    assert small.tobytes() == large[:64].tobytes()
    assert host_draw(shim, [200, 5], 3, [2, 2], 0.5, 1.25, 64).tobytes() == large[[200, 5]].tobytes()
    for lo, hi, buckets, ok in ((0.5, 1.25, 64, 1), (0.0, 0.0, 0, 1), (1.0, 0.5, 0, 0), (-0.1, 1.0, 0, 0), (np.nan, 1.0, 0, 0), (0.0, np.inf, 0, 0),
                                (0.5, 1.25, 1, 0), (0.5, 1.25, -2, 0), (0.5, 1.25, 2, 1)):
        assert shim.shim_range_ok(lo, hi, buckets) == ok, (lo, hi, buckets)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_spec_refusals():
    S = FR.FrictionSpec
    S().validate()
    assert S().range == (0.5, 1.25) and S().buckets == 64 and S().resample == "once"
    for spec, msg in ((S(range=(1.0, 0.5)), "lo > hi"), (S(range=(-0.1, 1.0)), "lo >= 0"), (S(range=(np.nan, 1.0)), "finite"), (S(range=(0.0, np.inf)), "finite"),
                      (S(range=(0.0, 1e39)), "finite"), (S(range=(0.0, 1.0, 2.0)), "finite"), (S(buckets=1), "buckets"), (S(buckets=-4), "buckets"),
                      (S(resample="sometimes"), "resample")):
        with pytest.raises(ValueError, match=msg):
            spec.validate()
        with pytest.raises(ValueError, match=msg):
            FR.Friction(4, spec)
    S(range=(0.0, 0.0), buckets=0, resample="reset").validate()
    for mu, msg in (([0.4, -0.1, 1.0, 1.0], "negative or NaN"), ([0.4, np.nan, 1.0, 1.0], "negative or NaN"), ([0.4, 0.4], r"\[4\]")):
        with pytest.raises(ValueError, match=msg):
            FR.Friction(4, mu=mu)
    FR.Friction(4, mu=[0.0, np.inf, 0.4, 1.0])
    FR.Friction(4, mu=0.4)
    with pytest.raises(ValueError, match="at least 1"):
        FR.Friction(0)
    fr = FR.Friction(4)
    with pytest.raises(ValueError, match="holds 4 environments, the task 5"):
        fr.validate(n=5)
    with pytest.raises(ValueError, match="not bound"):
        fr.get_mu()


def test_task_refusals_come_before_the_device(monkeypatch):
    from rl_mpc_locomotion_amd import rl_task as R

    def reached(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(R._lib, "need_gpu", reached)
    with pytest.raises(ValueError, match="friction holds 3 environments, the task 4"):
        R.BatchedRLTask([0] * 4, [0] * 4, friction=FR.Friction(3))
    fr = FR.Friction(4, FR.FrictionSpec())
    fr.spec.buckets = 1
    with pytest.raises(ValueError, match="buckets"):
        R.BatchedRLTask([0] * 4, [0] * 4, friction=fr)
    with pytest.raises(AssertionError, match="the device was asked for"):      # a valid one passes the refusal pass
        R.BatchedRLTask([0, 1, 2, 0], [0] * 4, friction=FR.Friction(4, FR.FrictionSpec(resample="reset")))


def test_abi_symbols_and_refusals_without_a_gpu():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "mpc_friction.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mpc_friction_[a-z_]+)\s*\(", header)))
    assert names == sorted(FR.SYMBOLS) and len(names) == 10
    assert not set(FR.SYMBOLS) & set(_lib.SYMBOLS)
    L = FR.lib()
    err = L.mpc_friction_last_error
    h = C.c_void_p()
    assert L.mpc_friction_attach(None, None, None, None) == E_ARG and b"null sim" in err()
    assert L.mpc_friction_create(None, 4, 0) == E_ARG and b"null" in err()
    assert L.mpc_friction_create(C.byref(h), 0, 0) == E_ARG and b"n must be" in err() and not h.value
    assert L.mpc_friction_create(C.byref(h), 4, 7) == 0 and h.value                                        # a host-only handle
    assert L.mpc_friction_bind(None, 0x1000) == E_ARG and b"null handle" in err()
    assert L.mpc_friction_bind(h, None) == E_ARG and b"null sim" in err()
    assert L.mpc_friction_draw(h, None, 4, 1.0, 0.5, 0, 1, None) == E_ARG and b"lo > hi" in err()
    assert L.mpc_friction_draw(h, None, 4, 0.5, 1.25, 1, 1, None) == E_ARG and b"buckets" in err()
    assert L.mpc_friction_draw(h, None, 4, -1.0, 1.25, 0, 1, None) == E_ARG and b"lo >= 0" in err()
    assert L.mpc_friction_draw(h, None, 4, 1.0, 0.5, 1, 0, None) == E_ARG and b"no sim bound" in err()     # (the range is not read without resample)
    assert L.mpc_friction_draw(h, None, 3, 0.5, 1.25, 64, 1, None) == E_ARG and b"k must be n" in err()
    assert L.mpc_friction_draw(None, None, 4, 0.5, 1.25, 64, 1, None) == E_ARG and b"null handle" in err()
    assert L.mpc_friction_get_mu(h, 0x1000) == E_ARG and b"no sim bound" in err()
    mu = (C.c_double * 4)(0.4, 0.4, -1.0, 0.4)
    assert L.mpc_friction_set_mu(h, mu) == E_ARG and b"robot 2" in err()
    assert L.mpc_friction_get_counters(None, 0x1000) == E_ARG and L.mpc_friction_set_counters(h, 0x1000) == E_ARG
    L.mpc_friction_destroy(h)
    L.mpc_friction_destroy(None)


def test_refusals_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/friction_refusals_main.cpp, a stand-alone program over the unit's host paths, built with AddressSanitizer and UBSan on the host code and
    run directly: negative and NaN mu, lo > hi, buckets == 1, a second attach and a wrong n, among the others."""
    exe = tmp_path / "friction_refusals"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-x", "hip",
                    os.path.join(ROOT, "tools", "friction_refusals_main.cpp"), os.path.join(CSRC, "mpc_friction.hip"), "-o", str(exe)], check=True, cwd=CSRC)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_classes_raise_without_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fr = FR.Friction(8)                                                          # host state only

    class Sim:
        _handle = None
        n = 8
    with pytest.raises(_lib.MpcLibraryError):
        fr.bind(Sim())


# ---- 6. the kernels -------------------------------------------------------------------------------------------------------------------------------------
def test_friction_kernels_cross_compile_without_scratch(tmp_path):
    s = tmp_path / "mpc_friction.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", os.path.join(CSRC, "mpc_friction.hip"),
                    "-o", str(s)], check=True, capture_output=True)
    text = s.read_text()
    kernels = re.findall(r"^(_Z\w*friction_\w+_kernel\w*):", text, flags=re.M)
    assert len(kernels) == 3 and all(any(part in k for k in kernels) for part in ("friction_draw_kernel", "friction_step_plane_kernel", "friction_step_field_kernel")), kernels
    for k in kernels:
        body = text.split(k + ":", 1)[1].split(".Lfunc_end", 1)[0]
        assert "scratch_" not in body and "buffer_" not in body, f"scratch access in {k}"
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(sizes) == 3 and all(v == "0" for v in sizes) and len(spills) == 3 and all(v == "0" for v in spills)
