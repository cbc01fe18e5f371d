"""A numpy restatement of the per-robot plant randomisation (csrc/plant_rand.h, csrc/toy_sim.h's toy_step_plant, the plant columns of
csrc/privileged_obs.h), written from the formulas of the issue and of the headers' heads, not from their code (TEST ONLY):

* the toy robot with a plant record -- ``mass + payload``, ``tau * strength``, its own gravity -- as subclasses of the numpy models of the plane
  (tests/toy_sim.py) and of the height field (tests/toy_terrain.py): the record is applied around the parent's own ``step``, whose statements
  stay the model;
* the draw, on tests/domain_rand_ref.py's mix64 / uniform01;
* the three privileged columns;
and what the CPU and the GPU tests share: the hand-set records and the comparison of one step.
"""
import contextlib
import copy

import numpy as np

from tests import toy_sim as TS, toy_terrain as TT
from tests.domain_rand_ref import uniform01

F = np.float32
GRAV_Z = -9.81
NEUTRAL = (0.0, 1.0, GRAV_Z)
DOM_PLANT = 0x4452504C414E5458
TIE = 1e-9
TOL_POS, TOL_VEL = 1e-9, 1e-7          # tests/test_toy_sim.py's
POS_LIKE = np.r_[0:7, 13:25, 37:49]
VEL_LIKE = np.r_[7:13, 25:37]


@contextlib.contextmanager
def gravity(grav_z):
    """The models read their modules' GRAV: (0, 0, grav_z) while a robot with a plant record steps."""
    old = TS.GRAV, TT.GRAV
    TS.GRAV = TT.GRAV = np.array([0.0, 0.0, float(grav_z)])
    try:
        yield
    finally:
        TS.GRAV, TT.GRAV = old


class _Plant:
    plant = NEUTRAL                    # (payload, strength, grav_z)

    def step(self, tau, dt=0.01, **kw):
        payload, strength, grav_z = (float(v) for v in self.plant)
        tau = np.asarray(tau, dtype=np.float64).reshape(4, 3) * strength
        nominal = self.mass
        self.mass = nominal + payload
        try:
            with gravity(grav_z):
                super().step(tau, dt, **kw)
        finally:
            self.mass = nominal


class PlantRobot(_Plant, TS.ToyRobot):
    def __init__(self, table_row, yaw0=0.0, slope=(0.0, 0.0), plant=NEUTRAL):
        super().__init__(table_row, yaw0=yaw0, slope=slope)
        self.plant = tuple(float(v) for v in plant)


class PlantTerrainRobot(_Plant, TT.ToyTerrainRobot):
    def __init__(self, table_row, terrain, origin=(0.0, 0.0), yaw0=0.0, plant=NEUTRAL):
        super().__init__(table_row, terrain, origin=origin, yaw0=yaw0)
        self.plant = tuple(float(v) for v in plant)


def decision_margin(t, tau, dt=0.01):
    """The smallest margin of a contact / fall decision of t.step(tau) under t's plant record, from the plain models' own margin functions."""
    if isinstance(t, TT.ToyTerrainRobot):
        return TT.decision_margin(t, tau, dt)                     # (a copy's step: _Plant.step applies the record)
    from tests.test_toy_sim import decision_margin as plane_margin
    payload, strength, grav_z = t.plant
    c = copy.deepcopy(t)
    c.mass = c.mass + payload
    with gravity(grav_z):
        return plane_margin(c, np.asarray(tau, dtype=np.float64) * strength, dt)


def ik_residual(t):
    """The largest |anchor - foot| [m] over t's legs in contact: what the last inverse-kinematics call left.  Above tests/test_toy_terrain.py's
    IK_LOST (1e-9) the robot is tumbling, its stance legs are out of reach and the Newton iterations no longer contract the few-ulp differences
    between two builds: such a state is not a mid-gait state and the 1e-9 / 1e-7 tolerances do not apply to a step from it."""
    R = TS.quat_to_rot(t.quat)
    worst = 0.0
    for l in range(4):
        if t.contact[l]:
            foot = t.pos + R @ (t.hiploc[l] + TS.leg_fk_jac(t.q[l], TS.SIDE[l], t.abad, t.hip, t.knee)[0])
            worst = max(worst, float(np.linalg.norm(t.anchor[l] - foot)))
    return worst


def to_record(t):
    f = np.concatenate([t.pos, t.quat, t.v, t.w, t.q.reshape(12), t.qd.reshape(12), t.anchor.reshape(12)]).astype(np.float64)
    k = np.concatenate([t.contact.astype(np.int32), t.lift.astype(np.int32), [int(t.fell)]]).astype(np.int32)
    return f, k


def from_record(t, f, k):
    """Load record (f [49], k [9]) into robot t."""
    f = np.asarray(f, dtype=np.float64)
    t.pos, t.quat, t.v, t.w = f[0:3].copy(), f[3:7].copy(), f[7:10].copy(), f[10:13].copy()
    t.q, t.qd, t.anchor = f[13:25].reshape(4, 3).copy(), f[25:37].reshape(4, 3).copy(), f[37:49].reshape(4, 3).copy()
    t.contact, t.lift, t.fell = np.asarray(k[:4]) != 0, np.asarray(k[4:8]).astype(int).copy(), bool(k[8])
    return t


def check_step(pre, t, f, k, tau, what):
    """One step's result (f, k) of the code under test against model t (already stepped from `pre` with tau): tests/test_toy_sim.py's tolerances
    and tie rule.  Returns (tie, |dpos|, |dvel|)."""
    rf, rk = to_record(t)
    if not (np.asarray(k) == rk).all():
        m = decision_margin(pre, tau)
        assert m < TIE, f"{what}: contact / lift / fell differ with a numpy decision margin of {m:.3e}"
        return True, 0.0, 0.0
    dpos, dvel = float(np.abs(f[POS_LIKE] - rf[POS_LIKE]).max()), float(np.abs(f[VEL_LIKE] - rf[VEL_LIKE]).max())
    assert dpos <= TOL_POS, f"{what}: |dpos, dquat, dq| {dpos:.3e}"
    assert dvel <= TOL_VEL, f"{what}: |dv, dw, dqd| {dvel:.3e}"
    return False, dpos, dvel


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------------
def draw_values(seed, env, e, ranges):
    """v [len(env), 3] float32 (NaN where the axis has no range): fminf(lo + (hi - lo) * uniform01(seed ^ DOM_PLANT, env, e, axis), hi), each
    operation in float32.  env, e broadcast ([k] arrays or scalars)."""
    env, e = np.broadcast_arrays(np.asarray(env, dtype=np.uint64), np.asarray(e, dtype=np.uint64))
    v = np.full((len(env), 3), np.nan, F)
    for a, rng in enumerate(ranges):
        if rng is None:
            continue
        lo, hi = F(rng[0]), F(rng[1])
        u = uniform01(int(seed) ^ DOM_PLANT, env, e, np.uint64(a))
        v[:, a] = np.minimum(lo + (hi - lo) * u, hi)
    return v


def draw_records(seed, env, e, ranges):
    """The records [len(env), 3] float64 after draw e: payload = v0, strength = v1, grav_z = GRAV_Z + v2; an absent axis its neutral value."""
    v = draw_values(seed, env, e, ranges).astype(np.float64)
    rec = np.empty_like(v)
    rec[:, 0] = v[:, 0] if ranges[0] is not None else NEUTRAL[0]
    rec[:, 1] = v[:, 1] if ranges[1] is not None else NEUTRAL[1]
    rec[:, 2] = GRAV_Z + v[:, 2] if ranges[2] is not None else NEUTRAL[2]
    return rec


# ---- the critic's columns -----------------------------------------------------------------------------------------------------------------------
def privileged_columns(params):
    """[n, 3] float32 of a record [n, 3] float64: one float64 subtraction (none for the first) and one conversion each."""
    p = np.asarray(params, dtype=np.float64)
    return np.stack([p[:, 0].astype(F), (p[:, 1] - 1.0).astype(F), (p[:, 2] - GRAV_Z).astype(F)], 1)


def width(P):
    return 16 * ((48 + P + 5 + 3 + 15) // 16)


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------------------
def hand_records(n, seed=5):
    """[n, 3]: every robot a different triple; payload of both signs (-1.5 .. 4 kg), strength on both sides of 1 (0.8 .. 1.25), gravity offset of
    both signs (-1.5 .. 1.5 m/s^2).  The first four rows are the corners."""
    rng = np.random.default_rng(seed)
    rec = np.stack([rng.uniform(-1.5, 4.0, n), rng.uniform(0.8, 1.25, n), GRAV_Z + rng.uniform(-1.5, 1.5, n)], 1)
    corners = np.array([[-1.5, 0.8, GRAV_Z - 1.5], [4.0, 1.25, GRAV_Z + 1.5], [-1.5, 1.25, GRAV_Z + 1.5], [4.0, 0.8, GRAV_Z - 1.5]])
    rec[:min(n, 4)] = corners[:min(n, 4)]
    return rec
