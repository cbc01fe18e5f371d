"""The numpy toy robots (tests/toy_sim.py on the plane, tests/toy_terrain.py on a height field) with a Coulomb friction cone on the plant side: the
model that csrc/toy_sim.h's Coulomb contact (toy_step_friction) restates (TEST ONLY).

The parents' ``step`` is restated here with ONE change, in the stance branch, after the lift-off tests and before ``F += f``::

    ft  = f - fn * n                 # componentwise
    ftn = sqrt(ft . ft)
    lim = mu * fn
    if ftn > lim:                    # NaN (mu = inf, fn = 0) compares false: the foot sticks
        t   = ft / ftn
        f   = fn * n + lim * t       # what the ground can supply; the body gets this
        d   = h * ((ftn - lim) / SLIP_DAMP)
        a   = anchor[l] - d * t ;  a[2] = ground(a) ;  anchor[l] = a
        slip[l] += d
    F += f ;  T += cross(R (hiploc + p), f) ;  force[l] = f

The lever arm is the foot's position before the slide; on a height field the normal is the one under the anchor before the slide; the substep's
closing inverse kinematics follows the moved anchor.  ``force`` [4, 3] is the world-frame ground reaction of the tick's last substep (zero for a leg
in the air, a leg that let go and a leg with fn < 0), ``slip`` [4] the distance slid over the tick's substeps.  With ``mu = inf`` the step is the
parents', bit for bit.

``step(tau, dt, log=list)`` appends one entry per stance leg-substep that reached the cone test: (leg, ftn, lim, slid, anchor before, t, d, anchor
after, pushes); the four before the last are None for a foot that stuck, and ``pushes`` is False for a leg whose torques, and so its force, are
exactly zero.
"""
import numpy as np

from tests import toy_sim as TS
from tests.toy_sim import B_J, I_J, LIFT_TICKS, RELEASE_N, SIDE, SUBSTEPS, ToyRobot, leg_fk_jac, quat_mul, quat_to_rot
from tests.toy_terrain import ToyTerrainRobot

SLIP_DAMP = 200.0                      # csrc/toy_sim.h's kSlipDamp [N s/m]


class _Friction:
    mu = np.inf

    def _tick_normal(self):
        """The normal every leg of this tick shares, or None where each leg looks up its own."""
        raise NotImplementedError

    def _leg_normal(self, l):
        raise NotImplementedError

    def step(self, tau, dt=0.01, log=None):
        tau = np.asarray(tau, dtype=np.float64).reshape(4, 3)
        h = dt / SUBSTEPS
        mu = float(self.mu)
        rec = log.append if log is not None else (lambda m: None)
        shared = self._tick_normal()
        self.slip = np.zeros(4)
        for _ in range(SUBSTEPS):
            self.force = np.zeros((4, 3))
            R = quat_to_rot(self.quat)
            F = np.zeros(3)
            T = np.zeros(3)
            pj = [leg_fk_jac(self.q[l], SIDE[l], self.abad, self.hip, self.knee) for l in range(4)]
            for l in range(4):
                if not self.contact[l]:
                    continue
                p, J = pj[l]
                f = -R @ np.linalg.solve(J.T + 1e-9 * np.eye(3), tau[l])
                n = shared if shared is not None else self._leg_normal(l)
                fn = f @ n
                if fn < -RELEASE_N:               # the leg pulls on the ground (a swing command): it lets go
                    self.contact[l] = False
                    self.lift[l] = LIFT_TICKS * SUBSTEPS
                    continue
                if fn < 0.0:                      # (unilateral contact: no pull, but not yet a lift-off either)
                    continue
                pushes = bool(f.any())            # (False: the leg's torques are exactly zero, and so are f, ftn and lim)
                ft = f - fn * n
                ftn = np.sqrt(ft[0] * ft[0] + ft[1] * ft[1] + ft[2] * ft[2])
                with np.errstate(invalid="ignore"):
                    lim = mu * fn
                if ftn > lim:                     # beyond the cone: the ground supplies the limit and the foot slides
                    t = ft / ftn
                    f = fn * n + lim * t
                    d = h * ((ftn - lim) / SLIP_DAMP)
                    before = self.anchor[l].copy()
                    a = self.anchor[l] - d * t
                    a[2] = self.ground(a)
                    self.anchor[l] = a
                    self.slip[l] = self.slip[l] + d
                    rec((l, float(ftn), float(lim), True, before, t.copy(), float(d), a.copy(), pushes))
                else:
                    rec((l, float(ftn), float(lim), False, None, None, None, None, pushes))
                F += f
                T += np.cross(R @ (self.hiploc[l] + p), f)
                self.force[l] = f
            Iw = R @ np.diag(self.inertia) @ R.T
            self.v = self.v + h * (TS.GRAV + F / self.mass)
            self.w = self.w + h * np.linalg.solve(Iw, T - np.cross(self.w, Iw @ self.w))
            self.pos = self.pos + h * self.v
            ang = np.linalg.norm(self.w) * h
            ax = self.w / max(np.linalg.norm(self.w), 1e-12)
            dq = np.concatenate([ax * np.sin(ang / 2), [np.cos(ang / 2)]])
            self.quat = quat_mul(dq, self.quat)
            self.quat /= np.linalg.norm(self.quat)
            R2 = quat_to_rot(self.quat)
            for l in range(4):
                if self.contact[l]:
                    qn = self._ik(l, R2.T @ (self.anchor[l] - self.pos) - self.hiploc[l], self.q[l])
                    self.qd[l] = (qn - self.q[l]) / h
                    self.q[l] = qn
                    continue
                p_old = R @ (self.hiploc[l] + pj[l][0]) + (self.pos - h * self.v)      # (world foot position before the substep)
                self.qd[l] = self.qd[l] + h * (tau[l] - B_J * self.qd[l]) / I_J
                self.q[l] = self.q[l] + h * self.qd[l]
                if self.lift[l] > 0:
                    self.lift[l] -= 1
                    continue
                p_new = self.pos + R2 @ (self.hiploc[l] + leg_fk_jac(self.q[l], SIDE[l], self.abad, self.hip, self.knee)[0])
                d_old, d_new = p_old[2] - self.ground(p_old), p_new[2] - self.ground(p_new)
                if d_new <= 0.0:                  # touch-down: the anchor is where the foot path crosses the ground
                    s = 1.0 if d_old <= 0.0 else d_old / (d_old - d_new)
                    a = p_old + s * (p_new - p_old)
                    a[2] = self.ground(a)
                    self.anchor[l] = a
                    self.contact[l] = True
                    self.q[l] = self._ik(l, R2.T @ (a - self.pos) - self.hiploc[l], self.q[l])
                    self.qd[l] = 0.0
        if not np.all(np.isfinite(self.pos)) or quat_to_rot(self.quat)[2, 2] < 0.3 or abs(self.pos[2] - self.ground(self.pos)) > 3 * self.height:
            self.fell = True


class ToyFrictionRobot(_Friction, ToyRobot):
    def __init__(self, table_row, yaw0=0.0, slope=(0.0, 0.0), mu=np.inf):
        super().__init__(table_row, yaw0=yaw0, slope=slope)
        self.mu = float(mu)
        self.force, self.slip = np.zeros((4, 3)), np.zeros(4)

    def _tick_normal(self):
        n = np.array([-self.slope[0], -self.slope[1], 1.0])
        n /= np.linalg.norm(n)
        return n


class ToyFrictionTerrainRobot(_Friction, ToyTerrainRobot):
    def __init__(self, table_row, terrain, origin=(0.0, 0.0), yaw0=0.0, mu=np.inf):
        super().__init__(table_row, terrain, origin=origin, yaw0=yaw0)
        self.mu = float(mu)
        self.force, self.slip = np.zeros((4, 3)), np.zeros(4)

    def _tick_normal(self):
        return None

    def _leg_normal(self, l):
        return self.ground_normal(self.anchor[l])[0]
