"""The numpy toy robot (tests/toy_sim.py) on a height field (rl_mpc_locomotion_amd.terrain.Terrain): the model that csrc/toy_sim.h's HeightField
instantiation of toy_init / toy_step restates (TEST ONLY).

The ground appears in two roles.  Its HEIGHT -- ToyRobot.ground, overridden here -- gives the initial stance, the touch-down test and crossing,
the anchor's z and the fall test under the base.  Its NORMAL for the lift-off test f . n is that of the triangle under the leg's ANCHOR, looked
up in the substep where it is used; ToyRobot.step computes one n from its slope before the substeps, so step is restated here with that one
change.  The robot's coordinates stay local; the terrain is sampled at local + origin.
"""
import copy

import numpy as np

from tests.toy_sim import (B_J, GRAV, I_J, LIFT_TICKS, RELEASE_N, SIDE, SUBSTEPS, ToyRobot, leg_fk_jac, quat_mul, quat_to_rot)


class ToyTerrainRobot(ToyRobot):
    def __init__(self, table_row, terrain, origin=(0.0, 0.0), yaw0=0.0):
        self.terrain = terrain
        self.origin = (float(origin[0]), float(origin[1]))
        self.ik_residual = 0.0          # the largest |anchor - foot| that an inverse kinematics call has left since this was last set to 0 [m]
        super().__init__(table_row, yaw0=yaw0, slope=(0.0, 0.0))

    def ground(self, p):
        return self.terrain.height(float(p[0]), float(p[1]), self.origin)

    def ground_normal(self, p):
        """(unit normal of the triangle under p, |fu - fv| of the lookup, whether it is the fu >= fv triangle)"""
        _, gx, gy, upper = self.terrain.surface(float(p[0]), float(p[1]), self.origin)
        _, _, fu, fv = self.terrain.cell(float(p[0]), float(p[1]), self.origin)
        n = np.array([-gx, -gy, 1.0])
        return n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), abs(fu - fv), upper

    def _ik(self, leg, target, q0, iters=4):
        q = super()._ik(leg, target, q0, iters)
        r = target - leg_fk_jac(q, SIDE[leg], self.abad, self.hip, self.knee)[0]
        self.ik_residual = max(self.ik_residual, float(np.sqrt(r @ r)))
        return q

    def step(self, tau, dt=0.01, margins=None):
        """ToyRobot.step with the per-anchor normal.  `margins`, a list, receives the operands of every decision of this step: |f.n + RELEASE_N|,
        |f.n| and the |fu - fv| of the lookup whose normal fed them, |d_new| of every touch-down test, and the fall test's two distances."""
        tau = np.asarray(tau, dtype=np.float64).reshape(4, 3)
        h = dt / SUBSTEPS
        rec = margins.append if margins is not None else (lambda m: None)
        for _ in range(SUBSTEPS):
            R = quat_to_rot(self.quat)
            F = np.zeros(3)
            T = np.zeros(3)
            pj = [leg_fk_jac(self.q[l], SIDE[l], self.abad, self.hip, self.knee) for l in range(4)]
            for l in range(4):
                if not self.contact[l]:
                    continue
                p, J = pj[l]
                f = -R @ np.linalg.solve(J.T + 1e-9 * np.eye(3), tau[l])
                n, diag, _ = self.ground_normal(self.anchor[l])
                rec(diag); rec(abs(f @ n + RELEASE_N)); rec(abs(f @ n))
                if f @ n < -RELEASE_N:            # the leg pulls on the ground (a swing command): it lets go
                    self.contact[l] = False
                    self.lift[l] = LIFT_TICKS * SUBSTEPS
                    continue
                if f @ n < 0.0:                   # (unilateral contact: no pull, but not yet a lift-off either)
                    continue
                F += f
                T += np.cross(R @ (self.hiploc[l] + p), f)
            Iw = R @ np.diag(self.inertia) @ R.T
            self.v = self.v + h * (GRAV + F / self.mass)
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
                rec(abs(d_new))
                if d_new <= 0.0:                  # touch-down: the anchor is where the foot path crosses the ground
                    s = 1.0 if d_old <= 0.0 else d_old / (d_old - d_new)
                    a = p_old + s * (p_new - p_old)
                    a[2] = self.ground(a)
                    self.anchor[l] = a
                    self.contact[l] = True
                    self.q[l] = self._ik(l, R2.T @ (a - self.pos) - self.hiploc[l], self.q[l])
                    self.qd[l] = 0.0
        tilt, off = quat_to_rot(self.quat)[2, 2], abs(self.pos[2] - self.ground(self.pos))
        rec(abs(tilt - 0.3)); rec(abs(off - 3 * self.height))
        if not np.all(np.isfinite(self.pos)) or tilt < 0.3 or off > 3 * self.height:
            self.fell = True


def decision_margin(t, tau, dt=0.01):
    """The smallest margin of a contact / fall decision of ToyTerrainRobot.step(tau) from t's state (on a copy): tests/test_toy_sim.py's
    decision_margin plus the |fu - fv| of every lookup whose normal feeds a release decision."""
    m = []
    copy.deepcopy(t).step(tau, dt, margins=m)
    m = np.asarray(m, dtype=np.float64)
    return float(np.nanmin(m)) if np.isfinite(m).any() else np.inf


def surface_test_field():
    """The 64 x 48 field of the surface tests: random heights of up to +-0.3 m, x0 == y0 so that a point with x == y has fu == fv exactly."""
    from rl_mpc_locomotion_amd.terrain import Terrain
    rng = np.random.default_rng(64048)
    return Terrain(rng.integers(-60, 61, (64, 48)).astype(np.int16), 0.1, 0.005, -1.7, -1.7)


def stance_test_field():
    """A 64 x 48 field of half the reference's amplitude (-0.1 .. 0 m in 0.025 m steps on a 0.3 m grid), for the initial-state and reset tests.
    Every stance on it is within the legs' reach (the tests assert the model's ik_residual).  At the reference's own 0.2 m about one placement
    in twenty of the two small robots is not -- the body stands at its highest foot's level and a foot 0.2 m lower is beyond a 0.4 m leg -- and
    there the 20 Newton iterations of the initial inverse kinematics do not converge, in the model as in the header."""
    from rl_mpc_locomotion_amd.terrain import Terrain
    return Terrain.random_uniform(64, 48, -0.1, 0.0, 0.025, seed=6448, x0=-1.7, y0=-1.7)


def surface_test_points(t):
    """[4133, 2] points of t's own frame: every node, points exactly on the cells' diagonals, on cell edges, outside the field on all four sides
    and beyond its corners, +-inf / NaN / +-1e300 in either coordinate, and points inside cells."""
    rng = np.random.default_rng(4133)
    (xa, xb), (ya, yb) = t.extent
    xs, ys = t.x0 + np.arange(t.rows) * t.hscale, t.y0 + np.arange(t.cols) * t.hscale
    nodes = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    d = (t.x0 + (np.arange(min(t.rows, t.cols) - 1)[:, None] + np.linspace(0.0, 0.96, 8)[None, :]) * t.hscale).reshape(-1)
    diag = np.stack([d, d], 1)                                                   # x == y and x0 == y0: fu == fv bit for bit
    ex = np.stack([xs[rng.integers(0, t.rows, 300)], rng.uniform(ya, yb, 300)], 1)          # fu == 0
    ey = np.stack([rng.uniform(xa, xb, 300), ys[rng.integers(0, t.cols, 300)]], 1)          # fv == 0
    out = []
    for k in range(10):
        out += [(xa - rng.uniform(0.01, 5), rng.uniform(ya, yb)), (xb + rng.uniform(0.01, 5), rng.uniform(ya, yb)),
                (rng.uniform(xa, xb), ya - rng.uniform(0.01, 5)), (rng.uniform(xa, xb), yb + rng.uniform(0.01, 5))]
    out += [(xa - 1, ya - 2), (xa - 1, yb + 2), (xb + 1, ya - 2), (xb + 1, yb + 2)]
    sp = [np.inf, -np.inf, np.nan, 1e300, -1e300, 0.33]
    special = [(a, b) for a in sp for b in sp if not (a == 0.33 and b == 0.33)]
    pts = np.concatenate([nodes, diag, ex, ey, np.array(out), np.array(special)])
    inside = np.stack([rng.uniform(xa, xb, 4133 - len(pts)), rng.uniform(ya, yb, 4133 - len(pts))], 1)
    return np.ascontiguousarray(np.concatenate([pts, inside]))
