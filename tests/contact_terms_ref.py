"""The contact terms restated in numpy (csrc/contact_terms.h is compared with this, on the host and on the device): the three terms, the reward, the
sums, the close with its blocked float64 reduction, the window, the critic's sixteen columns -- and the hand-made batches both sets of tests run.

Every per-environment operation is one numpy float32 operation, so one rounding, in the header's order; sums run left to right from +0.  The close is
the rule of tests/episode_terms_ref.py with three terms.  The task's own six terms are an INPUT here (rltask::reward_terms holds an expf, which is not
an IEEE operation): the tests take them from the build under test.  The shaping unit's eight are an input too: the tensor that unit writes.

NaN: where a value is NaN the tests ask for a NaN at the same place, not for the same payload (``same``); everything else is compared bit for bit."""
import numpy as np

F = np.float32
TERMS = ("feet_slip", "feet_contact_forces", "feet_stumble")
FEET_SLIP, FEET_CONTACT_FORCES, FEET_STUMBLE = range(3)
NT = 3
BLOCK = 64
WINDOW_LEN = 1 + NT
COLUMNS = 16
SHAPING_TERMINATION = 7
NEAR = np.nextafter


def same(got, want):
    """Bit for bit, but for NaN: a NaN wherever the other has one."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return got.tobytes() == want.tobytes()
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes())


def scales_of(per_second, dt):
    """The float32 scales: a Python float product rounded once, as ContactSpec.scales() and the C ABI's (float) cast do it."""
    return np.array([float(v) * float(dt) for v in per_second], dtype=np.float64).astype(F)


def terms_of(scale, max_contact_force, dt, force, slip, ids):
    """cterms::tick_terms: e [n, 3] float32 of force [n, 4, 3], slip [n, 4] and ids [n] (>= 0: the tick performs the environment's reset)."""
    force, slip = np.asarray(force, F).reshape(-1, 4, 3), np.asarray(slip, F).reshape(-1, 4)
    n = len(force)
    k, fmax, dt = np.asarray(scale, F), F(max_contact_force), F(dt)
    marked = np.asarray(ids) >= 0
    e = np.zeros((n, NT), F)
    with np.errstate(all="ignore"):
        if k[FEET_SLIP] != 0:
            s = np.zeros(n, F)
            for l in range(4):
                v = slip[:, l] / dt
                s = s + v * v
            e[:, FEET_SLIP] = np.where(marked, F(0), s * k[FEET_SLIP])
        if k[FEET_CONTACT_FORCES] != 0:
            s = np.zeros(n, F)
            for l in range(4):
                fx, fy, fz = force[:, l, 0], force[:, l, 1], force[:, l, 2]
                m = np.sqrt((fx * fx + fy * fy) + fz * fz)
                s = s + np.fmax(m - fmax, F(0))
            e[:, FEET_CONTACT_FORCES] = np.where(marked, F(0), s * k[FEET_CONTACT_FORCES])
        if k[FEET_STUMBLE] != 0:
            hit = np.zeros(n, bool)
            for l in range(4):
                fx, fy, fz = force[:, l, 0], force[:, l, 1], force[:, l, 2]
                hit = hit | (np.sqrt(fx * fx + fy * fy) > F(5) * np.abs(fz))
            e[:, FEET_STUMBLE] = np.where(marked, F(0), hit.astype(F) * k[FEET_STUMBLE])
    return e.astype(F)


def reward(scale, task_terms, e, shaping_scale=None, shaping_terms=None):
    """fmaxf(((s + k0) + k1) + k2, 0) over the live contact terms (+ the shaping termination term where live); s is the unclipped chain of the step
    without the unit: the task's six terms left to right, then the live shaping terms below termination.  fmaxf(NaN, 0) is 0."""
    t, k = np.asarray(task_terms, F), np.asarray(scale, F)
    with np.errstate(all="ignore"):
        s = ((((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]) + t[:, 4]) + t[:, 5]
        if shaping_scale is not None:
            g, se = np.asarray(shaping_scale, F), np.asarray(shaping_terms, F)
            for i in range(SHAPING_TERMINATION):
                if g[i] != 0:
                    s = s + se[:, i]
        for i in range(NT):
            if k[i] != 0:
                s = s + e[:, i]
        rew = np.fmax(s, F(0))
        if shaping_scale is not None and g[SHAPING_TERMINATION] != 0:
            rew = rew + se[:, SHAPING_TERMINATION]
    return rew.astype(F)


class Contact:
    """The unit's whole state and its two calls."""

    def __init__(self, n, scales, max_contact_force, dt):
        self.n = n
        self.scale = np.asarray(scales, F)
        self.max_contact_force, self.dt = F(max_contact_force), F(dt)
        self.sums, self.ticks = np.zeros((n, NT), F), np.zeros(n, np.int32)
        self.window = np.zeros(WINDOW_LEN, np.float64)

    def state(self):
        return dict(sums=self.sums, ticks=self.ticks, window=self.window)

    def close(self, ids):
        """mpc_contact_close: S [4] float64, the closed count and the three sums over the closed environments in the fixed order."""
        marked = np.asarray(ids) >= 0
        with np.errstate(all="ignore"):
            closed = marked & (self.ticks > 0) & np.isfinite(self.sums).all(1)
        S = [0.0] * WINDOW_LEN
        for first in range(0, self.n, BLOCK):
            part = [0.0] * WINDOW_LEN
            for e in range(first, min(first + BLOCK, self.n)):
                if closed[e]:
                    part[0] = part[0] + 1.0
                    for i in range(NT):
                        part[1 + i] = part[1 + i] + float(self.sums[e, i])
            for j in range(WINDOW_LEN):
                S[j] = S[j] + part[j]
        S = np.array(S, np.float64)
        self.window = self.window + S
        self.sums[marked] = 0
        self.ticks[marked] = 0
        return S

    def run(self, force, slip, ids, task_terms, shaping_scale=None, shaping_terms=None):
        """mpc_contact_run: (e [n, 3], rew [n]) float32."""
        e = terms_of(self.scale, self.max_contact_force, self.dt, force, slip, ids)
        rew = reward(self.scale, task_terms, e, shaping_scale, shaping_terms)
        with np.errstate(all="ignore"):
            self.sums = (self.sums + e).astype(F)
        self.ticks = self.ticks + np.int32(1)
        return e, rew


def summary(window, episode_length_s):
    return np.concatenate([window, [episode_length_s]])


def extend(priv, mu, force, force_scale, mu_clip, clip_obs):
    """mpc_contact_extend: priv [n, Wp] float32, mu [n] float64 (>= 0, inf allowed), force [n, 4, 3] float32 -> [n, Wp + 16] float32."""
    priv, force = np.asarray(priv, F), np.asarray(force, F).reshape(len(priv), 12)
    c = F(clip_obs)
    with np.errstate(all="ignore"):
        col_mu = np.fmin(np.asarray(mu, np.float64).astype(F), F(mu_clip))
        cols = np.fmin(np.fmax(force * F(force_scale), -c), c)
    return np.concatenate([priv, col_mu[:, None], cols, np.zeros((len(priv), 3), F)], 1).astype(F)


# ---- the batches ---------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 130)
ALL_ON = (-0.4, -0.02, -1.5)           # per-second scales: every term live
SUBSETS = tuple(tuple(v if (mask >> i) & 1 else 0.0 for i, v in enumerate(ALL_ON)) for mask in range(8))
DT = 0.01
MAX_FORCE = 100.0
FMAX = F(MAX_FORCE)


def _leg_of_norm(m):
    """A force [3] whose float32 norm sqrtf((x x + y y) + z z) is exactly m for x = y = 0: (0, 0, m)."""
    return np.array([0.0, 0.0, m], F)


def crafted_rows():
    """(force [R, 4, 3], slip [R, 4]) float32, one row per case:
       0  all zero;  1  one leg exactly at max_contact_force;  2  the same one ulp above it;  3  a leg with sqrt(Fx^2 + Fy^2) exactly 5 |Fz|;
       4  the same one ulp above;  5  every leg loaded above the limit and sliding;  6  a foot that slid and carries no force (it lifted);
       7  a stumble by a leg with Fz = 0 and a tangential force;  8  negative Fz of the same size as case 3 (fabsf)."""
    R = 9
    force, slip = np.zeros((R, 4, 3), F), np.zeros((R, 4), F)
    force[1, 2] = _leg_of_norm(FMAX)
    force[2, 2] = _leg_of_norm(NEAR(FMAX, F(np.inf)))
    force[3, 1] = (F(15), F(0), F(3))                                          # sqrt(225) = 15 = 5 * 3 exactly
    force[4, 1] = (NEAR(F(15), F(np.inf)), F(0), F(3))
    force[5] = [(30, -20, 140), (-25, 10, 150), (5, 5, 101), (0, 0, 260)]
    slip[5] = (0.004, 0.0005, 0.0, 0.012)
    slip[6, 3] = 0.007
    force[7, 0] = (F(0.5), F(0), F(0))
    force[8, 1] = (F(15), F(0), F(-3))
    return force, slip


def random_tick(n, rng):
    """One tick's rows for n environments: the crafted rows where n allows (row r takes case r % 12, cases 9 .. 11 random), reactions of a trot."""
    force = (rng.standard_normal((n, 4, 3)) * [25, 25, 60] + [0, 0, 70]).astype(F)
    force[rng.random((n, 4)) < 0.45] = 0                                       # feet in the air
    slip = (np.abs(rng.standard_normal((n, 4))) * 0.004 * (rng.random((n, 4)) < 0.4)).astype(F)
    cf, cs = crafted_rows()
    case = np.arange(n) % 12
    for c in range(len(cf)):
        force[case == c], slip[case == c] = cf[c], cs[c]
    task6 = (rng.standard_normal((n, 6)) * [0.004, 0.01, 0.0004, 0.002, 0.001, 0.0] + [0.008, -0.002, 0, 0.004, -0.0005, 0]).astype(F)
    return dict(force=force, slip=slip, task6=task6)


def shaping_tick(n, rng):
    """Eight shaping terms of a tick as the shaping unit writes them for SHAPING_ON: penalties below the clip, termination now and then."""
    se = (-np.abs(rng.standard_normal((n, 8))) * [2e-3, 1e-3, 5e-4, 1e-4, 2e-3, 1e-3, 1e-3, 0]).astype(F)
    se[:, 5] = np.abs(se[:, 5]) * (rng.random(n) < 0.3)
    se[:, SHAPING_TERMINATION] = np.where(rng.random(n) < 0.15, scales_of(SHAPING_ON, DT)[SHAPING_TERMINATION], F(0))
    se[:, np.asarray(SHAPING_ON) == 0] = 0
    return se


SHAPING_ON = (-0.7, -3.0, 0.0, -2.5e-7, -0.01, 1.5, -0.3, -200.0)              # per-second shaping scales: dof_vel off, termination live
SHAPING_NO_TERMINATION = SHAPING_ON[:7] + (0.0,)


def marks(n, pattern, k=0):
    r = np.arange(n)
    marked = {"none": np.zeros(n, bool), "some": ((r + k) * 2654435761 % 7) < 3, "all": np.ones(n, bool)}[pattern]
    return np.where(marked, r, -1).astype(np.int32)


# six ticks: everybody is reset at tick 0 (what the task's first tick does), some on two consecutive ticks, nobody on the others
PATTERN = ("all", "none", "some", "some", "none", "none")


def chain(n, seed):
    """[(ids, batch)] over the six ticks of PATTERN."""
    rng = np.random.default_rng(seed)
    return [(marks(n, p, k), random_tick(n, rng)) for k, p in enumerate(PATTERN)]
