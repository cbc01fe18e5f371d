"""The reward shaping terms restated in numpy (csrc/reward_shaping.h is compared with this, on the host and on the device): the eight terms, the
reward, the history and its reset, the sums, the close with its blocked float64 reduction, the window -- and the crafted batches both sets of tests run.

Every per-environment operation is one numpy float32 operation, so one rounding, in the header's order; sums run left to right from +0.  The
base-height mean repeats the header's order: 64 lane-strided partial sums, then the tree with the strides 32, 16, 8, 4, 2, 1.  The close is the rule
of tests/episode_terms_ref.py with eight terms.  The task's own six terms are an INPUT here (rltask::reward_terms holds an expf, which is not an IEEE
operation): the tests take them from the build under test.

NaN: where a value is NaN the tests ask for a NaN at the same place, not for the same payload (``same``); everything else is compared bit for bit."""
import numpy as np

F = np.float32
TERMS = ("orientation", "base_height", "dof_vel", "dof_acc", "action_rate", "feet_air_time", "stand_still", "termination")
ORIENTATION, BASE_HEIGHT, DOF_VEL, DOF_ACC, ACTION_RATE, FEET_AIR_TIME, STAND_STILL, TERMINATION = range(8)
NT = 8
BLOCK = 64
LANES = 64
WINDOW_LEN = 1 + NT


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
    """The eight float32 scales: a Python float product rounded once, as TaskConfig.reward_scales() and the C ABI's (float) cast do it."""
    return np.array([float(v) * float(dt) for v in per_second], dtype=np.float64).astype(F)


def quat_rotate_inverse(q, v):
    """rltask::quat_rotate_inverse, operation for operation; q [n, 4] xyzw, v [3] or [n, 3]."""
    v = np.broadcast_to(np.asarray(v, F), (len(q), 3))
    w = q[:, 3]
    s = F(2.0) * (w * w) - F(1.0)
    cx = q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1]
    cy = q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2]
    cz = q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0]
    d = (q[:, 0] * v[:, 0] + q[:, 1] * v[:, 1]) + q[:, 2] * v[:, 2]
    return np.stack([(v[:, 0] * s - cx * w * F(2.0)) + q[:, 0] * d * F(2.0), (v[:, 1] * s - cy * w * F(2.0)) + q[:, 1] * d * F(2.0),
                     (v[:, 2] * s - cz * w * F(2.0)) + q[:, 2] * d * F(2.0)], 1)


def height_mean(root_z, heights):
    """The mean of root_z - heights[p] in the header's order; heights [n, P] or None (P = 0: root_z)."""
    n = len(root_z)
    P = 0 if heights is None else heights.shape[1]
    if P == 0:
        return root_z.astype(F).copy()
    s = np.zeros((n, LANES), F)
    for l in range(LANES):
        for p in range(l, P, LANES):
            s[:, l] = s[:, l] + (root_z - heights[:, p])
    stride = LANES // 2
    while stride >= 1:
        s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
        stride //= 2
    return s[:, 0] / F(P)


def moving(commands):
    return np.sqrt(commands[:, 0] * commands[:, 0] + commands[:, 1] * commands[:, 1]) > F(0.1)


class Shaping:
    """The unit's whole state and its two calls."""

    def __init__(self, n, scales, base_height_target, air_time_target, dt, default_dof_pos, max_episode_length):
        self.n = n
        self.scale = np.asarray(scales, F)
        self.base_height_target, self.air_time_target, self.dt = F(base_height_target), F(air_time_target), F(dt)
        self.default_dof_pos = np.asarray(default_dof_pos, np.float64).astype(F)
        self.max_episode_length = int(max_episode_length)
        self.last_actions, self.last_dof_vel = np.zeros((n, 12), F), np.zeros((n, 12), F)
        self.air_time, self.last_contact = np.zeros((n, 4), F), np.zeros((n, 4), np.int32)
        self.sums, self.ticks = np.zeros((n, NT), F), np.zeros(n, np.int32)
        self.window = np.zeros(WINDOW_LEN, np.float64)

    def state(self):
        return dict(last_actions=self.last_actions, last_dof_vel=self.last_dof_vel, air_time=self.air_time, last_contact=self.last_contact, sums=self.sums,
                    ticks=self.ticks, window=self.window)

    def close(self, ids):
        """mpc_shaping_close: S [9] float64, the closed count and the eight sums over the closed environments in the fixed order."""
        marked = ids >= 0
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

    def run(self, root, dof, actions, commands, ids, reset, progress, contact, heights, task_terms):
        """mpc_shaping_run: (e [n, 8], rew [n]) float32; root [n, 13], dof [n, 12, 2], actions [n, 12], commands [n, 3], ids [n] int32, reset and
        progress [n] int64, contact [n, 4] (non-zero: in contact), heights [n, P] or None, task_terms [n, 6] the build's own six."""
        root, dof, actions, commands = (np.asarray(x, F) for x in (root, dof.reshape(self.n, 12, 2), actions, commands))
        n, k = self.n, self.scale
        marked = np.asarray(ids) >= 0
        mv = moving(commands)
        q, qd = dof[:, :, 0], dof[:, :, 1]
        e = np.zeros((n, NT), F)
        with np.errstate(all="ignore"):
            if k[ORIENTATION] != 0:
                g = quat_rotate_inverse(root[:, 3:7], (0.0, 0.0, -1.0))
                e[:, ORIENTATION] = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) * k[ORIENTATION]
            if k[BASE_HEIGHT] != 0:
                d = height_mean(root[:, 2], heights) - self.base_height_target
                e[:, BASE_HEIGHT] = (d * d) * k[BASE_HEIGHT]
            if k[DOF_VEL] != 0:
                s = np.zeros(n, F)
                for i in range(12):
                    s = s + qd[:, i] * qd[:, i]
                e[:, DOF_VEL] = s * k[DOF_VEL]
            if k[DOF_ACC] != 0:
                s = np.zeros(n, F)
                for i in range(12):
                    a = (self.last_dof_vel[:, i] - qd[:, i]) / self.dt
                    s = s + a * a
                e[:, DOF_ACC] = np.where(marked, F(0), s * k[DOF_ACC])
            if k[ACTION_RATE] != 0:
                s = np.zeros(n, F)
                for i in range(12):
                    a = self.last_actions[:, i] - actions[:, i]
                    s = s + a * a
                e[:, ACTION_RATE] = np.where(marked, F(0), s * k[ACTION_RATE])
            # feet_air_time: the history moves whatever the scale is
            now = np.asarray(contact) != 0
            s = np.zeros(n, F)
            air_next = np.zeros((n, 4), F)
            for l in range(4):
                filt = now[:, l] | (self.last_contact[:, l] != 0)
                first = (self.air_time[:, l] > 0) & filt
                air = self.air_time[:, l] + self.dt
                s = s + (air - self.air_time_target) * first.astype(F)
                air_next[:, l] = air * (~filt).astype(F)
            self.air_time = np.where(marked[:, None], F(0), air_next).astype(F)
            self.last_contact = now.astype(np.int32)
            if k[FEET_AIR_TIME] != 0:
                e[:, FEET_AIR_TIME] = np.where(marked, F(0), np.where(mv, s, F(0)) * k[FEET_AIR_TIME])
            if k[STAND_STILL] != 0:
                s = np.zeros(n, F)
                for i in range(12):
                    s = s + np.abs(q[:, i] - self.default_dof_pos[i])
                e[:, STAND_STILL] = np.where(mv, F(0), s * k[STAND_STILL])
            if k[TERMINATION] != 0:
                term = (np.asarray(reset) != 0) & ~(np.asarray(progress) > self.max_episode_length)
                e[:, TERMINATION] = term.astype(F) * k[TERMINATION]
            self.last_actions, self.last_dof_vel = actions.copy(), qd.copy()
            rew = reward(k, np.asarray(task_terms, F), e)
            self.sums = self.sums + e
            self.ticks = self.ticks + 1
        return e, rew


def reward(scale, t, e):
    """fmaxf((((((t0 + t1) + t2) + t3) + t4) + t5) + e0 + ... + e6, 0) + e7 over the live terms; fmaxf(NaN, 0) is 0."""
    with np.errstate(all="ignore"):
        s = ((((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]) + t[:, 4]) + t[:, 5]
        for i in range(TERMINATION):
            if scale[i] != 0:
                s = s + e[:, i]
        rew = np.fmax(s, F(0))
        if scale[TERMINATION] != 0:
            rew = rew + e[:, TERMINATION]
    return rew.astype(F)


def summary(window, episode_length_s):
    return np.concatenate([window, [episode_length_s]])


# ---- the batches ---------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 130)
POINTS = (0, 1, 63, 64, 65, 187)
ALL_ON = (-0.7, -3.0, -1e-3, -2.5e-7, -0.01, 1.5, -0.3, -200.0)      # per-second scales: every term live
DT = 0.01
MAX_EPISODE_LENGTH = 30
NEAR = np.nextafter
C01 = F(0.1)


def random_tick(n, P, rng, k=0):
    """One tick's inputs for n environments: states of mixed size and sign, unit quaternions that tilt, contacts that come and go."""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    root = np.concatenate([rng.standard_normal((n, 3)) * [3, 3, 0.1] + [0, 0, 0.35], q, rng.standard_normal((n, 6))], 1).astype(F)
    dof = np.stack([rng.standard_normal((n, 12)) * 0.4 + np.tile([0.0, 0.8, -1.6], 4), rng.standard_normal((n, 12)) * 10.0 ** rng.integers(-2, 2, (n, 12))], 2).astype(F)
    actions = np.clip(rng.standard_normal((n, 12)), -1, 1).astype(F)
    commands = (rng.standard_normal((n, 3)) * [0.6, 0.3, 1.0]).astype(F)
    commands[rng.random(n) < 0.3, :2] *= F(0.05)                            # a good share stands still
    torques = (rng.standard_normal((n, 12)) * 8).astype(F)
    calm = np.arange(n) % 3 == 1                                             # every third environment walks quietly on every tick: its reward stays above the clip
    root[calm, 3:6] *= F(0.02)
    root[calm, 3:7] /= np.linalg.norm(root[calm, 3:7].astype(np.float64), axis=1, keepdims=True).astype(F)
    root[calm, 7:] *= F(0.02)
    dof[calm, :, 0] = (np.tile([0.0, 0.8, -1.6], 4) + 0.01 * rng.standard_normal((int(calm.sum()), 12))).astype(F)
    dof[calm, :, 1] *= F(1e-3)
    torques[calm] *= F(0.1)
    commands[calm] = (rng.standard_normal((int(calm.sum()), 3)) * [0.15, 0.05, 0.1]).astype(F)
    contact =(rng.random((n, 4)) < 0.55).astype(np.int32) * rng.integers(1, 3, (n, 4)).astype(np.int32)      # non-zero flags of more than one value
    fell = rng.random(n) < 0.1
    progress = rng.integers(0, MAX_EPISODE_LENGTH + 3, n).astype(np.int64)
    reset = (fell | (progress > MAX_EPISODE_LENGTH)).astype(np.int64)
    heights = None if P == 0 else (rng.standard_normal((n, P)) * 0.15).astype(F)
    return dict(root=root, dof=dof, actions=actions, commands=commands, torques=torques, contact=contact, fell=fell, progress=progress, reset=reset,
                heights=heights)


def crafted_tick(n, P, rng, k=0):
    """random_tick with the rows that matter written in (row r of the batch takes case r % 12 where n allows):
       0-2  command norms just below, at and just above the float32 nearest 0.1 (c, 0);  3  the same at (0, c);  4  a zero command;
       5    a fall on the time-out tick: reset set and progress > max_episode_length;  6  a fall before it;  7  a time-out without a fall;
       8    all feet down;  9  all feet up;  10, 11  as random."""
    b = random_tick(n, P, rng, k)
    r = np.arange(n)
    case = r % 12
    for c, x in ((0, NEAR(C01, F(0))), (1, C01), (2, NEAR(C01, F(1)))):
        b["commands"][case == c, 0], b["commands"][case == c, 1] = x, 0
    b["commands"][case == 3, 0], b["commands"][case == 3, 1] = 0, NEAR(C01, F(1))
    b["commands"][case == 4, :2] = 0
    for c, fell, prog in ((5, True, MAX_EPISODE_LENGTH + 1), (6, True, 7), (7, False, MAX_EPISODE_LENGTH + 1)):
        b["fell"][case == c], b["progress"][case == c] = fell, prog
    b["reset"] = (b["fell"] | (b["progress"] > MAX_EPISODE_LENGTH)).astype(np.int64)
    b["contact"][case == 8] = 1
    b["contact"][case == 9] = 0
    return b


# a plant state that blew up: the row -> the term it reaches first (row 3: the quaternion, 5: the base height, 7: a joint velocity, 9: a measured height)
BLOWN = {3: ORIENTATION, 5: BASE_HEIGHT, 7: DOF_VEL, 9: BASE_HEIGHT}
BLOWN_OFF = tuple(0.0 if i in (ORIENTATION, BASE_HEIGHT, DOF_VEL, DOF_ACC) else v for i, v in enumerate(ALL_ON))      # the terms those values reach, switched off


def blown_up_ticks(n, P, bad, seed=11):
    """Two random ticks of n >= 10 environments with P >= 12 points; the second carries `bad` (NaN, +inf or -inf) in the rows of BLOWN."""
    rng = np.random.default_rng(seed)
    first, second = random_tick(n, P, rng), random_tick(n, P, rng)
    second["root"][3, 4], second["root"][5, 2], second["dof"][7, 2, 1], second["heights"][9, 11] = bad, bad, bad, bad
    return first, second


def landing_tick(rng):
    """Two environments that are moving, and what to seed: (batch, air_time [2, 4]).  Environment 0's foot 0 has flown 0.6 s and lands (above a target of
    0.5 s), environment 1's foot 1 has flown 0.2 s and lands (below it); feet 2 stay down, feet 3 stay up and keep counting."""
    b = random_tick(2, 0, rng)
    b["commands"][:] = (0.5, 0.0, 0.0)
    b["contact"] = np.array([[1, 0, 1, 0], [0, 1, 1, 0]], np.int32)
    air = np.array([[0.6, 0.3, 0.0, 0.25], [0.3, 0.2, 0.0, 0.25]], F)
    return b, air


def marks(n, pattern):
    r = np.arange(n)
    marked = {"none": np.zeros(n, bool), "some": (r * 2654435761 % 7) < 3, "all": np.ones(n, bool)}[pattern]
    return np.where(marked, r, -1).astype(np.int32)


def landing_sequence(target=0.5, dt=DT):
    """Contacts [ticks][4] of one environment whose feet 0 and 1 fly for more and for fewer ticks than `target` and land; foot 2 stays down, 3 up."""
    long_, short = int(round(target / dt)) + 6, max(int(round(target / dt)) - 6, 2)
    ticks = long_ + 6
    c = np.zeros((ticks, 4), np.int32)
    c[:, 2] = 1
    c[:2, :2] = 1
    c[2 + long_:, 0] = 1
    c[2 + short:, 1] = 1
    return c
