"""The per-term episode sums and the command curriculum restated in numpy (csrc/episode_terms.h is compared with this, on the host and on the
device): the close, the blocked float64 reduction, the decision, the range update, the window accumulators, the resample, and the crafted batch
both sets of tests run.

The rule that makes EQUAL possible is the header's: environments in blocks of 64 consecutive indices, the closed environments' float32 sums added
in environment order in float64, the block sums added in block order in float64.  Python floats are float64 and one addition is one rounding, so
the loops below are that rule written out.  The resample is float32 with one rounding per operation, as the header's under -ffp-contract=off."""
import numpy as np

from tests.curriculum_ref import uniform01

BLOCK = 64
TERMS = 6
COMMAND_AXIS = 4                       # epterms::kCommandAxis: 0-2 are sample_commands', 3 the terrain curriculum's redraw
G_RANGES, G_WINDOW, G_WIDENINGS, STATE_LEN = 0, 6, 13, 14
LIN_VEL_XY = 0
SENTINEL_SUM, SENTINEL_TICKS, SENTINEL_COUNT, SENTINEL_COMMAND = np.float32(-123.625), 7777, -55, np.float32(9.5)


def reduce_closed(ids, sums, ticks):
    """S [7] float64: the closed count and the six term sums over the closed environments, in the fixed order."""
    n = len(ids)
    closed = (ids >= 0) & (ticks > 0) & np.isfinite(sums).all(1)           # an episode with a NaN or an infinite sum closes nothing
    S = [0.0] * (1 + TERMS)
    for first in range(0, n, BLOCK):
        part = [0.0] * (1 + TERMS)
        for e in range(first, min(first + BLOCK, n)):
            if closed[e]:
                part[0] = part[0] + 1.0
                for i in range(TERMS):
                    part[1 + i] = part[1 + i] + float(sums[e, i])
        for j in range(1 + TERMS):
            S[j] = S[j] + part[j]
    return np.array(S, np.float64)


def decide(S, tick, spec, enabled=True):
    """update_command_curriculum's condition; spec: dict(update_every, max_episode_length, threshold, scale, step, max_curriculum), scale the
    float32 reward scale of lin_vel_xy (already multiplied by dt) as a float."""
    if spec is None or not enabled or tick % spec["update_every"] != 0 or not S[0] > 0:
        return False
    return bool((S[1 + LIN_VEL_XY] / S[0]) / float(spec["max_episode_length"]) > spec["threshold"] * float(np.float32(spec["scale"])))


def resample(seed, env, count, ranges):
    f = np.float32
    out = np.zeros(3, f)
    for a in range(3):
        lo, hi = f(ranges[a, 0]), f(ranges[a, 1])
        out[a] = min(f(lo + f(f(hi - lo) * uniform01(seed, env, count, COMMAND_AXIS + a))), hi)
    return out


def close_and_resample(ids, sums, ticks, counts, state, commands, tick, spec, seed, enabled=True):
    """What mpc_episode_terms_close_and_resample leaves: (sums, ticks, counts, state, commands, S) as new arrays.  spec None: no command curriculum
    (the commands are not touched)."""
    sums, ticks, counts, state, commands = sums.copy(), ticks.copy(), counts.copy(), state.copy(), commands.copy()
    S = reduce_closed(ids, sums, ticks)
    if decide(S, tick, spec, enabled):
        state[G_RANGES + 0] = min(max(state[G_RANGES + 0] - spec["step"], -spec["max_curriculum"]), 0.0)
        state[G_RANGES + 1] = min(max(state[G_RANGES + 1] + spec["step"], 0.0), spec["max_curriculum"])
        state[G_WIDENINGS] += 1.0
    state[G_WINDOW:G_WINDOW + 1 + TERMS] = state[G_WINDOW:G_WINDOW + 1 + TERMS] + S
    marked = ids >= 0
    sums[marked] = 0
    ticks[marked] = 0
    counts[marked] += 1
    if spec is not None:
        ranges = state[G_RANGES:G_RANGES + 6].reshape(3, 2)
        for r in np.flatnonzero(marked):
            commands[r] = resample(seed, int(r), int(counts[r]), ranges)
    return sums, ticks, counts, state, commands, S


def summary(state, episode_length_s):
    return np.concatenate([state[G_WINDOW:G_WINDOW + 1 + TERMS], state[G_RANGES:G_RANGES + 2], [state[G_WIDENINGS], episode_length_s]])


def state0(cfg_ranges, x_range0=None):
    s = np.zeros(STATE_LEN)
    s[G_RANGES:G_RANGES + 6] = np.asarray(cfg_ranges, np.float64).reshape(-1)
    if x_range0 is not None:
        s[G_RANGES:G_RANGES + 2] = x_range0
    return s


PATTERNS = ("nobody", "everybody", "everybody_fresh", "one_per_block", "mix")


def crafted(n, pattern, seed=0):
    """ids [n] int32, sums [n, 6] float32, ticks [n] int32, counts [n] int32, commands [n, 3] float32 for one of PATTERNS.  Environments that are not
    marked carry the sentinels; marked ones sums of mixed sign and magnitude (so that the order of a float64 sum of them matters), ticks >= 1 (0 for
    `everybody_fresh`, and for every fifth marked environment of `mix`, which also has NaN, +inf and -inf sums in some) and counts that differ."""
    rng = np.random.default_rng(1000 * n + PATTERNS.index(pattern) + seed)
    r = np.arange(n)
    marked = {"nobody": np.zeros(n, bool), "everybody": np.ones(n, bool), "everybody_fresh": np.ones(n, bool), "one_per_block": r == np.minimum(r // BLOCK * BLOCK + (r // BLOCK * 7 + 3) % BLOCK, n - 1),
              "mix": (r * 2654435761 % 7) < 4}[pattern]
    ids = np.where(marked, r, -1).astype(np.int32)
    mag = np.float32(10.0) ** rng.integers(-6, 4, (n, TERMS)).astype(np.float32)
    sums = (rng.standard_normal((n, TERMS)).astype(np.float32) * mag).astype(np.float32)
    sums[:, LIN_VEL_XY] = np.abs(sums[:, LIN_VEL_XY])
    ticks = rng.integers(1, 2000, n).astype(np.int32)
    if pattern == "everybody_fresh":
        ticks[:] = 0
    if pattern == "mix":
        ticks[np.flatnonzero(marked)[::5]] = 0
        for k, bad in enumerate((np.nan, np.inf, -np.inf)):                    # marked, ticks > 0, and a sum that is not finite: closes nothing
            hit = np.flatnonzero(marked)[1 + k::15]
            sums[hit, (k + hit) % TERMS] = bad
    counts = rng.integers(0, 50, n).astype(np.int32)
    commands = np.full((n, 3), SENTINEL_COMMAND, np.float32)
    sums[~marked], ticks[~marked], counts[~marked] = SENTINEL_SUM, SENTINEL_TICKS, SENTINEL_COUNT
    return dict(ids=ids, sums=sums, ticks=ticks, counts=counts, commands=commands, marked=marked)
