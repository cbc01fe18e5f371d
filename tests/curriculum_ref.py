"""The terrain curriculum restated in numpy float32 (csrc/terrain_curriculum.h is compared with this, on the host and on the device): the decision,
the level rule, the counter-based redraw, and the crafted batch both sets of tests run.

Everything is float32 with one rounding per operation, as the header's: numpy's float32 multiply, add and sqrt are correctly rounded, and so are the
header's under -ffp-contract=off, so decisions, levels, counters and origins must be EQUAL.  (sqrt(fl(x x)) == |x| in binary floating point, which
is what lets a row sit exactly on a threshold.)"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
LEVEL_AXIS = 3                         # curriculum::kLevelAxis: the commands use 0, 1, 2
F32_MAX = np.float32(3.402823466e+38)
SENTINEL_LEVEL, SENTINEL_ORIGIN = -77, (123456.75, -654321.5)


def mix64(x):
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def uniform01(seed, env, episode, axis):
    """rl_task.h's uniform01: 24 bits as a float32 in [0, 1)."""
    k = mix64((seed + GOLDEN) & M64)
    x = mix64(k ^ mix64((((env << 32) | episode) + GOLDEN * (axis + 1)) & M64))
    return np.float32(x >> 40) * np.float32(1.0 / 16777216.0)


def draw_level(seed, env, k, max_level):
    return min(int(np.float32(uniform01(seed, env, k, LEVEL_AXIS) * np.float32(max_level))), max_level - 1)


def decide(xy, commands, half_len, episode_length_s):
    """+1 / -1 / 0 per row; xy [n, 2], commands [n, >=2] float32."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, cx, cy = (np.asarray(a, f) for a in (xy[:, 0], xy[:, 1], commands[:, 0], commands[:, 1]))
        d = np.sqrt(x * x + y * y)
        finite = d <= F32_MAX
        up = finite & (d > f(half_len))
        down = finite & (d < (np.sqrt(cx * cx + cy * cy) * f(episode_length_s)) * f(0.5)) & ~up
    assert d.dtype == np.float32
    return up.astype(np.int32) - down.astype(np.int32)


def update(reset, root, commands, types, tile_origins, levels, counts, origins, env_length, episode_length_s, seed):
    """What mpc_curriculum_update leaves: (levels, counts, origins, moves) as new arrays; rows with reset == 0 untouched (moves 0 there)."""
    num_levels = tile_origins.shape[0]
    levels, counts, origins = levels.copy(), counts.copy(), origins.copy()
    moves = decide(root[:, :2], commands, np.float32(env_length / 2.0), np.float32(episode_length_s))
    moves[reset == 0] = 0
    for r in np.flatnonzero(reset):
        counts[r] += 1
        l = int(levels[r]) + int(moves[r])
        l = draw_level(seed, int(r), int(counts[r]), num_levels) if l >= num_levels else max(l, 0)
        levels[r] = l
        origins[r] = tile_origins[l, types[r]]
    return levels, counts, origins, moves


PATTERN = 16                           # rows of the crafted pattern


def crafted(n, num_levels, num_types, env_length, episode_length_s):
    """n rows, the PATTERN below repeated (with another environment index and type, so another redraw and another origin): reset [n] int64, root [n, 13],
    commands [n, 3] float32, levels [n] int32, types [n] int32, and `expect` [n]: the move each row must make, None where it is a redraw."""
    f = np.float32
    half = f(env_length / 2.0)
    c = f(0.1)
    thr = f(f(c * f(episode_length_s)) * f(0.5))          # commands (c, 0): sqrt(c c) == c
    assert 0 < thr < half and num_levels >= 3
    top = num_levels - 1
    inf, nan = f(np.inf), f(np.nan)
    #        x                       y      cx   cy   level  reset  move
    rows = [(half,                   0,     c,   0,   1,     1,     0),        # d == half_len: the comparison is strict
            (np.nextafter(half, inf), 0,    c,   0,   1,     1,     1),        # one ulp above
            (thr,                    0,     c,   0,   1,     1,     0),        # d == the down threshold: strict again
            (np.nextafter(thr, f(0)), 0,    c,   0,   1,     1,     -1),       # one ulp below
            (f(0.01),                0,     c,   0,   0,     1,     -1),       # level 0 demoted: stays 0
            (0,                      -half * f(1.5), c, 0, top, 1,  1),        # the top level promoted: the redraw
            (nan,                    0,     c,   0,   1,     1,     0),
            (inf,                    0,     c,   0,   1,     1,     0),
            (0,                      -inf,  c,   0,   1,     1,     0),
            (0,                      0,     0,   0,   1,     1,     0),        # the first tick: zero command, zero distance
            (half * f(2),            0,     c,   0,   SENTINEL_LEVEL, 0, 0),   # not being reset: sentinels must survive
            (nan,                    nan,   c,   0,   SENTINEL_LEVEL, 0, 0),
            (half * f(0.8),          half * f(0.8), f(0.5), f(-0.3), 0, 1, 1), # 0 -> 1 on a diagonal
            (f(0.3),                 f(-0.2), f(0.5), f(-0.3), 1, 1, -1),      # 1 -> 0
            (f(-3e19),               f(3e19), c, 0,   1,     1,     0),        # the squares overflow float32: not finite, keeps its level
            (half * f(0.9),          0,     f(2.5), f(1.0), top, 1, 0)]        # inside the tile, and a threshold beyond it: `up` is false, so demoted
    rows[15] = rows[15][:6] + (-1,)
    assert len(rows) == PATTERN
    reset, root, commands = np.zeros(n, np.int64), np.zeros((n, 13), f), np.zeros((n, 3), f)
    levels, types, expect = np.zeros(n, np.int32), (np.arange(n) % num_types).astype(np.int32), []
    rng = np.random.default_rng(11)
    root[:, 2:] = rng.standard_normal((n, 11)).astype(f)                       # (what the kernel must not read)
    commands[:, 2] = rng.standard_normal(n).astype(f)
    for r in range(n):
        x, y, cx, cy, level, rs, move = rows[r % PATTERN]
        root[r, 0], root[r, 1], commands[r, 0], commands[r, 1], levels[r], reset[r] = x, y, cx, cy, level, rs
        expect.append(None if r % PATTERN == 5 else move)
    return dict(reset=reset, root=root, commands=commands, levels=levels, types=types, expect=expect)


def summary(levels, types, num_types):
    """What mpc_curriculum_summary writes: n, the mean level, per type the count, per type the mean level (0.0 without members)."""
    out = np.zeros(2 + 2 * num_types)
    out[0], out[1] = len(levels), np.sum(levels.astype(np.int64)) / len(levels)
    for t in range(num_types):
        m = types == t
        out[2 + t] = m.sum()
        out[2 + num_types + t] = np.sum(levels[m].astype(np.int64)) / m.sum() if m.any() else 0.0
    return out
