"""A numpy restatement of csrc/domain_rand.h, written from the formulas of its head and of the issue, not from its code: the counter-based draws
(rl_task.h's splitmix64 finaliser and uniform01, ppo_rollout.h's Box-Muller pair, restated here on uint64 arrays), the noise formula one float32
operation at a time, the push value, and what the CPU and the GPU tests share: the crafted batch, the seeds, and the checks a build's output owes this
restatement (check_against_restatement, check_moments)."""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PPO_NOISE_DOMAIN = 0x50504F5F4E4F4953          # ppo_rollout.h's own constant: normal_pair XORs it into whatever seed it is given
DOM_OBS_NOISE, DOM_OBS_CORR = 0x44524F42534E4F49, 0x44524F4253434F52
DOM_ACT_NOISE, DOM_ACT_CORR = 0x44524143544E4F49, 0x4452414354434F52
DOM_PUSH = 0x445250555348585A
DOMAINS = {"observations": (DOM_OBS_NOISE, DOM_OBS_CORR), "actions": (DOM_ACT_NOISE, DOM_ACT_CORR)}
F = np.float32
INV24 = F(1.0 / 16777216.0)

# The worst |float32 Box-Muller draw - its float64 evaluation from the same u1, u2| the host build (g++, glibc's logf / cosf / sinf) shows on the
# crafted batch and on the moment batch (tests/test_domain_rand.py measures it and asserts it stays below this).  Where it comes from: theta =
# float32(2 pi) * u2 is rounded to float32 (half an ulp of a number below 2 pi: 2.4e-7) and multiplied by r <= 5.77.  The GPU test allows the
# device's own logf / cosf / sinf 4 x this.
HOST_NORMAL_GAP = 1.61e-6

SEED = 20261019
MOMENT_SEEDS = {"gaussian": 7, "uniform": 7}          # the seeds of the moment tests, here and on the GPU (chosen on the host build)
MOMENT_SHAPE = (4096, 48, 4)                           # environments, columns, ticks
N = 67
SHAPES = ((12, 12), (48, 48), (240, 235), (2, 1))       # (W, active)
CLIP = 5.0


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix64(x):
    with np.errstate(over="ignore"):
        x = u64(x).copy()
        x ^= x >> u64(30); x *= u64(0xBF58476D1CE4E5B9)
        x ^= x >> u64(27); x *= u64(0x94D049BB133111EB)
        x ^= x >> u64(31)
    return x


def _word(seed, env, step, item):
    """mix64(k ^ mix64((env << 32 | step) + GOLDEN * (item + 1))), k = mix64(seed + GOLDEN); env, step, item broadcast."""
    with np.errstate(over="ignore"):
        k = mix64(u64((int(seed) + GOLDEN) & M64))
        key = (u64(env) << u64(32) | u64(step)) + u64(GOLDEN) * (u64(item) + u64(1))
        return mix64(k ^ mix64(key))


def uniform01(seed, env, step, col):
    """rl_task.h's uniform01: 24 bits as a float32 in [0, 1)."""
    return (_word(seed, env, step, col) >> u64(40)).astype(F) * INV24


def normal_u(seed, env, step, pair):
    """The two uniforms of ppo_rollout.h's normal_pair: u1 in (0, 1], u2 in [0, 1), float32."""
    x = _word((int(seed) ^ PPO_NOISE_DOMAIN) & M64, env, step, pair)
    u1 = ((x >> u64(40)) + u64(1)).astype(F) * INV24
    u2 = ((x >> u64(16)) & u64(0xFFFFFF)).astype(F) * INV24
    return u1, u2


def normal_pair64(seed, env, step, pair):
    """Box-Muller in float64 from the float32 u1, u2."""
    u1, u2 = normal_u(seed, env, step, pair)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    th = 2.0 * np.pi * u2.astype(np.float64)
    return r * np.cos(th), r * np.sin(th)


def grid(n, active):
    env = np.arange(n, dtype=np.uint64)[:, None]
    col = np.arange(active, dtype=np.uint64)[None, :]
    return env, col


def uniform_draws(target, seed, n, active, tick):
    """d [n, active] float32 of a uniform spec."""
    env, col = grid(n, active)
    return uniform01(int(seed) ^ DOMAINS[target][0], env, tick, col)


def normal_draws64(target, seed, n, active, tick, corr=False):
    """d (or zc with corr=True: tick 0 of the corr domain) [n, active] in float64."""
    env, col = grid(n, active)
    z0, z1 = normal_pair64(int(seed) ^ DOMAINS[target][1 if corr else 0], env, 0 if corr else tick, col >> u64(1))
    return np.where((col & u64(1)) == 0, z0, z1)


def apply(x, d, zc, m, s, m_corr, s_corr, clip, scaling, col_scale=None):
    """The element formula, each line one float32 operation.  x, d, zc [n, active] float32."""
    x, d, zc = np.asarray(x, F), np.asarray(d, F), np.asarray(zc, F)
    m, s, m_corr, s_corr, clip = F(m), F(s), F(m_corr), F(s_corr), F(clip)
    with np.errstate(all="ignore"):
        corr = zc * s_corr
        corr = corr + m_corr
        term = d * s
        term = corr + term
        term = term + m
        term = term * (np.ones(x.shape[1], F) if col_scale is None else np.asarray(col_scale, F)[None, :x.shape[1]])
        y = x * term if scaling else x + term
        out = np.where(y < -clip, -clip, np.where(y > clip, clip, y))          # torch.clamp: a NaN stays
    return out.astype(F)


def push_value(seed, env, push_index, axis, v):
    v = F(v)
    u = uniform01(int(seed) ^ DOM_PUSH, env, push_index, axis)
    return np.minimum(-v + (v - (-v)) * u, v).astype(F)


SPECIALS = (0.0, -0.0, CLIP, -CLIP, 5.5, -7.25, np.nan, np.inf, -np.inf, 1e-30, 4.9999995, -4.9999995, 3.0e38)


def crafted(n, W, seed=11):
    """Rows [n][W]: random values of a few magnitudes with the special values (signed zeros, the clip, values beyond it, NaN, the infinities)
    spread over every column position, the last pair and the pad included."""
    rng = np.random.default_rng(seed + W)
    x = (rng.standard_normal((n, W)) * rng.choice([0.01, 1.0, 4.0, 30.0], (n, W))).astype(F)
    k = 0
    for r in range(n):
        for c in range((r * 5) % 3, W, 3):
            if (r + c) % 2 == 0:
                x[r, c] = SPECIALS[k % len(SPECIALS)]
                k += 1
    return x


def column_scale(W, seed=5):
    cs = np.random.default_rng(seed).uniform(0.0, 2.0, W).astype(F)
    cs[::7] = 0.0
    return cs


# (distribution, operation, range, range_correlated): the four pairs, with and without the correlated term
CASES = [(dist, op, rng, corr)
         for dist, rng, corrs in (("gaussian", (0.05, 0.3), ((0.0, 0.0), (-0.02, 0.1))), ("uniform", (-0.4, 0.7), ((0.0, 0.0), (0.1, 0.35))))
         for op in ("additive", "scaling") for corr in corrs]


def kernel_params(dist, rng, corr):
    if dist == "gaussian":
        return rng[0], rng[1], corr[0], corr[1]
    return rng[0], rng[1] - rng[0], corr[0], corr[1] - corr[0]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_restatement(x, out, d, zc, used, target, seed, dist, op, rng, corr, active, tick, col_scale, gap_bound):
    """What both the host build and the kernel owe the restatement; returns the worst normal gap seen."""
    n, W = x.shape
    kp = kernel_params(dist, rng, corr)
    assert used == int(corr != (0.0, 0.0))
    gap = 0.0
    if dist == "uniform":
        assert same(d, uniform_draws(target, seed, n, active, tick))                  # ==
        assert d.min() >= 0.0 and d.max() < 1.0
    else:
        gap = max(gap, float(np.abs(d.astype(np.float64) - normal_draws64(target, seed, n, active, tick)).max()))
    if used:
        gap = max(gap, float(np.abs(zc.astype(np.float64) - normal_draws64(target, seed, n, active, tick, corr=True)).max()))
    else:
        assert (zc == 0).all() and not np.signbit(zc).any()
    assert gap <= gap_bound, (gap, gap_bound)
    want = apply(x[:, :active], d, zc, *kp, CLIP, op == "scaling", col_scale)
    assert same(out[:, :active], want)                                                      # == from the build's own draws
    assert same(out[:, active:], x[:, active:])                                             # the pad is copied
    nan_in = np.isnan(x[:, :active])
    assert nan_in.any() or W == 2
    assert np.isnan(out[:, :active][nan_in]).all()                                           # a NaN stays a NaN
    fin = ~np.isnan(out[:, :active])
    assert (np.abs(out[:, :active][fin]) <= F(CLIP)).all()
    return gap


def moments(d, dist):
    """d [ticks, n, W] -> what the issue bounds: mean, variance, lag-1 correlation across ticks and across adjacent columns"""
    v = d.astype(np.float64)
    mu, var = (0.0, 1.0) if dist == "gaussian" else (0.5, 1.0 / 12.0)
    z = (v - mu) / math.sqrt(var)
    return v.mean(), v.var(), float((z[:-1] * z[1:]).mean()), float((z[:, :, :-1] * z[:, :, 1:]).mean())


def check_moments(d, dist):
    n = d.size
    mean, var, lag_tick, lag_col = moments(d, dist)
    print(f"{dist}: n {n} mean {mean:+.3e} var {var:.6f} lag-1 ticks {lag_tick:+.3e} columns {lag_col:+.3e} (5/sqrt(n) = {5 / math.sqrt(n):.3e})")
    if dist == "gaussian":
        assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
    else:
        assert abs(mean - 0.5) <= 5 / math.sqrt(12 * n) and abs(var - 1 / 12) <= 5 / math.sqrt(180 * n)
    assert abs(lag_tick) <= 5 / math.sqrt(n) and abs(lag_col) <= 5 / math.sqrt(n)
