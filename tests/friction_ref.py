"""A numpy restatement of the per-robot friction draw (csrc/friction.h), written from the formula of the header's head, not from its code (TEST ONLY),
on tests/domain_rand_ref.py's mix64 / uniform01::

    u  = uniform01(seed ^ DOM_FRICTION, env, e, 0)
    mu = fminf(lo + (hi - lo) * u, hi)                                          buckets == 0
    mu = fminf(lo + ((hi - lo) * floorf(u * buckets)) / (buckets - 1), hi)      buckets >= 2

each operation in float32; the plant steps with ``float64(mu)``.
"""
import numpy as np

from tests.domain_rand_ref import uniform01

F = np.float32
DOM_FRICTION = 0x4452465249435458      # "DRFRICTX", csrc/domain_rand.h's kDomFriction


def draw_mu(seed, env, e, lo, hi, buckets=0):
    """mu [len(env)] float32 of draw e; env, e broadcast ([k] arrays or scalars)."""
    env, e = np.broadcast_arrays(np.atleast_1d(np.asarray(env, dtype=np.uint64)), np.asarray(e, dtype=np.uint64))
    lo, hi = F(lo), F(hi)
    u = uniform01(int(seed) ^ DOM_FRICTION, env, e, np.uint64(0))
    assert u.dtype == F
    if buckets > 0:
        b = np.floor(u * F(buckets))
        return np.minimum(lo + ((hi - lo) * b) / F(buckets - 1), hi).astype(F)
    return np.minimum(lo + (hi - lo) * u, hi).astype(F)
