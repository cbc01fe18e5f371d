"""Opt-in Coulomb friction of the toy plant on the device (csrc/mpc_friction.h, csrc/mpc_friction.hip, csrc/friction.h, csrc/toy_sim.h's Coulomb
contact): every robot of a ``BatchedToySim`` gets a friction coefficient of its own, and the step publishes each foot's ground reaction and slip.

Without it a stance foot holds its anchor whatever the leg asks of it.  With it, where a leg asks for more tangential force than ``mu`` times its
normal force, the body gets only what the cone allows and the massless foot slides: its anchor moves against the excess by
``h (|ft| - mu fn) / 200 N s/m`` per substep and is put back on the ground.  ``mu = inf`` is the plant without the option, bit for bit; ``mu = 0``
leaves the normal force alone.  legged_gym's ``randomize_friction`` (``friction_range``, 64 buckets), by its published algorithm, draws ``mu`` on the
device with a counter-based generator keyed by (seed, environment, draw index): no generator state, and a draw does not depend on the batch size::

    fr = Friction(n, FrictionSpec(range=(0.5, 1.25), buckets=64, resample="reset"), seed=3)
    task = BatchedRLTask(robot_type, gait_id, cfg, friction=fr)
    PPOTrainer(task).learn(k)
    fr.contact_forces                    # [n, 4, 3] float32, world frame, newtons: Isaac Gym's net_contact_forces of the four feet
    fr.foot_slip                         # [n, 4] float32, metres slid in the last tick

The MPC controller keeps planning with the robot table's mu = 0.4 while the plant disagrees.  Works together with ``plant_rand.PlantRand`` in either
bind order.  ``Friction(n, mu=0.4)`` without a spec is a fixed coefficient (a scalar or [n]) and never draws.

``contact_terms.ContactTerms`` reads the two outputs and the coefficients: ``feet_slip`` / ``feet_contact_forces`` / ``feet_stumble`` reward terms and a
friction column with the ground reactions in the critic's privileged row.  Not built: per-level terrain friction, passing the plant's mu to the
controller.

``FrictionSpec`` and ``Friction.validate`` are host arithmetic and need no GPU; the kernels do (MpcLibraryError without one, no CPU fallback).
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib, toy_sim
from ._lib import cd, ci, pvp, text, vp

RESAMPLE = ("once", "reset")
MAX_BUCKETS = 1 << 24

# the entry points of csrc/mpc_friction.h (bound here, not in any other module's list)
DECLS = {
    "mpc_friction_attach": (ci, [vp, vp, vp, vp]),
    "mpc_friction_create": (ci, [pvp, ci, C.c_ulonglong]),
    "mpc_friction_destroy": (None, [vp]),
    "mpc_friction_bind": (ci, [vp, vp]),
    "mpc_friction_draw": (ci, [vp, vp, ci, cd, cd, ci, ci, vp]),
    "mpc_friction_get_mu": (ci, [vp, vp]),
    "mpc_friction_set_mu": (ci, [vp, vp]),
    "mpc_friction_get_counters": (ci, [vp, vp]),
    "mpc_friction_set_counters": (ci, [vp, vp]),
    "mpc_friction_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what attach takes) with these entry points bound
check = _lib.checker(lib, "mpc_friction_last_error")


@dataclass
class FrictionSpec:
    """``range``: ``(lo, hi)`` of the uniform draw, ``0 <= lo <= hi``.  ``buckets``: 0 for a continuous draw, or the number (>= 2) of equally spaced
    values from lo to hi the draw is quantised to.  ``resample``: ``"once"`` draws every coefficient once, when the task is built (legged_gym's),
    ``"reset"`` draws an environment's anew at each of its resets."""
    range: tuple = (0.5, 1.25)
    buckets: int = 64
    resample: str = "once"

    def validate(self):
        """Everything that can be refused without the device."""
        if self.resample not in RESAMPLE:
            raise ValueError(f"friction: resample {self.resample!r}: 'once' or 'reset'")
        rng = self.range
        with np.errstate(over="ignore"):           # (a bound beyond float32's range becomes inf, and is refused as such)
            finite = len(rng) == 2 and all(math.isfinite(float(v)) and math.isfinite(float(np.float32(v))) for v in rng)
        if not finite:
            raise ValueError("friction: range must be (lo, hi), two numbers that are finite as float32")
        if float(rng[0]) < 0:
            raise ValueError("friction: range needs lo >= 0")
        if float(rng[0]) > float(rng[1]):
            raise ValueError("friction: range with lo > hi")
        if int(self.buckets) != self.buckets or self.buckets < 0 or self.buckets == 1 or self.buckets > MAX_BUCKETS:
            raise ValueError(f"friction: buckets {self.buckets!r}: 0 (a continuous draw) or 2 .. 2^24")


def _mu_array(mu, n):
    """[n] float64 of a scalar or an [n] array, every entry >= 0 and not NaN (inf allowed)."""
    m = np.asarray(mu, dtype=np.float64)
    if m.ndim == 0:
        m = np.full(n, float(m))
    if m.shape != (n,):
        raise ValueError(f"mu: a number or [{n}] expected")
    if not (m >= 0).all():
        raise ValueError("mu: an entry is negative or NaN")
    return np.ascontiguousarray(m)


class Friction(_lib.DrawnRecord):
    """The friction coefficients of ``n`` environments and the step's two outputs.  ``bind(sim)`` attaches the record to a ``BatchedToySim`` (whose
    ``step`` consumes it from then on and fills ``contact_forces`` and ``foot_slip``), ``draw(ids)`` is the one launch per reset;
    ``BatchedRLTask(friction=...)`` does both.  ``spec``: a ``FrictionSpec`` to draw from, or None for coefficients that are only ever set; ``mu``:
    the coefficients before the first draw, a number or [n] (None: inf, the anchor holds).  ``get_mu`` / ``set_mu`` move the coefficients [n]
    between host and device, ``state_dict`` / ``load_state_dict`` the coefficients and the draw counters."""
    WHAT, COUNTERS = "friction", (lib, check, "mpc_friction_get_counters", "mpc_friction_set_counters")
    __del__ = _lib.finalizer("mpc_friction_destroy")

    def __init__(self, n, spec=None, mu=None, seed=0, device=None):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("n must be at least 1")
        self.spec = spec
        self.seed = int(seed) & (2 ** 64 - 1)
        if spec is not None:
            spec.validate()
        self._mu0 = None if mu is None else _mu_array(mu, self.n)
        self.device = device
        self.launches = 0
        self._handle, self.sim = None, None
        self.contact_forces, self.foot_slip = None, None

    def validate(self, n=None):
        """Everything that can be refused without the device; the task calls it with its batch size."""
        if n is not None and int(n) != self.n:
            raise ValueError(f"the friction holds {self.n} environments, the task {int(n)}")
        if self.spec is not None:
            self.spec.validate()

    def bind(self, sim):
        """Give ``sim`` (a ``BatchedToySim`` with ``n`` robots) its friction record and its two output tensors, and this object its draw counters,
        zero.  Once per sim and per object."""
        import torch
        if self.sim is not None:
            raise ValueError("the friction is bound to a sim already")
        if int(sim.n) != self.n:
            raise ValueError(f"the friction holds {self.n} environments, the sim {int(sim.n)}")
        _lib.need_gpu("Friction")
        self.device = _lib.device_of(sim.device if self.device is None else self.device)
        forces = torch.zeros((self.n, 4, 3), dtype=torch.float32, device=self.device)
        slip = torch.zeros((self.n, 4), dtype=torch.float32, device=self.device)
        h = C.c_void_p()
        check(lib().mpc_friction_create(C.byref(h), self.n, self.seed), "mpc_friction_create")
        self._handle = h
        torch.cuda.synchronize(self.device)            # (the zero fills, before a kernel on another stream writes the rows)
        check(lib().mpc_friction_attach(sim._handle, None if self._mu0 is None else self._mu0.ctypes.data, forces.data_ptr(), slip.data_ptr()), "mpc_friction_attach")
        check(lib().mpc_friction_bind(h, sim._handle), "mpc_friction_bind")
        self.contact_forces, self.foot_slip = forces, slip
        self.sim = sim
        sim._friction = self                           # the sim's step writes into this object's tensors: they live as long as the sim

    def draw(self, ids=None, resample=None):
        """One launch: every environment listed in ``ids`` (a cuda int32 tensor as ``TaskPostPhysics.begin`` returns it -- r where environment r is
        reset, -1 elsewhere; None: all of them) has its force and slip rows zeroed and, where ``resample`` (None: the spec's resample is
        ``"reset"``), draws its coefficient anew and counts the draw.  Stream-ordered, no host synchronisation."""
        h = self._bound()
        if resample is None:
            resample = self.spec is not None and self.spec.resample == "reset"
        if resample and self.spec is None:
            raise ValueError("the friction has no spec to draw from")
        ptr, k = self._ids(ids)
        lo, hi, buckets = (0.0, 0.0, 0) if self.spec is None else (float(self.spec.range[0]), float(self.spec.range[1]), int(self.spec.buckets))
        check(lib().mpc_friction_draw(h, ptr, k, lo, hi, buckets, int(bool(resample)), _lib.stream(self.device)), "mpc_friction_draw")
        self.launches += 1

    def get_mu(self):
        """The coefficients on the host: [n] float64.  Synchronous."""
        m = np.zeros(self.n, np.float64)
        check(lib().mpc_friction_get_mu(self._bound(), m.ctypes.data), "mpc_friction_get_mu")
        return m

    def set_mu(self, mu):
        """Overwrite the coefficients from a number or a host array [n] (>= 0, not NaN).  Synchronous."""
        m = _mu_array(mu, self.n)                      # (a local: the array lives until the call has returned)
        check(lib().mpc_friction_set_mu(self._bound(), m.ctypes.data), "mpc_friction_set_mu")

    def state_dict(self):
        import torch
        return {"mu": torch.from_numpy(self.get_mu()), "counters": torch.from_numpy(self.get_counters().astype(np.int64))}

    def load_state_dict(self, state):
        self.set_mu(_lib.host_array(state["mu"], np.float64))
        self.set_counters(_lib.host_array(state["counters"], np.uint32))
