"""Opt-in per-robot plant randomisation on the device (csrc/mpc_plant_rand.h, csrc/mpc_plant_rand.hip, csrc/plant_rand.h): every robot of a
``BatchedToySim`` gets a payload, a motor strength and a gravity of its own.

legged_gym's ``randomize_base_mass`` (``added_mass_range``) and the motor-strength and gravity randomisation of its descendants, by their published
algorithms, on the toy plant: a record of three float64 per robot -- ``payload`` [kg] added to the body's mass (the inertia is left alone, as Isaac
Gym's added base mass leaves it), ``strength``, a factor on all twelve joint torques, and ``grav_z`` [m/s^2], the absolute gravity -- that the plant's
step kernel consumes.  The record is drawn on the device at reset by a counter-based generator keyed by (seed, environment, draw index, axis): no
generator state, and a draw does not depend on the batch size::

    pr = PlantRand(n, PlantSpec(payload=(-1.0, 3.0), strength=(0.9, 1.1), gravity=(-1.0, 1.0)), seed=3)
    task = BatchedRLTask(robot_type, gait_id, cfg, plant_rand=pr, privileged_obs=PrivilegedObs(n, plant=True))
    PPOTrainer(task).learn(k)            # the critic sees the record, the actor and the MPC controller do not

``gravity`` is an OFFSET from -9.81.  The MPC controller keeps planning with the robot table's nominal mass and gravity while the plant disagrees:
that mismatch is what the weight policy is trained to cope with.  Without the option a sim launches the kernels it launched before; with the neutral
record (0, 1, -9.81) the parametrised kernel computes the same state bit for bit.

Not built: COM displacement, inertia scaling.  (Friction is ``friction.Friction``, an option of its own that works together with this one.)

``PlantSpec`` and ``PlantRand.validate`` are host arithmetic and need no GPU; the kernels do (MpcLibraryError without one, no CPU fallback).
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib, toy_sim
from ._lib import ci, pvp, text, vp
from .quadruped import ROBOT_TABLE64

AXES = ("payload", "strength", "gravity")
GRAV_Z = -9.81                         # csrc/toy_sim.h's kGravZ
NEUTRAL = (0.0, 1.0, GRAV_Z)           # the record of a robot that has not drawn: (payload, strength, grav_z)
COL_MASS = 6                           # ROBOT_TABLE64's mass column
RESAMPLE = ("reset", "once")

# the entry points of csrc/mpc_plant_rand.h (bound here, not in any other module's list)
DECLS = {
    "mpc_plant_rand_create": (ci, [pvp, ci, C.c_ulonglong]),
    "mpc_plant_rand_destroy": (None, [vp]),
    "mpc_plant_rand_attach": (ci, [vp, vp]),
    "mpc_plant_rand_draw": (ci, [vp, vp, ci, vp, vp, vp]),
    "mpc_plant_rand_get_params": (ci, [vp, vp]),
    "mpc_plant_rand_set_params": (ci, [vp, vp, vp]),
    "mpc_plant_rand_get_counters": (ci, [vp, vp]),
    "mpc_plant_rand_set_counters": (ci, [vp, vp]),
    "mpc_plant_rand_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what attach takes) with these entry points bound
check = _lib.checker(lib, "mpc_plant_rand_last_error")


@dataclass
class PlantSpec:
    """``payload`` [kg], ``strength`` [factor] and ``gravity`` [m/s^2, an offset from -9.81]: each ``(lo, hi)`` for a uniform draw or None for the
    neutral value.  ``resample``: ``"reset"`` draws an environment's record anew at each of its resets, ``"once"`` draws every record once, when the
    task is built."""
    payload: tuple = None
    strength: tuple = None
    gravity: tuple = None
    resample: str = "reset"

    def ranges(self):
        return (self.payload, self.strength, self.gravity)

    def validate(self, robot_type=None):
        """Everything that can be refused without the device.  ``robot_type``: the robot types in use (rows of ``ROBOT_TABLE64``); the lowest
        payload, as the float32 the kernel draws with, must leave each of them a positive mass."""
        if self.resample not in RESAMPLE:
            raise ValueError(f"plant: resample {self.resample!r}: 'reset' or 'once'")
        for name, rng in zip(AXES, self.ranges()):
            if rng is None:
                continue
            with np.errstate(over="ignore"):       # (a bound beyond float32's range becomes inf, and is refused as such)
                finite = len(rng) == 2 and all(math.isfinite(float(v)) and math.isfinite(float(np.float32(v))) for v in rng)
            if not finite:
                raise ValueError(f"plant: {name} must be (lo, hi), two numbers that are finite as float32")
            if float(rng[0]) > float(rng[1]):
                raise ValueError(f"plant: {name} range with lo > hi")
        if self.strength is not None and float(self.strength[0]) < 0:
            raise ValueError("plant: strength lo must be >= 0")
        if self.payload is not None and robot_type is not None:
            lo = float(np.float32(self.payload[0]))
            for rt in sorted(set(int(t) for t in np.asarray(robot_type).reshape(-1))):
                mass = float(ROBOT_TABLE64[rt][COL_MASS])
                if not mass + lo > 0.0:
                    raise ValueError(f"plant: a payload of {lo} kg leaves robot type {rt} (mass {mass} kg) without a positive mass")


class PlantRand(_lib.DrawnRecord):
    """The plant records of ``n`` environments.  ``bind(sim)`` attaches the record to a ``BatchedToySim`` (whose ``step`` consumes it from then
    on), ``draw(ids)`` is the one launch per reset; ``BatchedRLTask(plant_rand=...)`` does both.  ``get_params`` / ``set_params`` move the record
    [n, 3] (payload, strength, grav_z) between host and device, ``state_dict`` / ``load_state_dict`` the record and the draw counters."""
    WHAT, COUNTERS = "plant randomisation", (lib, check, "mpc_plant_rand_get_counters", "mpc_plant_rand_set_counters")
    __del__ = _lib.finalizer("mpc_plant_rand_destroy")

    def __init__(self, n, spec=None, seed=0, device=None):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("n must be at least 1")
        self.spec = spec if spec is not None else PlantSpec()
        self.seed = int(seed) & (2 ** 64 - 1)
        self.spec.validate()
        self.device = device
        self.launches = 0
        self._handle, self.sim, self._mass = None, None, None
        self._present = (C.c_int * 3)(*[int(r is not None) for r in self.spec.ranges()])
        self._ranges = (C.c_double * 6)(*[float(v) for r in self.spec.ranges() for v in (r if r is not None else (0.0, 0.0))])

    def validate(self, n=None, robot_type=None):
        """Everything that can be refused without the device; the task calls it with its batch size and its robot types."""
        if n is not None and int(n) != self.n:
            raise ValueError(f"the plant randomisation holds {self.n} environments, the task {int(n)}")
        self.spec.validate(robot_type)

    def _ensure(self):
        if self._handle is None:
            import torch
            _lib.need_gpu("PlantRand")
            self.device = _lib.device_of(self.device)
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                check(lib().mpc_plant_rand_create(C.byref(h), self.n, self.seed), "mpc_plant_rand_create")
            self._handle = h
        return self._handle

    def bind(self, sim):
        """Give ``sim`` (a ``BatchedToySim`` with ``n`` robots) its plant record, neutral, and this object its draw counters, zero.  Once."""
        check(lib().mpc_plant_rand_attach(self._ensure(), sim._handle), "mpc_plant_rand_attach")
        self.sim = sim
        rt = getattr(sim, "robot_type", None)
        self._mass = None if rt is None else np.ascontiguousarray(ROBOT_TABLE64[np.asarray(rt, dtype=np.int64), COL_MASS], dtype=np.float64)

    def draw(self, ids=None):
        """One launch: every environment listed in ``ids`` (a cuda int32 tensor as ``TaskPostPhysics.begin`` returns it -- r where environment r is
        reset, -1 elsewhere; None: all of them) draws its record anew and counts the draw.  Stream-ordered, no host synchronisation."""
        h = self._bound()
        ptr, k = self._ids(ids)
        check(lib().mpc_plant_rand_draw(h, ptr, k, self._present, self._ranges, _lib.stream(self.device)), "mpc_plant_rand_draw")
        self.launches += 1

    def get_params(self):
        """The record on the host: [n, 3] float64 (payload, strength, grav_z).  Synchronous."""
        p = np.zeros((self.n, 3), np.float64)
        check(lib().mpc_plant_rand_get_params(self._bound(), p.ctypes.data), "mpc_plant_rand_get_params")
        return p

    def set_params(self, params):
        """Overwrite the record from a host array [n, 3] (finite, strength >= 0, mass + payload > 0).  Synchronous."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.shape != (self.n, 3):
            raise ValueError(f"params: [{self.n}, 3] expected")
        h = self._bound()
        check(lib().mpc_plant_rand_set_params(h, p.ctypes.data, None if self._mass is None else self._mass.ctypes.data), "mpc_plant_rand_set_params")

    def state_dict(self):
        import torch
        return {"params": torch.from_numpy(self.get_params()), "counters": torch.from_numpy(self.get_counters().astype(np.int64))}

    def load_state_dict(self, state):
        self.set_params(_lib.host_array(state["params"], np.float64))
        self.set_counters(_lib.host_array(state["counters"], np.uint32))
