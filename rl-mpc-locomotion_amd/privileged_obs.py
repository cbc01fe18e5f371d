"""Privileged critic observations on the device (csrc/mpc_privileged_obs.h, csrc/mpc_privileged_obs.hip, csrc/privileged_obs.h).

rsl_rl's asymmetric actor-critic seam (``num_critic_obs``, ``env.get_privileged_observations()``) filled the way legged_gym fills it: the critic sees
the observation row BEFORE the observation noise, and a few columns the actor never sees.  One kernel per tick writes one float32 row per
environment::

    columns 0 .. 47            the task's 48 observation columns, before any observation noise
    columns 48 .. 48 + P - 1   the height scan's P columns as ``HeightScan.measure`` wrote them, before noise (P = 0 without a scan)
    4 columns                  the plant's foot-contact flags FL FR RL RR as 0.0 / 1.0, read from the sim's state record on the device
    1 column                   the episode phase: float32(progress_buf) * float32(1 / max_episode_length)
    zeros                      up to ``privileged_width(P)`` = 16 * ceil((48 + P + 5) / 16): 64 without a scan, 240 with the default 17 x 11 scan

    task = BatchedRLTask(robot_type, gait_id, terrain=terrain, height_scan=scan, domain_rand=dr, privileged_obs=PrivilegedObs(n))
    PPOTrainer(task).learn(k)              # the critic's first layer, the storage and the update take num_privileged_obs from the task

With ``PrivilegedObs(n, plant=True)`` and a ``plant_rand.PlantRand`` in the task, three columns follow the phase -- the plant's per-robot record as
``float32(payload)``, ``float32(strength - 1.0)``, ``float32(grav_z + 9.81)`` -- and the row is 16 * ceil((48 + P + 5 + 3) / 16) wide: still 64 without
a scan, 256 with the default one.  Not in this row: friction -- ``contact_terms.ContactTerms(privileged=True)`` widens the row by the
plant's friction coefficient and its ground reactions (sixteen columns, one more launch).

The entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib, toy_sim
from ._lib import cd, ci, need_gpu, pvp, text, vp

NUM_TASK_OBS = 48                      # columns 0 .. 47: the task's row
SCAN_OFFSET = NUM_TASK_OBS             # where the height scan's P columns start
NUM_CONTACTS = 4                       # FL FR RL RR
NUM_EXTRA = NUM_CONTACTS + 1           # the contacts and the phase
NUM_PLANT = 3                          # with plant=True: payload, strength - 1, grav_z + 9.81
MAX_SCAN = 208                         # height_scan.MAX_POINTS

# the entry points of csrc/mpc_privileged_obs.h (bound here, not in any other module's list)
DECLS = {
    "mpc_privobs_width": (ci, [ci]),
    "mpc_privobs_create": (ci, [pvp, ci]),
    "mpc_privobs_destroy": (None, [vp]),
    "mpc_privobs_bind": (ci, [vp, vp]),
    "mpc_privobs_run": (ci, [vp, vp, ci, ci, vp, cd, vp, vp]),
    "mpc_privobs_width_plant": (ci, [ci]),
    "mpc_privobs_bind_plant": (ci, [vp, vp]),
    "mpc_privobs_run_plant": (ci, [vp, vp, ci, ci, vp, cd, vp, vp]),
    "mpc_privobs_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what bind takes) with these entry points bound
check = _lib.checker(lib, "mpc_privobs_last_error")


def contact_offset(num_scan=0):
    """The first of the four contact columns."""
    return NUM_TASK_OBS + int(num_scan)


def phase_offset(num_scan=0):
    """The episode-phase column."""
    return NUM_TASK_OBS + int(num_scan) + NUM_CONTACTS


def plant_offset(num_scan=0):
    """The first of the three plant columns of a row with ``plant=True``."""
    return NUM_TASK_OBS + int(num_scan) + NUM_EXTRA


def privileged_width(num_scan=0, plant=False):
    """The row's length ``Wp`` for a scan of ``num_scan`` points: 48 + P + 5 (+ 3 with the plant columns) rounded up to a multiple of 16 (needs
    no device)."""
    num_scan = int(num_scan)
    if not 0 <= num_scan <= MAX_SCAN:
        raise ValueError(f"{num_scan} scan columns: 0 .. {MAX_SCAN}")
    return 16 * ((NUM_TASK_OBS + num_scan + NUM_EXTRA + (NUM_PLANT if plant else 0) + 15) // 16)


def inverse_length(max_episode_length):
    """float32(1 / max_episode_length): what the kernel multiplies the episode counter by."""
    return np.float32(1.0 / float(max_episode_length))


class PrivilegedObs:
    """The privileged rows of ``n`` environments.  ``bind(sim)`` keeps the device address of a ``BatchedToySim``'s state record;
    ``assemble`` is the one launch per tick.  ``BatchedRLTask(privileged_obs=...)`` does both.  ``plant=True``: the row carries the three plant
    columns; ``bind_plant(sim)`` keeps the address of the sim's plant record (``PlantRand.bind`` made it) and is required before ``assemble``."""

    def __init__(self, n, device=None, plant=False):
        self.n = int(n)
        self.plant = bool(plant)
        need_gpu("PrivilegedObs")
        self.device = _lib.device_of(device)
        self._handle = C.c_void_p()
        check(lib().mpc_privobs_create(C.byref(self._handle), self.n), "mpc_privobs_create")
        self.sim = None

    __del__ = _lib.finalizer("mpc_privobs_destroy")

    def bind(self, sim):
        check(lib().mpc_privobs_bind(self._handle, sim._handle), "mpc_privobs_bind")
        self.sim = sim                     # (the record lives as long as the sim does)

    def bind_plant(self, sim):
        check(lib().mpc_privobs_bind_plant(self._handle, sim._handle), "mpc_privobs_bind_plant")

    def width(self, num_scan=0):
        return privileged_width(num_scan, self.plant)

    def assemble(self, obs, progress_buf, inv_len, num_scan=0, out=None):
        """``obs`` [n, W] (contiguous cuda float32, W >= 48 + num_scan: the task's row or the height scan's wide row, before noise) and
        ``progress_buf`` [n] int64 -> ``out`` [n, privileged_width(num_scan, plant)], the whole row, pad included.  ``inv_len``: ``inverse_length(...)``.
        ``out`` is allocated when it is None.  Stream-ordered, no host synchronisation."""
        import torch
        if obs.dim() != 2 or obs.shape[0] != self.n:
            raise ValueError(f"obs: [{self.n}, W] expected")
        w_in = int(obs.shape[1])
        _lib.tensor_arg(obs, torch.float32, self.n * w_in, "obs")
        _lib.tensor_arg(progress_buf, torch.long, self.n, "progress_buf")
        wp = privileged_width(num_scan, self.plant)
        run, name = (lib().mpc_privobs_run_plant, "mpc_privobs_run_plant") if self.plant else (lib().mpc_privobs_run, "mpc_privobs_run")
        if out is None:
            out = torch.empty((self.n, wp), dtype=torch.float32, device=self.device)
        _lib.tensor_arg(out, torch.float32, self.n * wp, "out")
        check(run(self._handle, obs.data_ptr(), w_in, int(num_scan), progress_buf.data_ptr(), float(np.float32(inv_len)), out.data_ptr(),
                  _lib.stream(self.device)), name)
        return out
