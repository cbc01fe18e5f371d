"""Opt-in contact reward terms and friction-aware critic columns on the device (csrc/mpc_contact_terms.h, csrc/mpc_contact_terms.hip,
csrc/contact_terms.h).

``friction.Friction`` gives every robot a friction coefficient of its own, and the plant's step publishes each foot's ground reaction and slide.
This unit reads them.  It adds three reward terms by their published formulas -- ``feet_slip`` (the squared mean sliding speed of the feet over the
tick), ``feet_contact_forces`` (what each foot's reaction exceeds ``max_contact_force`` by) and ``feet_stumble`` (a reaction outside a world-frame
cone of 5) --, puts them inside the reward's clip, keeps per-term episode sums with a window record for ``PPOTrainer.learn``, and with
``privileged=True`` widens the critic's privileged row by sixteen columns: the coefficient, the twelve force components, three zeros::

    fr = Friction(n, FrictionSpec(range=(0.1, 1.25), resample="reset"), seed=3)
    contact = ContactTerms(n, ContactSpec(feet_slip=-0.1, feet_contact_forces=-0.01), cfg=cfg, privileged=True)
    task = BatchedRLTask(robot_type, gait_id, cfg, friction=fr, privileged_obs=PrivilegedObs(n), contact_terms=contact)
    PPOTrainer(task).learn(k)            # records carry contact_terms: rew_<term>

``BatchedRLTask.step`` calls ``close`` inside its ``resets`` stage, ``run`` right after ``reward_shaping.run`` (after ``finish`` without shaping) and
``extend`` inside its ``privileged_obs`` stage.  Callers with a simulator of their own call the three themselves.

Each scale is the per-second value times ``cfg.dt``, as ``ShapingSpec.scales`` does it.  A term whose scale is 0 is not evaluated: it adds nothing to
the reward and its sum stays 0.  The reward is ``max(s + feet_slip + feet_contact_forces + feet_stumble, 0)`` (+ the shaping ``termination``), ``s``
being the unclipped sum the step without the unit clips.  csrc/contact_terms.h lists what is not legged_gym's: ``feet_slip`` has no contact filter
and reads a mean speed; on the tick that performs a reset the three terms are 0; on this plant ``feet_stumble`` fires only outside a world-frame
cone of 5, so only with a large mu or on steep ground (the plant has no foot-edge collision).

Not built: passing the plant's mu to the controller, per-level terrain friction, joint and torque limit terms.

The spec's validation is host arithmetic and needs no GPU; the kernels do (MpcLibraryError without one, no CPU fallback).
"""
import ctypes as C
import math
from dataclasses import dataclass

from . import _lib, toy_sim
from ._lib import cd, ci, pvp, text, vp
from .rl_task import TaskConfig

CONTACT_TERMS = ("feet_slip", "feet_contact_forces", "feet_stumble")
NUM_TERMS = len(CONTACT_TERMS)
# summary()'s layout (cterms::kSum*)
S_CLOSED, S_TERMS, S_EPISODE_S, SUMMARY_LEN = 0, 1, 1 + NUM_TERMS, 2 + NUM_TERMS
WINDOW_LEN = 1 + NUM_TERMS
COLUMNS = 16                           # what ``extend`` widens the privileged row by
NUM_SHAPING_TERMS = 8                  # reward_shaping.NUM_TERMS

# the entry points of csrc/mpc_contact_terms.h (bound here, not in any other module's list)
DECLS = {
    "mpc_contact_create": (ci, [pvp, ci, vp, vp, cd, cd, cd, cd, cd]),
    "mpc_contact_destroy": (None, [vp]),
    "mpc_contact_bind": (ci, [vp, vp]),
    "mpc_contact_close": (ci, [vp, vp, vp]),
    "mpc_contact_run": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mpc_contact_extend": (ci, [vp, vp, ci, vp, vp]),
    "mpc_contact_summary": (ci, [vp, vp, vp]),
    "mpc_contact_new_window": (ci, [vp, vp]),
    "mpc_contact_arrays": (ci, [vp, pvp, pvp, pvp]),
    "mpc_contact_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what bind takes) with these entry points bound
check = _lib.checker(lib, "mpc_contact_last_error")


@dataclass
class ContactSpec:
    """The three per-second scales (0.0: the term is off), the force [N] ``feet_contact_forces`` pays above, and what shapes the critic's columns:
    the forces are multiplied by ``force_scale`` (and clipped to the task's ``clip_observations``), the coefficient is clipped from above to
    ``mu_clip``."""
    feet_slip: float = 0.0
    feet_contact_forces: float = 0.0
    feet_stumble: float = 0.0
    max_contact_force: float = 100.0
    force_scale: float = 0.01
    mu_clip: float = 2.0

    def validate(self):
        numbers = [float(getattr(self, name)) for name in CONTACT_TERMS] + [float(self.max_contact_force), float(self.force_scale), float(self.mu_clip)]
        if not all(math.isfinite(v) for v in numbers):
            raise ValueError("contact terms: the scales, max_contact_force, force_scale and mu_clip must be finite")
        if not self.max_contact_force >= 0:
            raise ValueError("contact terms: max_contact_force must be >= 0")
        if not (self.force_scale > 0 and self.mu_clip > 0):
            raise ValueError("contact terms: force_scale and mu_clip must be > 0")
        return self

    def scales(self, dt):
        """The three scales x dt, in CONTACT_TERMS order (a Python float product, as ``ShapingSpec.scales``)."""
        return [float(getattr(self, name)) * float(dt) for name in CONTACT_TERMS]


class ContactTerms:
    """The contact terms of ``n`` environments under ``spec`` and ``cfg`` (keyword-only: the task's own ``TaskConfig``, whose ``dt``, episode length,
    ``clip_observations`` and six reward scales the unit reads; None is ``TaskConfig()``, and ``BatchedRLTask`` refuses a unit made under another
    one).  ``privileged=True`` asks the task to widen the critic's privileged row with ``extend``.  The handle is host memory until ``bind(sim)``;
    from then on cuda tensor views over its memory, valid while the object lives: ``sums`` [n, 3] float32 (``CONTACT_TERMS`` order), ``ticks`` [n]
    int32, ``window`` [4] float64 (the closed count and the three sums).  ``terms_buf`` (None, or a [n, 3] float32 cuda tensor the caller sets)
    receives every tick's three terms when ``run`` is given no ``terms``."""

    def __init__(self, n, spec=None, device=None, *, cfg=None, privileged=False):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("n must be at least 1")
        self.spec = (spec if spec is not None else ContactSpec()).validate()
        self.cfg = cfg if cfg is not None else TaskConfig()
        self.privileged = bool(privileged)
        self.device = device
        self.terms_buf = None
        self.sim = None
        self.sums = self.ticks = self.window = self._summary = None
        self.max_episode_length_s = float(self.cfg.episode_length_s)
        cs = self.cfg._struct()
        scales = (C.c_double * NUM_TERMS)(*self.spec.scales(self.cfg.dt))
        self._handle = C.c_void_p()
        check(lib().mpc_contact_create(C.byref(self._handle), self.n, C.addressof(cs), C.addressof(scales), float(self.spec.max_contact_force),
                                       float(self.spec.force_scale), float(self.spec.mu_clip), float(self.cfg.dt), self.max_episode_length_s),
              "mpc_contact_create")

    __del__ = _lib.finalizer("mpc_contact_destroy")

    def bind(self, sim):
        """Keep the device addresses of a ``BatchedToySim``'s friction coefficients and of the force and slip rows its step fills (the sim has a
        ``friction.Friction`` bound), and put the unit's own arrays on the sim's device.  Once per object."""
        import torch
        _lib.need_gpu("ContactTerms")
        self.device = _lib.device_of(sim.device if self.device is None else self.device)
        check(lib().mpc_contact_bind(self._handle, sim._handle), "mpc_contact_bind")
        self.sim = sim                     # (the rows live as long as the sim does)
        p = [C.c_void_p() for _ in range(3)]
        check(lib().mpc_contact_arrays(self._handle, *(C.byref(x) for x in p)), "mpc_contact_arrays")
        view = lambda i, shape, typestr: _lib.device_view(p[i].value, shape, typestr, self.device)
        self.sums, self.ticks, self.window = view(0, (self.n, NUM_TERMS), "<f4"), view(1, (self.n,), "<i4"), view(2, (WINDOW_LEN,), "<f8")
        self._summary = torch.zeros((SUMMARY_LEN,), dtype=torch.float64, device=self.device)

    def close(self, reset_ids):
        """After the task's ``begin``: ``reset_ids`` [n] int32 (r where environment r is being reset, -1 elsewhere).  Two launches, stream-ordered."""
        import torch
        _lib.tensor_arg(reset_ids, torch.int32, self.n, "reset_ids")
        check(lib().mpc_contact_close(self._handle, reset_ids.data_ptr(), _lib.stream(self.device)), "mpc_contact_close")

    def run(self, root_states, commands, torques, fell, reset_ids, rew_buf, shaping_terms=None, shaping_scales=None, terms=None):
        """After the task's ``finish`` and, with reward shaping, after ``RewardShaping.run``, on what they read and wrote: root_states [n, 13], commands
        [n, 3], torques [n, 12] float32, ``fell`` [n] bool / uint8 or None, reset_ids [n] int32; ``shaping_terms`` [n, 8] float32 is the tensor
        ``RewardShaping.run`` has just written and ``shaping_scales`` that unit's ``spec.scales(cfg.dt)`` (both None without shaping); ``rew_buf`` [n]
        float32 is rewritten.  ``terms`` [n, 3] float32 (default: ``terms_buf``) receives the tick's three terms.  One launch, stream-ordered."""
        import torch
        n = self.n
        terms = self.terms_buf if terms is None else terms
        for name, t, numel in (("root_states", root_states, n * 13), ("commands", commands, n * 3), ("torques", torques, n * 12), ("rew_buf", rew_buf, n)):
            _lib.tensor_arg(t, torch.float32, numel, name)
        _lib.tensor_arg(reset_ids, torch.int32, n, "reset_ids")
        if (shaping_terms is None) != (shaping_scales is None):
            raise ValueError("shaping_terms goes with shaping_scales")
        scales = None
        if shaping_terms is not None:
            _lib.tensor_arg(shaping_terms, torch.float32, n * NUM_SHAPING_TERMS, "shaping_terms")
            if len(shaping_scales) != NUM_SHAPING_TERMS:
                raise ValueError(f"shaping_scales: {NUM_SHAPING_TERMS} numbers expected")
            scales = (C.c_double * NUM_SHAPING_TERMS)(*(float(v) for v in shaping_scales))
        if terms is not None:
            _lib.tensor_arg(terms, torch.float32, n * NUM_TERMS, "terms")
        fell_ptr = None if fell is None else _lib.flag_arg(fell, n, "fell").data_ptr()
        check(lib().mpc_contact_run(self._handle, root_states.data_ptr(), commands.data_ptr(), torques.data_ptr(), fell_ptr, reset_ids.data_ptr(),
                                    None if shaping_terms is None else shaping_terms.data_ptr(), None if scales is None else C.addressof(scales),
                                    rew_buf.data_ptr(), None if terms is None else terms.data_ptr(), _lib.stream(self.device)), "mpc_contact_run")

    def width(self, privileged_width):
        """The width of the row ``extend`` writes for an assembled row of ``privileged_width`` columns."""
        return int(privileged_width) + COLUMNS

    def extend(self, priv_row, out):
        """After ``PrivilegedObs.assemble``: ``priv_row`` [n, Wp] float32 (Wp a multiple of 16) is copied bit for bit into ``out`` [n, Wp + 16], followed
        by the friction coefficient clipped to ``mu_clip``, the twelve force components times ``force_scale`` clipped to ``clip_observations``, and
        three zeros.  One launch, stream-ordered."""
        import torch
        if priv_row.dim() != 2 or priv_row.shape[0] != self.n or priv_row.shape[1] < 16 or priv_row.shape[1] % 16:
            raise ValueError(f"priv_row: [{self.n}, Wp] with Wp a multiple of 16 expected")
        wp = int(priv_row.shape[1])
        _lib.tensor_arg(priv_row, torch.float32, self.n * wp, "priv_row")
        if out.dim() != 2 or tuple(out.shape) != (self.n, wp + COLUMNS):
            raise ValueError(f"out: [{self.n}, {wp + COLUMNS}] expected")
        _lib.tensor_arg(out, torch.float32, self.n * (wp + COLUMNS), "out")
        check(lib().mpc_contact_extend(self._handle, priv_row.data_ptr(), wp, out.data_ptr(), _lib.stream(self.device)), "mpc_contact_extend")
        return out

    def summary(self):
        """float64 [5] on the device (the same tensor on every call): the episodes closed since the last ``new_window``, the three sums of their
        terms, ``max_episode_length_s``.  Stream-ordered."""
        check(lib().mpc_contact_summary(self._handle, self._summary.data_ptr(), _lib.stream(self.device)), "mpc_contact_summary")
        return self._summary

    def new_window(self):
        """Zero the window accumulators.  Stream-ordered."""
        check(lib().mpc_contact_new_window(self._handle, _lib.stream(self.device)), "mpc_contact_new_window")

    @staticmethod
    def record(values):
        """``summary().tolist()`` as the ``contact_terms`` entry of a training record: ``rew_<term>`` is the window's term sum per closed episode and
        per second of a full episode (0.0 when nothing closed)."""
        closed, seconds = values[S_CLOSED], values[S_EPISODE_S]
        return {"rew_" + name: (values[S_TERMS + i] / closed / seconds if closed > 0 else 0.0) for i, name in enumerate(CONTACT_TERMS)}
