"""Opt-in legged_gym reward shaping terms on the device (csrc/mpc_reward_shaping.h, csrc/mpc_reward_shaping.hip, csrc/reward_shaping.h).

The task pays the reference's six reward terms.  This unit adds eight of legged_gym's, by their published formulas -- ``orientation``,
``base_height`` (over the measured heights of the scan), ``dof_vel``, ``dof_acc``, ``action_rate``, ``feet_air_time``, ``stand_still``,
``termination`` --, rewrites ``rew_buf`` with the fourteen, and keeps per-term episode sums with a window record for ``PPOTrainer.learn``::

    shaping = RewardShaping(n, ShapingSpec(orientation=-0.2, base_height=-1.0, action_rate=-0.01, base_height_target=0.3), cfg=cfg)
    task = BatchedRLTask(robot_type, gait_id, cfg, terrain=terrain, height_scan=scan, reward_shaping=shaping)
    PPOTrainer(task).learn(k)            # records carry reward_shaping: rew_<term>

``BatchedRLTask.step`` calls ``close`` inside its ``resets`` stage and ``run`` after the height scan (after ``finish`` without one), on the tensors
``finish`` read and wrote.  Callers with a simulator of their own call the two themselves.

Each scale is the per-second value times ``cfg.dt``, as ``TaskConfig.reward_scales()`` does it.  A term whose scale is 0 is not evaluated: it adds
nothing to the reward and its sum stays 0.  The reward is ``max(task terms + orientation .. stand_still, 0) + termination``.

Not legged_gym's (csrc/reward_shaping.h has the list): the history is reset on the tick that performs the reset, where the terms that read it are 0;
``stand_still`` and ``feet_air_time`` share one ``moving`` flag; ``termination`` uses ``finish``'s own time-out clause; the record is episode-weighted
over the iteration; an episode whose sums are not all finite closes nothing.

The spec's validation is host arithmetic and needs no GPU; the kernels do (MpcLibraryError without one, no CPU fallback).
"""
import ctypes as C
import math
from dataclasses import dataclass

from . import _lib, toy_sim
from ._lib import cd, ci, pvp, text, vp
from .rl_task import TaskConfig

SHAPING_TERMS = ("orientation", "base_height", "dof_vel", "dof_acc", "action_rate", "feet_air_time", "stand_still", "termination")
NUM_TERMS = len(SHAPING_TERMS)
# summary()'s layout (rshape::kSum*)
S_CLOSED, S_TERMS, S_EPISODE_S, SUMMARY_LEN = 0, 1, 1 + NUM_TERMS, 2 + NUM_TERMS
WINDOW_LEN = 1 + NUM_TERMS
MAX_POINTS = 208                       # height_scan.MAX_POINTS

# the entry points of csrc/mpc_reward_shaping.h (bound here, not in any other module's list)
DECLS = {
    "mpc_shaping_create": (ci, [pvp, ci, vp, vp, cd, cd, cd, cd]),
    "mpc_shaping_destroy": (None, [vp]),
    "mpc_shaping_bind": (ci, [vp, vp]),
    "mpc_shaping_close": (ci, [vp, vp, vp]),
    "mpc_shaping_run": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp]),
    "mpc_shaping_summary": (ci, [vp, vp, vp]),
    "mpc_shaping_new_window": (ci, [vp, vp]),
    "mpc_shaping_arrays": (ci, [vp, pvp, pvp, pvp, pvp, pvp, pvp, pvp]),
    "mpc_shaping_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what bind takes) with these entry points bound
check = _lib.checker(lib, "mpc_shaping_last_error")


@dataclass
class ShapingSpec:
    """The eight per-second scales (0.0: the term is off), the height ``base_height`` aims at and the air time ``feet_air_time`` pays from."""
    orientation: float = 0.0
    base_height: float = 0.0
    dof_vel: float = 0.0
    dof_acc: float = 0.0
    action_rate: float = 0.0
    feet_air_time: float = 0.0
    stand_still: float = 0.0
    termination: float = 0.0
    base_height_target: float = 0.0
    air_time_target: float = 0.5

    def validate(self):
        numbers = [float(getattr(self, name)) for name in SHAPING_TERMS] + [float(self.base_height_target), float(self.air_time_target)]
        if not all(math.isfinite(v) for v in numbers):
            raise ValueError("reward shaping: the scales, base_height_target and air_time_target must be finite")
        if not self.air_time_target >= 0:
            raise ValueError("reward shaping: air_time_target must be >= 0")
        return self

    def scales(self, dt):
        """The eight scales x dt, in SHAPING_TERMS order (a Python float product, as ``TaskConfig.reward_scales()``)."""
        return [float(getattr(self, name)) * float(dt) for name in SHAPING_TERMS]


class RewardShaping:
    """The shaping terms of ``n`` environments under ``spec`` and ``cfg`` (keyword-only: the task's own ``TaskConfig``, whose ``dt``, episode length,
    ``default_dof_pos`` and six reward scales the unit reads; None is ``TaskConfig()``, and ``BatchedRLTask`` refuses a unit made under another one).
    Cuda tensor views over the handle's memory, valid while the object lives: ``last_actions``, ``last_dof_vel`` [n, 12] and ``air_time`` [n, 4] float32, ``last_contact`` [n, 4] int32,
    ``sums`` [n, 8] float32 (``SHAPING_TERMS`` order), ``ticks`` [n] int32, ``window`` [9] float64 (the closed count and the eight sums).
    ``terms_buf`` (None, or a [n, 8] float32 cuda tensor the caller sets) receives every tick's eight terms when ``run`` is given no ``terms``."""

    def __init__(self, n, spec=None, device=None, *, cfg=None):
        import torch
        self.n = int(n)
        if self.n < 1:
            raise ValueError("n must be at least 1")
        self.spec = (spec if spec is not None else ShapingSpec()).validate()
        self.cfg = cfg if cfg is not None else TaskConfig()
        _lib.need_gpu("RewardShaping")
        self.device = _lib.device_of(device)
        self.terms_buf = None
        self.sim = None
        self.max_episode_length_s = float(self.cfg.episode_length_s)
        cs = self.cfg._struct()
        scales = (C.c_double * NUM_TERMS)(*self.spec.scales(self.cfg.dt))
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().mpc_shaping_create(C.byref(self._handle), self.n, C.addressof(cs), C.addressof(scales), float(self.spec.base_height_target),
                                           float(self.spec.air_time_target), float(self.cfg.dt), self.max_episode_length_s), "mpc_shaping_create")
        p = [C.c_void_p() for _ in range(7)]
        check(lib().mpc_shaping_arrays(self._handle, *(C.byref(x) for x in p)), "mpc_shaping_arrays")
        view = lambda i, shape, typestr: _lib.device_view(p[i].value, shape, typestr, self.device)
        self.last_actions, self.last_dof_vel = view(0, (self.n, 12), "<f4"), view(1, (self.n, 12), "<f4")
        self.air_time, self.last_contact = view(2, (self.n, 4), "<f4"), view(3, (self.n, 4), "<i4")
        self.sums, self.ticks, self.window = view(4, (self.n, NUM_TERMS), "<f4"), view(5, (self.n,), "<i4"), view(6, (WINDOW_LEN,), "<f8")
        self._summary = torch.zeros((SUMMARY_LEN,), dtype=torch.float64, device=self.device)

    __del__ = _lib.finalizer("mpc_shaping_destroy")

    def bind(self, sim):
        """Keep the device address of a ``BatchedToySim``'s state record, whose foot-contact flags ``feet_air_time`` reads."""
        check(lib().mpc_shaping_bind(self._handle, sim._handle), "mpc_shaping_bind")
        self.sim = sim                     # (the record lives as long as the sim does)

    def close(self, reset_ids):
        """After the task's ``begin``: ``reset_ids`` [n] int32 (r where environment r is being reset, -1 elsewhere).  Two launches, stream-ordered."""
        import torch
        _lib.tensor_arg(reset_ids, torch.int32, self.n, "reset_ids")
        check(lib().mpc_shaping_close(self._handle, reset_ids.data_ptr(), _lib.stream(self.device)), "mpc_shaping_close")

    def run(self, root_states, dof_state, actions, commands, torques, fell, reset_ids, reset_buf, progress_buf, rew_buf, heights=None, terms=None):
        """After the task's ``finish`` (and the height scan), on what it read and wrote: root_states [n, 13], dof_state [n * 12, 2], actions [n, 12],
        commands [n, 3], torques [n, 12] float32, ``fell`` [n] bool / uint8 or None, reset_ids [n] int32, reset_buf and progress_buf [n] int64,
        ``heights`` [n, P] float32 in metres or None; ``rew_buf`` [n] float32 is rewritten.  ``terms`` [n, 8] float32 (default: ``terms_buf``) receives
        the tick's eight terms.  One launch, stream-ordered."""
        import torch
        n = self.n
        terms = self.terms_buf if terms is None else terms
        for name, t, numel in (("root_states", root_states, n * 13), ("dof_state", dof_state, n * 24), ("actions", actions, n * 12),
                               ("commands", commands, n * 3), ("torques", torques, n * 12), ("rew_buf", rew_buf, n)):
            _lib.tensor_arg(t, torch.float32, numel, name)
        _lib.tensor_arg(reset_ids, torch.int32, n, "reset_ids")
        _lib.tensor_arg(reset_buf, torch.long, n, "reset_buf")
        _lib.tensor_arg(progress_buf, torch.long, n, "progress_buf")
        P = 0
        if heights is not None:
            if heights.dim() != 2 or heights.shape[0] != n or not 1 <= heights.shape[1] <= MAX_POINTS:
                raise ValueError(f"heights: [{n}, P] with 1 <= P <= {MAX_POINTS} expected")
            P = int(heights.shape[1])
            _lib.tensor_arg(heights, torch.float32, n * P, "heights")
        if terms is not None:
            _lib.tensor_arg(terms, torch.float32, n * NUM_TERMS, "terms")
        fell_ptr = None if fell is None else _lib.flag_arg(fell, n, "fell").data_ptr()
        check(lib().mpc_shaping_run(self._handle, root_states.data_ptr(), dof_state.data_ptr(), actions.data_ptr(), commands.data_ptr(), torques.data_ptr(),
                                    fell_ptr, reset_ids.data_ptr(), reset_buf.data_ptr(), progress_buf.data_ptr(), None if heights is None else heights.data_ptr(),
                                    P, rew_buf.data_ptr(), None if terms is None else terms.data_ptr(), _lib.stream(self.device)), "mpc_shaping_run")

    def summary(self):
        """float64 [10] on the device (the same tensor on every call): the episodes closed since the last ``new_window``, the eight sums of their
        terms, ``max_episode_length_s``.  Stream-ordered."""
        check(lib().mpc_shaping_summary(self._handle, self._summary.data_ptr(), _lib.stream(self.device)), "mpc_shaping_summary")
        return self._summary

    def new_window(self):
        """Zero the window accumulators.  Stream-ordered."""
        check(lib().mpc_shaping_new_window(self._handle, _lib.stream(self.device)), "mpc_shaping_new_window")

    @staticmethod
    def record(values):
        """``summary().tolist()`` as the ``reward_shaping`` entry of a training record: ``rew_<term>`` is the window's term sum per closed episode and
        per second of a full episode (0.0 when nothing closed)."""
        closed, seconds = values[S_CLOSED], values[S_EPISODE_S]
        return {"rew_" + name: (values[S_TERMS + i] / closed / seconds if closed > 0 else 0.0) for i, name in enumerate(SHAPING_TERMS)}
