"""Opt-in domain randomisation on the device (csrc/mpc_domain_rand.h, csrc/mpc_domain_rand.hip, csrc/domain_rand.h): noise on the observations
and on the actions, and random pushes of the base.

The noise restates the hook the reference carries and never calls: ``VecTask.apply_randomizations`` (RL_Environment/tasks/base/vec_task.py:491-599)
builds a ``noise_lambda`` for ``observations`` and for ``actions`` -- gaussian or uniform, additive or scaling, a correlated term drawn once and kept,
a ``linear`` / ``constant`` schedule, a ``frequency`` -- and ``VecTask.step`` applies them before the action clamp (:308-312) and before the observation
clamp (:331-337).  Here each is one kernel on the matrix, with counter-based draws keyed by (seed, environment, tick, column): no generator state, and
a draw does not depend on the batch size.  The pushes restate legged_gym's ``_push_robots`` by its published algorithm::

    dr = DomainRand(n, observations=NoiseSpec.legged_gym(cfg, height_scan=scan), push=PushSpec(), seed=3)
    task = BatchedRLTask(robot_type, gait_id, cfg, terrain=terrain, height_scan=scan, domain_rand=dr)
    PPOTrainer(task).learn(k)            # unchanged: it sees only obs_buf
    dr.enabled = False                   # an evaluation run: the step runs the launches it runs without the option

``DomainRand.from_dr_params`` takes IsaacGymEnvs' ``task.randomization_params`` dictionary.

Not the reference's: the draws are this package's generator, so parity with ``torch.randn_like`` / ``rand_like`` is in distribution only; the correlated
term is a function of (seed, environment, column) for the whole run, where the reference draws a new one each time the parameters are recomputed; and
the task's 48 columns and the scan are clipped before the noise is added and again after it (the reference clips once, after the noise), which
differs only where a clean value already lay outside the clip.

The schedule is host arithmetic in Python floats, as in the reference, and needs no GPU; the kernels do (MpcLibraryError without one, no CPU fallback).
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib, toy_sim
from ._lib import cd, ci, ll, pvp, text, vp

OBSERVATIONS, ACTIONS = 0, 1
TARGETS = {"observations": OBSERVATIONS, "actions": ACTIONS}
DISTRIBUTIONS = {"gaussian": 0, "uniform": 1}
OPERATIONS = {"additive": 0, "scaling": 1}
SCHEDULES = (None, "linear", "constant")

# the entry points of csrc/mpc_domain_rand.h (bound here, not in any other module's list)
DECLS = {
    "mpc_drand_create": (ci, [pvp, ci, C.c_ulonglong]),
    "mpc_drand_destroy": (None, [vp]),
    "mpc_drand_bind": (ci, [vp, vp]),
    "mpc_drand_noise": (ci, [vp, ci, ci, ci, cd, cd, cd, cd, cd, vp, vp, vp, ci, ci, ll, vp, vp]),
    "mpc_drand_push": (ci, [vp, vp, cd, ll, vp]),
    "mpc_drand_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what bind takes) with these entry points bound
check = _lib.checker(lib, "mpc_drand_last_error")


@dataclass
class NoiseSpec:
    """One entry of ``randomization_params``: ``range`` is (mu, var) for ``gaussian`` -- the reference multiplies the draw by what it calls var -- and
    (lo, hi) for ``uniform``; ``range_correlated`` the same for the term that is drawn once and kept.  ``schedule`` None, ``"linear"`` or
    ``"constant"`` over ``schedule_steps`` ticks.  ``column_scale`` [num_obs] multiplies the noise term per column (legged_gym's ``noise_scale_vec``)."""
    distribution: str
    operation: str
    range: tuple
    range_correlated: tuple = (0.0, 0.0)
    schedule: str = None
    schedule_steps: int = 0
    column_scale: object = None

    def validate(self, what="noise", width=None):
        if self.distribution not in DISTRIBUTIONS:
            raise ValueError(f"{what}: distribution {self.distribution!r}: 'gaussian' or 'uniform'")
        if self.operation not in OPERATIONS:
            raise ValueError(f"{what}: operation {self.operation!r}: 'additive' or 'scaling'")
        for name, rng in (("range", self.range), ("range_correlated", self.range_correlated)):
            if len(rng) != 2 or not all(math.isfinite(float(v)) for v in rng):
                raise ValueError(f"{what}: {name} must be two finite numbers")
        if self.schedule not in SCHEDULES:
            raise ValueError(f"{what}: schedule {self.schedule!r}: None, 'linear' or 'constant'")
        if self.schedule is not None and not self.schedule_steps > 0:
            raise ValueError(f"{what}: schedule_steps must be > 0 when a schedule is named")
        if self.column_scale is not None:
            cs = np.asarray(self.column_scale, dtype=np.float64).reshape(-1)
            if not np.isfinite(cs).all():
                raise ValueError(f"{what}: column_scale must be finite")
            if width is not None and len(cs) != width:
                raise ValueError(f"{what}: column_scale has {len(cs)} entries, the rows {width} columns")

    def scheduled(self, last_step):
        """The reference's parameters after ``last_step`` ticks (vec_task.py:533-561, :579-588), in its names and as the Python numbers it
        computes: ``mu, var, mu_corr, var_corr`` or ``lo, hi, lo_corr, hi_corr``."""
        sched_step = self.schedule_steps
        if self.schedule == "linear":
            sched_scaling = 1.0 / sched_step * min(last_step, sched_step)
        elif self.schedule == "constant":
            sched_scaling = 0 if last_step < sched_step else 1
        else:
            sched_scaling = 1
        a, b = self.range
        a_corr, b_corr = self.range_correlated
        if self.distribution == "gaussian":
            if self.operation == "additive":
                a, b, a_corr, b_corr = a * sched_scaling, b * sched_scaling, a_corr * sched_scaling, b_corr * sched_scaling
            else:                          # the spread grows over time, the mean is interpolated from 1
                b = b * sched_scaling
                a = a * sched_scaling + 1.0 * (1.0 - sched_scaling)
                b_corr = b_corr * sched_scaling
                a_corr = a_corr * sched_scaling + 1.0 * (1.0 - sched_scaling)
            return {"mu": a, "var": b, "mu_corr": a_corr, "var_corr": b_corr}
        if self.operation == "additive":
            a, b, a_corr, b_corr = a * sched_scaling, b * sched_scaling, a_corr * sched_scaling, b_corr * sched_scaling
        else:
            a, b, a_corr, b_corr = (v * sched_scaling + 1.0 * (1.0 - sched_scaling) for v in (a, b, a_corr, b_corr))
        return {"lo": a, "hi": b, "lo_corr": a_corr, "hi_corr": b_corr}

    @staticmethod
    def kernel_params(params):
        """(m, s, m_corr, s_corr) of csrc/domain_rand.h from ``scheduled``'s dictionary; the differences are taken in Python floats (:596-597)."""
        if "mu" in params:
            return params["mu"], params["var"], params["mu_corr"], params["var_corr"]
        return params["lo"], params["hi"] - params["lo"], params["lo_corr"], params["hi_corr"] - params["lo_corr"]

    @classmethod
    def legged_gym(cls, task_cfg=None, noise_level=1.0, height_scan=None):
        """legged_gym's ``_get_noise_scale_vec`` by its published formula on this task's columns (csrc/rl_task.h): ``(2 * rand - 1) * vec`` is
        uniform, additive, range (-1, 1), and the column scales are its ``noise_scales`` (lin_vel 0.1, ang_vel 0.2, dof_pos 0.01, dof_vel 1.5,
        height_measurements 0.1) times ``noise_level`` times the observation scale of the column; the base position, the commands, the previous
        actions and the pad get none."""
        from .rl_task import NUM_OBS, TaskConfig
        cfg = task_cfg if task_cfg is not None else TaskConfig()
        width = NUM_OBS if height_scan is None else height_scan.width(NUM_OBS)
        vec = np.zeros(width, np.float64)
        vec[3:6] = 0.1 * noise_level * cfg.lin_vel_scale
        vec[6:9] = 0.2 * noise_level * cfg.ang_vel_scale
        vec[12:24] = 0.01 * noise_level * cfg.dof_pos_scale
        vec[24:36] = 1.5 * noise_level * cfg.dof_vel_scale
        if height_scan is not None:
            vec[NUM_OBS:NUM_OBS + height_scan.num_points] = 0.1 * noise_level * height_scan.scale
        return cls("uniform", "additive", (-1.0, 1.0), column_scale=vec)


@dataclass
class PushSpec:
    """legged_gym's ``domain_rand.push_robots``: every ``interval_s`` seconds the base's world x, y velocity is set to a uniform draw in
    [-``max_vel_xy``, ``max_vel_xy``]."""
    interval_s: float = 15.0
    max_vel_xy: float = 1.0

    def interval(self, dt):
        """``np.ceil(push_interval_s / dt)`` ticks."""
        return int(math.ceil(float(self.interval_s) / float(dt)))

    def validate(self, dt=None):
        if not (math.isfinite(float(self.interval_s)) and math.isfinite(float(self.max_vel_xy)) and self.max_vel_xy >= 0):
            raise ValueError("push: interval_s must be finite, max_vel_xy finite and >= 0")
        if dt is not None and not self.interval(dt) >= 1:
            raise ValueError(f"push: the interval must be at least 1 tick (interval_s {self.interval_s}, dt {dt})")


class DomainRand:
    """The randomisation of ``n`` environments: ``observations`` / ``actions`` a ``NoiseSpec`` or None, ``push`` a ``PushSpec`` or None,
    ``frequency`` the reference's (the scheduled parameters are recomputed on the first step and then whenever that many ticks have passed).
    ``enabled`` is a plain attribute: False leaves every launch out.  ``params`` holds the current parameters in the reference's names."""

    def __init__(self, n, observations=None, actions=None, push=None, frequency=1, seed=0, device=None):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("n must be at least 1")
        self.specs = {"observations": observations, "actions": actions}
        self.push = push
        self.frequency = frequency
        self.seed = int(seed) & (2 ** 64 - 1)
        self.enabled = True
        self.validate()
        self.device = device
        self.params = {}
        self.first_randomization, self.last_step, self.last_rand_step = True, 0, 0
        self.common_step_counter = self.tick = 0
        self.launches = {"observations": 0, "actions": 0, "push": 0}
        self.push_interval = None
        self._handle, self._scales, self.sim = None, {}, None

    __del__ = _lib.finalizer("mpc_drand_destroy")

    @classmethod
    def from_dr_params(cls, n, dr_params, seed=0, push=None, device=None):
        """From IsaacGymEnvs' ``task.randomization_params``: the keys ``frequency``, ``observations`` and ``actions``.  What the toy plant cannot
        randomise (``sim_params``, ``actor_params``, anything else) raises ValueError."""
        specs = {}
        for key, v in dr_params.items():
            if key == "frequency":
                continue
            if key not in TARGETS:
                raise ValueError(f"randomization_params[{key!r}]: the toy plant cannot randomise {key}; only 'frequency', 'observations' and 'actions' are taken")
            unknown = set(v) - {"distribution", "operation", "range", "range_correlated", "schedule", "schedule_steps"}
            if unknown:
                raise ValueError(f"randomization_params[{key!r}]: unknown keys {sorted(unknown)}")
            sched = v.get("schedule")
            specs[key] = NoiseSpec(v["distribution"], v["operation"], tuple(v["range"]), tuple(v.get("range_correlated", [0., 0.])), sched,
                                   v["schedule_steps"] if sched is not None else 0)
        return cls(n, specs.get("observations"), specs.get("actions"), push=push, frequency=dr_params.get("frequency", 1), seed=seed, device=device)

    # ---- host: validation and the schedule -------------------------------------------------------------------------------------------------
    def validate(self, n=None, num_obs=None, dt=None):
        """Everything that can be refused without the device; the task calls it with its batch size, its row width and its tick."""
        if n is not None and int(n) != self.n:
            raise ValueError(f"the domain randomisation holds {self.n} environments, the task {int(n)}")
        if not (isinstance(self.frequency, (int, float)) and math.isfinite(self.frequency)):
            raise ValueError("frequency must be a finite number")
        for key, spec in self.specs.items():
            if spec is not None:
                spec.validate(key, width=(num_obs if key == "observations" else 12) if num_obs is not None else None)
        if self.push is not None:
            self.push.validate(dt)

    def update_schedule(self, last_step):
        """The head of ``apply_randomizations`` (:507-519) for the two noise entries: recompute on the first call, afterwards whenever
        ``last_step - last_rand_step >= frequency``.  Returns ``params``."""
        self.last_step = last_step
        if self.first_randomization:
            do_randomize = True
        else:
            do_randomize = (self.last_step - self.last_rand_step) >= self.frequency
        if do_randomize:
            self.last_rand_step = self.last_step
            for key, spec in self.specs.items():
                if spec is not None:
                    self.params[key] = spec.scheduled(self.last_step)
        self.first_randomization = False
        return self.params

    # ---- device ---------------------------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._handle is None:
            import torch
            _lib.need_gpu("DomainRand")
            self.device = _lib.device_of(self.device)
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                check(lib().mpc_drand_create(C.byref(h), self.n, self.seed), "mpc_drand_create")
            self._handle = h
        return self._handle

    def bind(self, sim, dt=None):
        """Keep the device addresses of ``sim``'s state (a ``BatchedToySim`` with ``n`` robots) for the pushes; ``dt`` fixes the push interval."""
        check(lib().mpc_drand_bind(self._ensure(), sim._handle), "mpc_drand_bind")
        self.sim = sim
        if dt is not None and self.push is not None:
            self.push_interval = self.push.interval(dt)

    def _scale(self, key, width):
        spec = self.specs[key]
        if spec.column_scale is None:
            return None
        t = self._scales.get(key)
        if t is None or t.numel() != width:
            import torch
            cs = np.ascontiguousarray(np.asarray(spec.column_scale, dtype=np.float64).reshape(-1), dtype=np.float32)
            if len(cs) != width:
                raise ValueError(f"{key}: column_scale has {len(cs)} entries, the rows {width} columns")
            t = self._scales[key] = torch.from_numpy(cs).to(self.device)
        return t

    def noise(self, key, x, out=None, active=None, clip=math.inf, tick=0, params=None, draws=None):
        """One launch: ``x`` [n, W] (contiguous cuda float32, W even) -> ``out`` (``x`` itself when None: in place) with ``key``'s noise
        (``"observations"`` or ``"actions"``) on the columns below ``active`` (W when None) and the clamp to +-``clip``.  ``params`` is a dictionary
        of ``NoiseSpec.scheduled`` (the current schedule's when None); ``draws`` [n, active, 2] receives (d, zc).  Stream-ordered."""
        import torch
        h = self._ensure()
        spec = self.specs[key]
        if spec is None:
            raise ValueError(f"no {key} noise was configured")
        if x.dim() != 2 or x.shape[0] != self.n:
            raise ValueError(f"x: [{self.n}, W] expected")
        W = int(x.shape[1])
        _lib.tensor_arg(x, torch.float32, self.n * W, "x")
        out = x if out is None else _lib.tensor_arg(out, torch.float32, self.n * W, "out")
        active = W if active is None else int(active)
        if draws is not None:
            _lib.tensor_arg(draws, torch.float32, self.n * active * 2, "draws")
        if params is None:
            params = self.params[key] if key in self.params else self.update_schedule(self.last_step)[key]
        m, s, m_corr, s_corr = self.kernel_params(params)
        cs = self._scale(key, W)
        check(lib().mpc_drand_noise(h, TARGETS[key], DISTRIBUTIONS[spec.distribution], OPERATIONS[spec.operation], m, s, m_corr, s_corr, float(clip),
                                    None if cs is None else cs.data_ptr(), x.data_ptr(), out.data_ptr(), W, active, int(tick),
                                    None if draws is None else draws.data_ptr(), _lib.stream(self.device)), "mpc_drand_noise")
        self.launches[key] += 1
        return out

    kernel_params = staticmethod(NoiseSpec.kernel_params)

    def push_robots(self, root_states, push_index, max_vel=None):
        """One launch: every robot of the bound sim that has not fallen gets a world x, y velocity uniform in [-max_vel, max_vel], in the sim's
        state and in ``root_states`` [n, 13].  Stream-ordered."""
        import torch
        _lib.tensor_arg(root_states, torch.float32, self.n * 13, "root_states")
        v = self.push.max_vel_xy if max_vel is None else max_vel
        check(lib().mpc_drand_push(self._ensure(), root_states.data_ptr(), float(v), int(push_index), _lib.stream(self.device)), "mpc_drand_push")
        self.launches["push"] += 1

    # ---- the three places of BatchedRLTask.step ------------------------------------------------------------------------------------------------
    def begin_step(self):
        """Once per step, at its head: the schedule after ``common_step_counter`` completed ticks, and ``tick``, the key of this step's draws."""
        self.tick = self.common_step_counter
        self.update_schedule(self.common_step_counter)

    def after_physics(self, root_states):
        """legged_gym's ``_post_physics_step_callback``: count the tick, and push when the counter is a multiple of the interval."""
        self.common_step_counter += 1
        if self.push is not None and self.common_step_counter % self.push_interval == 0:
            self.push_robots(root_states, self.common_step_counter // self.push_interval)
