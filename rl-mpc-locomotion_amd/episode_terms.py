"""Per-term episode reward sums and a command curriculum on the device (csrc/mpc_episode_terms.h, csrc/mpc_episode_terms.hip,
csrc/episode_terms.h).

legged_gym's ``episode_sums`` and ``update_command_curriculum`` and rsl_rl's per-term ``ep_infos`` restated from their published algorithms: for every
environment the running float32 sum of each of the task's six reward terms over the episode under way; when the task's ``begin`` marks an environment
its episode is closed -- the sums go into float64 window accumulators, and on the ticks the curriculum looks, the closed episodes' mean tracking sum
decides whether the x command range widens -- the sums are zeroed, and with a curriculum the environment's commands are drawn afresh from the updated
range, in the same tick and with no host round trip::

    terms = EpisodeTerms(n, cfg, command_curriculum=CommandCurriculumSpec(max_curriculum=2.5, x_range0=(-1.0, 1.0)))
    task = BatchedRLTask(robot_type, gait_id, cfg, episode_terms=terms)
    PPOTrainer(task).learn(k)            # records carry episode_terms: rew_<term>, max_command_x, min_command_x, command_widenings

``BatchedRLTask.step`` calls ``close_and_resample`` straight after ``begin`` (before the resets and ``finish``, which writes the commands into the
observations) and ``accumulate`` after ``finish``, on the tensors ``finish`` read.  Callers with a simulator of their own call the two themselves.

Not legged_gym's or rsl_rl's (csrc/episode_terms.h has the list): the mean is a float64 sum in a fixed blocked order; the record is episode-weighted
over the iteration; an episode closes at the head of the tick that performs the reset; the command draws are counter-based, uniform in distribution;
the terms are the unclipped products while the reward is clipped at 0; only the x range moves; an episode whose sums are not all finite (a plant
state that blew up) is zeroed and resampled but neither counted nor added.

The spec's validation is host arithmetic and needs no GPU; the kernels do (MpcLibraryError without one, no CPU fallback).
"""
import ctypes as C
import math
from dataclasses import dataclass

from . import _lib
from ._lib import cd, ci, ll, pvp, text, vp
from .rl_task import REWARD_TERMS, TaskConfig

NUM_TERMS = len(REWARD_TERMS)
# summary()'s layout (epterms::kSum*)
S_CLOSED, S_TERMS, S_LO, S_HI, S_WIDENINGS, S_EPISODE_S, SUMMARY_LEN = 0, 1, 1 + NUM_TERMS, 2 + NUM_TERMS, 3 + NUM_TERMS, 4 + NUM_TERMS, 5 + NUM_TERMS
# the device state's layout (epterms::kGlob*)
G_RANGES, G_WINDOW, G_WIDENINGS, STATE_LEN = 0, 6, 7 + NUM_TERMS, 8 + NUM_TERMS

# the entry points of csrc/mpc_episode_terms.h (bound here, not in any other module's list)
DECLS = {
    "mpc_episode_terms_create": (ci, [pvp, ci, vp, cd, ci, cd, cd, cd, cd, cd, ll]),
    "mpc_episode_terms_destroy": (None, [vp]),
    "mpc_episode_terms_close_and_resample": (ci, [vp, vp, vp, ll, ci, vp]),
    "mpc_episode_terms_accumulate": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "mpc_episode_terms_summary": (ci, [vp, vp, vp]),
    "mpc_episode_terms_new_window": (ci, [vp, vp]),
    "mpc_episode_terms_arrays": (ci, [vp, pvp, pvp, pvp, pvp]),
    "mpc_episode_terms_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS)               # libmpc_batch.so with these entry points bound
check = _lib.checker(lib, "mpc_episode_terms_last_error")


@dataclass
class CommandCurriculumSpec:
    """legged_gym's ``commands.curriculum``: the x range starts at ``x_range0`` (None: ``TaskConfig.command_x_range``) and widens by ``step`` on either
    side, inside +-``max_curriculum``, whenever the closed episodes' mean tracking sum per tick exceeds ``threshold`` times the term's scale, looked at
    every ``update_every`` ticks (None: ``cfg.max_episode_length``)."""
    max_curriculum: float
    x_range0: tuple = None
    step: float = 0.5
    threshold: float = 0.8
    update_every: int = None

    def resolved(self, cfg):
        """(lo0, hi0, update_every) against ``cfg``, validated: everything that can be refused without the device."""
        rng = cfg.command_x_range if self.x_range0 is None else self.x_range0
        if len(rng) != 2:
            raise ValueError("command curriculum: x_range0 must be (lo, hi)")
        lo0, hi0 = float(rng[0]), float(rng[1])
        numbers = (lo0, hi0, float(self.max_curriculum), float(self.step), float(self.threshold))
        if not all(math.isfinite(v) for v in numbers):
            raise ValueError("command curriculum: x_range0, max_curriculum, step and threshold must be finite")
        if not lo0 <= 0.0 <= hi0:
            raise ValueError(f"command curriculum: the initial x range must satisfy lo <= 0 <= hi, got ({lo0}, {hi0})")
        if not self.max_curriculum >= max(abs(lo0), abs(hi0)):
            raise ValueError(f"command curriculum: max_curriculum {self.max_curriculum} lies inside the initial x range ({lo0}, {hi0})")
        if not self.step > 0:
            raise ValueError("command curriculum: step must be > 0")
        every = cfg.max_episode_length if self.update_every is None else self.update_every
        if int(every) != every or every < 1:
            raise ValueError("command curriculum: update_every must be a whole number of ticks, at least 1")
        return lo0, hi0, int(every)


class EpisodeTerms:
    """The sums of ``n`` environments under ``cfg`` (a ``TaskConfig``; the task's own).  Cuda tensor views over the handle's memory, valid while the
    object lives: ``sums`` [n, 6] float32 (``REWARD_TERMS`` order), ``ticks`` [n] int32 (the ticks held in the sums), ``counts`` [n] int32 (resamples
    seen), ``ranges`` [3, 2] float64 (the x, y and yaw command ranges as they stand).  ``curriculum_enabled`` is a plain attribute: False skips the
    decision (an evaluation run) while episodes are still closed and commands still drawn from the ranges as they are.  ``terms_buf`` (None, or a
    [n, 6] float32 cuda tensor the caller sets) receives every tick's six terms when ``accumulate`` is given no ``terms`` of its own."""

    def __init__(self, n, cfg=None, command_curriculum=None, device=None):
        import torch
        self.n = int(n)
        if self.n < 1:
            raise ValueError("n must be at least 1")
        self.cfg = cfg if cfg is not None else TaskConfig()
        self.command_curriculum = command_curriculum
        lo0, hi0, every = command_curriculum.resolved(self.cfg) if command_curriculum is not None else (0.0, 0.0, 1)
        self.update_every = every
        _lib.need_gpu("EpisodeTerms")
        self.device = _lib.device_of(device)
        self.curriculum_enabled = True
        self.tick = 0                      # the last tick close_and_resample was given
        self.terms_buf = None
        self.max_episode_length_s = float(self.cfg.episode_length_s)
        cs, k = self.cfg._struct(), command_curriculum
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().mpc_episode_terms_create(C.byref(self._handle), self.n, C.addressof(cs), self.max_episode_length_s, 0 if k is None else 1, lo0, hi0,
                                                 0.0 if k is None else float(k.step), 0.0 if k is None else float(k.threshold),
                                                 0.0 if k is None else float(k.max_curriculum), every), "mpc_episode_terms_create")
        p = [C.c_void_p() for _ in range(4)]
        check(lib().mpc_episode_terms_arrays(self._handle, *(C.byref(x) for x in p)), "mpc_episode_terms_arrays")
        self.sums = _lib.device_view(p[0].value, (self.n, NUM_TERMS), "<f4", self.device)
        self.ticks = _lib.device_view(p[1].value, (self.n,), "<i4", self.device)
        self.counts = _lib.device_view(p[2].value, (self.n,), "<i4", self.device)
        self.state = _lib.device_view(p[3].value, (STATE_LEN,), "<f8", self.device)      # ranges, window accumulators, widenings
        self.ranges = self.state[G_RANGES:G_RANGES + 6].view(3, 2)
        self._summary = torch.zeros((SUMMARY_LEN,), dtype=torch.float64, device=self.device)

    __del__ = _lib.finalizer("mpc_episode_terms_destroy")

    def close_and_resample(self, reset_ids, commands, tick):
        """Straight after the task's ``begin``: ``reset_ids`` [n] int32 (r where environment r is being reset, -1 elsewhere), ``commands`` [n, 3]
        float32 (rewritten for the marked environments, with a command curriculum only), ``tick`` the caller's count of ticks.  Stream-ordered, no
        host synchronisation."""
        import torch
        _lib.tensor_arg(reset_ids, torch.int32, self.n, "reset_ids")
        _lib.tensor_arg(commands, torch.float32, self.n * 3, "commands")
        check(lib().mpc_episode_terms_close_and_resample(self._handle, reset_ids.data_ptr(), commands.data_ptr(), int(tick),
                                                         1 if self.curriculum_enabled else 0, _lib.stream(self.device)),
              "mpc_episode_terms_close_and_resample")
        self.tick = int(tick)

    def accumulate(self, root_states, commands, torques, fell, terms=None):
        """After the task's ``finish``, on what it read: root_states [n, 13], commands [n, 3], torques [n, 12] float32, ``fell`` [n] bool / uint8 or
        None.  ``terms`` [n, 6] float32 (default: ``terms_buf``) receives the tick's six terms.  Stream-ordered."""
        import torch
        n = self.n
        terms = self.terms_buf if terms is None else terms
        for name, t, numel in (("root_states", root_states, n * 13), ("commands", commands, n * 3), ("torques", torques, n * 12)):
            _lib.tensor_arg(t, torch.float32, numel, name)
        if terms is not None:
            _lib.tensor_arg(terms, torch.float32, n * NUM_TERMS, "terms")
        fell_ptr = None if fell is None else _lib.flag_arg(fell, n, "fell").data_ptr()
        check(lib().mpc_episode_terms_accumulate(self._handle, root_states.data_ptr(), commands.data_ptr(), torques.data_ptr(), fell_ptr,
                                                 None if terms is None else terms.data_ptr(), _lib.stream(self.device)), "mpc_episode_terms_accumulate")

    def summary(self):
        """float64 [11] on the device (the same tensor on every call): the episodes closed since the last ``new_window``, the six sums of their
        terms, x lo, x hi, the widenings, ``max_episode_length_s``.  Stream-ordered."""
        check(lib().mpc_episode_terms_summary(self._handle, self._summary.data_ptr(), _lib.stream(self.device)), "mpc_episode_terms_summary")
        return self._summary

    def new_window(self):
        """Zero the window accumulators.  Stream-ordered."""
        check(lib().mpc_episode_terms_new_window(self._handle, _lib.stream(self.device)), "mpc_episode_terms_new_window")

    @staticmethod
    def record(values):
        """``summary().tolist()`` as the ``episode_terms`` entry of a training record: ``rew_<term>`` is the window's term sum per closed episode and
        per second of a full episode (0.0 when nothing closed), legged_gym's ``extras["episode"]`` entries averaged over the closed episodes."""
        closed, seconds = values[S_CLOSED], values[S_EPISODE_S]
        out = {"rew_" + name: (values[S_TERMS + i] / closed / seconds if closed > 0 else 0.0) for i, name in enumerate(REWARD_TERMS)}
        out.update(max_command_x=values[S_HI], min_command_x=values[S_LO], command_widenings=int(values[S_WIDENINGS]))
        return out

    def state_dict(self):
        """The x range, the widenings and the tick (one host read)."""
        lo, hi, w = self.state[[G_RANGES, G_RANGES + 1, G_WIDENINGS]].tolist()
        return {"command_x_range": (lo, hi), "command_widenings": int(w), "tick": self.tick}

    def load_state_dict(self, sd):
        import torch
        lo, hi = (float(v) for v in sd["command_x_range"])
        if not lo <= hi:
            raise ValueError("command_x_range: lo <= hi")
        self.state[G_RANGES:G_RANGES + 2].copy_(torch.tensor([lo, hi], dtype=torch.float64))
        self.state[G_WIDENINGS:G_WIDENINGS + 1].copy_(torch.tensor([float(sd["command_widenings"])], dtype=torch.float64))
        self.tick = int(sd["tick"])
