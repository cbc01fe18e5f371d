"""Episode statistics on the device (include/mpc_episode.h, csrc/mpc_episode.hip, csrc/episode_stats.h).

rsl_rl's ``OnPolicyRunner.learn`` keeps, per tick and on the host, ``cur_reward_sum += rewards``, ``cur_episode_length += 1`` and, for
``dones.nonzero()``, an extend of two ``deque(maxlen=100)`` -- a host round trip on every tick.  ``EpisodeStats`` keeps the same on the device:

    stats = EpisodeStats(env.num_envs, window=100, groups=robot_type, num_groups=3)
    obs, rew, reset, extras = env.step(actions)
    stats.add(rew, reset, extras["time_outs"])          # stream-ordered: nothing is copied to the host, nothing waits for the device
    stats.read()                                         # the one place that goes to the host

``add`` takes any ``(rew, reset, time_outs)``: float32 rewards and int64 flags (finished: ``reset > 0``; timed out: finished and
``time_outs > 0``), contiguous cuda tensors of ``n`` elements.  The window is ``deque(maxlen=window)`` extended in (tick, environment) order;
totals (episodes, timed out, float64 sum of returns, int64 sum of lengths) are kept overall and per group.  ``summary`` is one float64 device tensor
(layout: ``S_*`` below); a caller that reads other device values anyway concatenates it into that read.

The entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ci, ll, need_gpu, pvp, tensor_arg, text, vp

# the entry points of include/mpc_episode.h (bound here, not in _lib.SYMBOLS or ppo.SYMBOLS)
DECLS = {
    "mpc_episode_create": (ci, [pvp, ci, ci, ci]),
    "mpc_episode_destroy": (None, [vp]),
    "mpc_episode_bind": (ci, [vp, vp]),
    "mpc_episode_add": (ci, [vp, vp, vp, vp, vp]),
    "mpc_episode_summary": (ci, [vp, vp]),
    "mpc_episode_restart": (ci, [vp, vp]),
    "mpc_episode_clear": (ci, [vp, vp]),
    "mpc_episode_random_progress": (ci, [vp, ci, ll, C.c_ulonglong, vp]),
    "mpc_episode_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS)             # libmpc_batch.so with the episode entry points bound
check = _lib.checker(lib, "mpc_episode_last_error")

MAX_GROUPS = 64
# counters [COUNTERS + COUNTER_STRIDE * (1 + G)] int64: head, the window's count, then per block (0 overall, 1 + g group g) episodes, timed out, sum of lengths
HEAD, COUNT, COUNTERS, COUNTER_STRIDE = 0, 1, 2, 3
C_EPISODES, C_TIMEOUTS, C_SUM_LENGTH = 0, 1, 2
# summary [S_TOTALS + S_STRIDE * (1 + G)] float64: the window's count, mean return, mean length, timed-out count, then per block episodes, timed out, sum of
# returns, sum of lengths
S_WINDOW_COUNT, S_MEAN_RETURN, S_MEAN_LENGTH, S_WINDOW_TIMEOUTS, S_TOTALS, S_STRIDE = 0, 1, 2, 3, 4, 4
T_EPISODES, T_TIMEOUTS, T_SUM_RETURN, T_SUM_LENGTH = 0, 1, 2, 3
S_EPISODES = S_TOTALS + T_EPISODES                   # the overall count of finished episodes


class _Buffers(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("cur_return", "cur_length", "win_return", "win_length", "win_timed_out", "counters", "sums", "summary", "groups")]


def random_progress(progress, max_len, seed):
    """rsl_rl's ``init_at_random_ep_len``: ``progress`` (contiguous cuda int64, e.g. ``BatchedRLTask.progress_buf``) <- integers uniform on
    [0, max_len), element i a function of (seed, i) alone.  Stream-ordered."""
    need_gpu("random_progress", progress)
    tensor_arg(progress, torch.long, progress.numel(), "progress")
    with torch.cuda.device(progress.device):
        check(lib().mpc_episode_random_progress(progress.data_ptr(), progress.numel(), int(max_len), int(seed) & (2 ** 64 - 1), _lib.stream(progress.device)),
              "mpc_episode_random_progress")
    return progress


class EpisodeStats:
    """The window of the last ``window`` finished episodes and the running totals of ``n`` environments, on the device.

    ``groups``: an integer per environment (a robot type, a terrain level) in [0, num_groups); an id outside counts in the overall totals only.
    Public device tensors: ``cur_return`` [n] float32, ``cur_length`` [n] int32 (the episodes in flight), ``win_return`` / ``win_length`` /
    ``win_timed_out`` [window] (the ring), ``counters`` int64 and ``sums`` float64 (the totals), and ``summary``.  ``guard`` (for tests) puts
    that many spare elements on either side of every one of them."""

    def __init__(self, n, window=100, groups=None, num_groups=1, device=None, guard=0):
        need_gpu("EpisodeStats")
        self.n, self.window, self.num_groups = int(n), int(window), int(num_groups)
        self.device = _lib.device_of(device)
        self._handle = C.c_void_p()
        check(lib().mpc_episode_create(C.byref(self._handle), self.n, self.window, self.num_groups), "mpc_episode_create")
        blocks, g = 1 + self.num_groups, int(guard)
        self._raw = {}

        def z(name, numel, dtype):
            self._raw[name] = torch.zeros(numel + 2 * g, dtype=dtype, device=self.device)
            return self._raw[name][g:g + numel]
        self.cur_return, self.cur_length = z("cur_return", self.n, torch.float32), z("cur_length", self.n, torch.int32)
        self.win_return, self.win_length = z("win_return", self.window, torch.float32), z("win_length", self.window, torch.int32)
        self.win_timed_out = z("win_timed_out", self.window, torch.int32)
        self.counters, self.sums = z("counters", COUNTERS + COUNTER_STRIDE * blocks, torch.long), z("sums", blocks, torch.float64)
        self._summary = z("summary", S_TOTALS + S_STRIDE * blocks, torch.float64)
        self.groups = None
        if groups is not None:
            self.groups = torch.as_tensor(groups).to(self.device, torch.int32).contiguous()
            if self.groups.numel() != self.n:
                raise ValueError(f"groups: one id per environment ({self.n}) expected")
        b = _Buffers(*(t.data_ptr() for t in (self.cur_return, self.cur_length, self.win_return, self.win_length, self.win_timed_out, self.counters,
                                              self.sums, self._summary)), self.groups.data_ptr() if self.groups is not None else None)
        with torch.cuda.device(self.device):
            check(lib().mpc_episode_bind(self._handle, C.addressof(b)), "mpc_episode_bind")

    __del__ = _lib.finalizer("mpc_episode_destroy")

    def add(self, rew, reset, time_outs):
        """One tick, in rsl_rl's order: accumulate, then every finished environment in ascending index appends (return, length, timed out) to the
        window, adds it to the totals and zeroes its accumulators.  Reads the task's buffers as they are; stream-ordered, no host synchronisation."""
        need_gpu("EpisodeStats.add", rew, reset, time_outs)
        tensor_arg(rew, torch.float32, self.n, "rew"); tensor_arg(reset, torch.long, self.n, "reset"); tensor_arg(time_outs, torch.long, self.n, "time_outs")
        check(lib().mpc_episode_add(self._handle, rew.data_ptr(), reset.data_ptr(), time_outs.data_ptr(), _lib.stream(self.device)), "mpc_episode_add")

    def restart(self):
        """Zeroes the in-flight accumulators: the episodes under way are dropped, the window and the totals stay."""
        check(lib().mpc_episode_restart(self._handle, _lib.stream(self.device)), "mpc_episode_restart")

    def clear(self):
        """Zeroes everything."""
        check(lib().mpc_episode_clear(self._handle, _lib.stream(self.device)), "mpc_episode_clear")

    @property
    def summary(self):
        """The float64 device tensor of the ``S_*`` layout.  LAUNCHES ON ACCESS: every read of this attribute enqueues one stream-ordered kernel that
        brings the tensor up to date (the means are float64 sums over the window's slots divided by the count, 0.0 for an empty window) and returns
        the SAME tensor, which the next access rewrites: ``clone()`` a value that has to outlive it.  No host synchronisation.  The summary is not
        refreshed per tick because the means need the window after the tick's last launch; the trainer asks once per iteration."""
        check(lib().mpc_episode_summary(self._handle, _lib.stream(self.device)), "mpc_episode_summary")
        return self._summary

    @staticmethod
    def _block(s, k):
        o = S_TOTALS + S_STRIDE * k
        episodes, timeouts = int(s[o + T_EPISODES]), int(s[o + T_TIMEOUTS])
        return dict(episodes=episodes, time_outs=timeouts, terminations=episodes - timeouts, sum_return=s[o + T_SUM_RETURN], sum_length=int(s[o + T_SUM_LENGTH]),
                    mean_return=s[o + T_SUM_RETURN] / episodes if episodes else 0.0, mean_length=s[o + T_SUM_LENGTH] / episodes if episodes else 0.0)

    def read(self):
        """The summary as a dict -- the one place in this class that goes to the host (one copy, which waits for the stream): the window's
        ``episodes_in_window``, ``mean_episode_return``, ``mean_episode_length``, ``timeouts_in_window``; the overall totals (``episodes``,
        ``time_outs``, ``terminations``, ``sum_return``, ``sum_length``, ``mean_return``, ``mean_length``) and the same per group under ``groups``."""
        s = self.summary.tolist()
        out = dict(episodes_in_window=int(s[S_WINDOW_COUNT]), mean_episode_return=s[S_MEAN_RETURN], mean_episode_length=s[S_MEAN_LENGTH],
                   timeouts_in_window=int(s[S_WINDOW_TIMEOUTS]))
        out.update(self._block(s, 0))
        out["groups"] = [self._block(s, 1 + g) for g in range(self.num_groups)]
        return out
