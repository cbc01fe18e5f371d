"""The stage timer of tools/_rate.py on a stub task and a stub event class (no device), and the names of BatchedRLTask.step's stages."""
import os
import sys

import numpy as np

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import rl_task as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _rate  # noqa: E402

NAMES = ("actions", "controller", "plant", "push", "terrain_curriculum", "begin", "episode_close", "resets", "finish", "episode_accumulate", "height_scan",
         "privileged_obs", "observation_noise")


def test_the_stage_names():
    assert isinstance(R.STAGES, tuple) and R.STAGES == NAMES and len(set(R.STAGES)) == 13


class _Clock:
    """Stub events on one clock: the k-th event recorded reads 2 ** k ms, so every span between two events is a different number that names both."""

    def __init__(self):
        self.recorded, self.synchronised = [], 0
        clock = self

        class Event:
            def __init__(self):
                self.at = None

            def record(self):
                assert self.at is None                                     # every event is recorded once
                self.at = len(clock.recorded)
                clock.recorded.append(self)

            def elapsed_time(self, other):
                assert clock.synchronised == 1                             # spans are read after the one synchronise
                return float(2 ** other.at - 2 ** self.at)
        self.Event = Event

    def synchronize(self):
        self.synchronised += 1


class _Task:
    """``step`` marks the stages of ``ticks[k]`` on its k-th call."""

    def __init__(self, ticks, clock):
        self.ticks, self.clock, self.calls, self.seen = ticks, clock, 0, []

    def step(self, actions, mark=None):
        self.seen.append(actions)
        before = len(self.clock.recorded)
        for stage in self.ticks[self.calls]:
            mark(stage)
        assert len(self.clock.recorded) == before + len(self.ticks[self.calls])      # one event a mark, recorded inside it
        self.calls += 1


def _run(ticks):
    clock = _Clock()
    task = _Task(ticks, clock)
    actions = object()
    got = _rate.stage_times(task, actions, len(ticks) // 2, event=clock.Event, synchronize=clock.synchronize)
    assert task.calls == len(ticks) and all(a is actions for a in task.seen) and clock.synchronised == 1
    assert len(clock.recorded) == len(ticks) + sum(len(t) for t in ticks)            # one event before each step, one at each mark
    return got


def _want(ticks):
    """Every event in order -- one before each step, one for each mark -- and a stage's span from the event before it to its own."""
    want, k = {}, 0
    for tick in ticks:
        k += 1                                                                       # the event before the step
        for stage in tick:
            want.setdefault(stage, []).append(float(2 ** k - 2 ** (k - 1)))
            k += 1
    return want


def test_stage_timer_returns_each_stages_spans():
    ticks = [("actions", "controller", "plant", "begin", "resets", "finish")] * 4
    got = _run(ticks)
    want = _want(ticks)
    assert list(got) == list(ticks[0])
    for stage, ms in got.items():
        assert isinstance(ms, np.ndarray) and ms.shape == (4,) and ms.tolist() == want[stage]
    assert got["actions"].tolist() == [1.0, 2.0 ** 7, 2.0 ** 14, 2.0 ** 21]           # the span from the event before the step
    assert got["controller"][0] == 2.0 and got["finish"][0] == 32.0


def test_stage_timer_tolerates_a_stage_that_some_ticks_leave_out():
    base = ("actions", "controller", "plant", "push", "begin", "resets", "finish")
    ticks = [base, tuple(s for s in base if s != "push"), base + ("observation_noise",), tuple(s for s in base if s != "push"), base, base]
    got = _run(ticks)
    want = _want(ticks)
    assert set(got) == set(base) | {"observation_noise"}
    for stage, ms in got.items():
        assert ms.tolist() == want[stage], stage
    assert len(got["push"]) == 4 and len(got["observation_noise"]) == 1 and len(got["begin"]) == 6
    # on a tick without the push, begin's span starts at the plant's event, not at an event of another tick
    k = 1 + len(base) + 1 + 3                                                        # the second tick's begin: after its before-event and three marks
    assert got["begin"][1] == float(2 ** k - 2 ** (k - 1))
