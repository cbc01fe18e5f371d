"""The model of the episode statistics (rl_mpc_locomotion_amd.episode, csrc/episode_stats.h): rsl_rl v1.0.2's lines of OnPolicyRunner.learn in torch
float32 on the CPU with ``collections.deque(maxlen=cap)``, plus exact totals (``math.fsum``, Python ints) overall and per group; the cases the CPU and the
GPU tests share; and the comparison of one implementation's state with the model after a tick.

Bounds.  Accumulators, window entries, counts and integer totals are chains of exactly rounded float32 adds and integers: ``==``.  A float64 sum of k
terms taken in ANY order is within (k - 1) u sum|x| (1 + O(k u)), u = 2^-53, of the exact sum; the tests allow k 2^-52 sum|x| (and that divided by the
count for a mean, which also covers the division's own rounding)."""
import math
from collections import deque

import numpy as np
import torch

NS = (1, 63, 64, 65, 1025, 2113)
CAPS = (1, 3, 100)
GROUPS = (1, 3, 8)
TICKS = 40
# the layouts of include/mpc_episode.h
HEAD, COUNT, COUNTERS, COUNTER_STRIDE = 0, 1, 2, 3


class Model:
    def __init__(self, n, cap, num_groups=1, groups=None):
        self.n, self.cap, self.num_groups = n, cap, num_groups
        self.groups = None if groups is None else [int(g) for g in groups]
        self.cur_reward_sum = torch.zeros(n, dtype=torch.float32)
        self.cur_episode_length = torch.zeros(n, dtype=torch.float32)           # (rsl_rl keeps the length as a float tensor too)
        self.rewbuffer, self.lenbuffer, self.tobuffer = deque(maxlen=cap), deque(maxlen=cap), deque(maxlen=cap)
        self.blocks = [dict(episodes=0, timeouts=0, sum_length=0, returns=[]) for _ in range(1 + num_groups)]

    def add(self, rew, reset, time_outs):
        """rew float32 [n], reset and time_outs int64 [n] (cpu tensors)."""
        self.cur_reward_sum += rew
        self.cur_episode_length += 1
        new_ids = (reset > 0).nonzero(as_tuple=False)
        returns = self.cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist()
        lengths = self.cur_episode_length[new_ids][:, 0].cpu().numpy().tolist()
        timed = (time_outs[new_ids][:, 0] > 0).tolist()
        self.rewbuffer.extend(returns)
        self.lenbuffer.extend(lengths)
        self.tobuffer.extend(timed)
        self.cur_reward_sum[new_ids] = 0
        self.cur_episode_length[new_ids] = 0
        for i, r, l, t in zip(new_ids[:, 0].tolist(), returns, lengths, timed):
            g = 0 if self.groups is None else self.groups[i]
            for b in [0] + ([1 + g] if 0 <= g < self.num_groups else []):
                blk = self.blocks[b]
                blk["episodes"] += 1; blk["timeouts"] += int(t); blk["sum_length"] += int(l); blk["returns"].append(r)

    def restart(self):
        self.cur_reward_sum.zero_(); self.cur_episode_length.zero_()

    def window(self):
        """(count, exact mean return, bound on it, exact mean length, bound, timed out) of the window; 0.0 for an empty one."""
        k = len(self.rewbuffer)
        if k == 0:
            return 0, 0.0, 0.0, 0.0, 0.0, 0
        eps = k * 2.0 ** -52
        return (k, math.fsum(self.rewbuffer) / k, eps * math.fsum(abs(x) for x in self.rewbuffer) / k, math.fsum(self.lenbuffer) / k,
                eps * math.fsum(self.lenbuffer) / k, sum(self.tobuffer))


def make_case(n, cap, num_groups, seed):
    """TICKS ticks of (rew, reset, time_outs) and the group ids: none finished for 10 ticks, everyone at once, Bernoulli 0.1, only environment 0, only
    n - 1, exactly cap, cap + 1, and everyone again once the head has moved.  Flags take the values 0, 1, 2 and -1 (finished is > 0); time-outs are
    a random half of the finished plus some where nothing finished; rewards are normal x 3 with exact zeros and negative zeros; group ids run from -1
    to G inclusive."""
    g = torch.Generator().manual_seed(seed)
    groups = torch.randint(-1, num_groups + 1, (n,), generator=g, dtype=torch.int32)
    ticks = []
    for t in range(TICKS):
        rew = torch.randn(n, generator=g) * 3
        z = torch.rand(n, generator=g)
        rew[z < 0.03] = 0.0
        rew[z > 0.97] = -0.0
        done = torch.zeros(n, dtype=torch.bool)
        if t < 10:
            pass
        elif t in (10, 30):
            done[:] = True
        elif t == 21:
            done[0] = True
        elif t == 22:
            done[n - 1] = True
        elif t in (23, 24):
            done[torch.randperm(n, generator=g)[:min(n, cap + (t - 23))]] = True
        else:
            done = torch.rand(n, generator=g) < 0.1
        reset = torch.where(done, torch.randint(1, 3, (n,), generator=g), -(torch.rand(n, generator=g) < 0.05).long())
        time_outs = ((done & (torch.rand(n, generator=g) < 0.5)) | (torch.rand(n, generator=g) < 0.1)).long() * torch.randint(1, 3, (n,), generator=g)
        ticks.append((rew.contiguous(), reset.contiguous(), time_outs.contiguous()))
    return groups, ticks


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def check_state(model, st, what):
    """``st``: numpy arrays cur_return, cur_length, win_return, win_length, win_timed_out, counters (int64, the header's layout), sums (float64) of the
    implementation under test, after the tick the model has just taken."""
    assert np.array_equal(bits(st["cur_return"]), bits(model.cur_reward_sum.numpy())), f"{what}: cur_return"
    assert np.array_equal(st["cur_length"], model.cur_episode_length.numpy().astype(np.int64)), f"{what}: cur_length"
    head, count, cap = int(st["counters"][HEAD]), int(st["counters"][COUNT]), model.cap
    assert count == len(model.rewbuffer) and 0 <= head < cap, f"{what}: count {count} head {head}"
    order = np.arange(count) if count < cap else (head + np.arange(cap)) % cap
    if count < cap:
        assert head == count % cap
    assert np.array_equal(bits(st["win_return"][order]), bits(list(model.rewbuffer))), f"{what}: window returns"
    assert np.array_equal(st["win_length"][order], np.array(list(model.lenbuffer), dtype=np.int64)), f"{what}: window lengths"
    assert np.array_equal(st["win_timed_out"][order], np.array(list(model.tobuffer), dtype=np.int64)), f"{what}: window time-outs"
    for b, blk in enumerate(model.blocks):
        k = st["counters"][COUNTERS + COUNTER_STRIDE * b:COUNTERS + COUNTER_STRIDE * (b + 1)]
        assert [int(v) for v in k] == [blk["episodes"], blk["timeouts"], blk["sum_length"]], f"{what}: totals of block {b}: {k} != {blk}"
        exact, bound = math.fsum(blk["returns"]), len(blk["returns"]) * 2.0 ** -52 * math.fsum(abs(x) for x in blk["returns"])
        assert abs(float(st["sums"][b]) - exact) <= bound, f"{what}: sum of returns of block {b}: {st['sums'][b]!r} against {exact!r} +- {bound:.3e}"


def check_summary(model, s, what):
    """``s``: the float64 summary (the header's layout) against the model's exact values."""
    count, mean_r, bound_r, mean_l, bound_l, timed = model.window()
    assert np.isfinite(s).all(), f"{what}: summary not finite"
    assert s[0] == count and s[3] == timed, f"{what}: window count / time-outs {s[0]}, {s[3]} != {count}, {timed}"
    assert abs(s[1] - mean_r) <= bound_r and abs(s[2] - mean_l) <= bound_l, f"{what}: window means {s[1]!r}, {s[2]!r} against {mean_r!r}, {mean_l!r}"
    if count == 0:
        assert s[1] == 0.0 and s[2] == 0.0
    for b, blk in enumerate(model.blocks):
        o = 4 + 4 * b
        exact, bound = math.fsum(blk["returns"]), len(blk["returns"]) * 2.0 ** -52 * math.fsum(abs(x) for x in blk["returns"])
        assert [s[o], s[o + 1], s[o + 3]] == [blk["episodes"], blk["timeouts"], blk["sum_length"]] and abs(s[o + 2] - exact) <= bound, f"{what}: summary block {b}"
