"""The episode statistics on the CPU (csrc/episode_stats.h, include/mpc_episode.h, rl_mpc_locomotion_amd.episode): the header is compiled with g++ into a
small shim and driven tick by tick against the model of tests/episode_ref.py (whose text gives the bounds); the ABI's symbols and argument checks; the
random episode lengths (every bucket count inside five standard deviations, the project's rule for its samplers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, episode as E, ppo as P, rl_task, terrain, toy_sim
from tests import episode_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mpc_episode.h")
HIPCC = "/opt/rocm/bin/hipcc"

SHIM = r"""
#include <vector>
#include "episode_stats.h"
using namespace episode;
extern "C" {
// counters and sums in the layout of include/mpc_episode.h
void shim_tick(int n, int cap, int G, float *cur_return, int *cur_length, float *win_return, int *win_length, int *win_timed_out, long long *counters,
               double *sums, const int *groups, const float *rew, const long long *reset, const long long *time_outs) {
  std::vector<Totals> totals(1 + G);
  for (int b = 0; b <= G; ++b) totals[b] = Totals{counters[2 + 3 * b], counters[3 + 3 * b], counters[4 + 3 * b], sums[b]};
  State s{n, cap, G, cur_return, cur_length, win_return, win_length, win_timed_out, counters[0], counters[1], totals.data(), groups};
  tick(s, rew, reset, time_outs);
  counters[0] = s.head; counters[1] = s.count;
  for (int b = 0; b <= G; ++b) {
    counters[2 + 3 * b] = totals[b].episodes; counters[3 + 3 * b] = totals[b].timeouts; counters[4 + 3 * b] = totals[b].sum_length;
    sums[b] = totals[b].sum_return;
  }
}
void shim_random_progress(unsigned long long seed, int env0, int n, long long max_len, long long *out) {
  for (int i = 0; i < n; ++i) out[i] = random_progress(seed, (uint32_t)(env0 + i), max_len);
}
long long shim_slot_of(long long head, long long rank, long long total, long long cap) { return slot_of(head, rank, total, cap); }
}
"""


def build_shim(d):
    src, so = d / "episode_shim.cpp", d / "episode_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    L.shim_tick.argtypes = [ci, ci, ci] + [vp] * 11; L.shim_tick.restype = None
    L.shim_random_progress.argtypes = [C.c_ulonglong, ci, ci, ll, vp]; L.shim_random_progress.restype = None
    L.shim_slot_of.argtypes = [ll] * 4; L.shim_slot_of.restype = ll
    return L


def host_progress(L, seed, n, max_len, env0=0):
    out = np.zeros(n, np.int64)
    L.shim_random_progress(seed, env0, n, max_len, out.ctypes.data)
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("episode_shim"))


def test_abi_symbols_are_the_headers_and_nobody_elses():
    names = sorted(set(re.findall(r"\b(mpc_episode_[a-z_]+)\s*\(", open(HEADER).read())))
    assert names == sorted(E.SYMBOLS)
    others = set(_lib.SYMBOLS) | set(P.SYMBOLS) | set(P.UPDATE_SYMBOLS) | set(rl_task.SYMBOLS) | set(toy_sim.SYMBOLS) | set(terrain.SYMBOLS)
    assert not set(names) & others
    for h in ("mpc_batch.h", "mpc_ppo.h", "mpc_ppo_update.h", "mpc_task.h", "mpc_sim.h", "mpc_terrain.h"):
        assert "mpc_episode_" not in open(os.path.join(ROOT, "include", h)).read(), h
    L = E.lib()
    for s in E.SYMBOLS:
        assert getattr(L, s).argtypes is not None, s
    # the layouts named in Python are the header's
    text = open(HEADER).read()
    enum = {k: int(v) for k, v in re.findall(r"\b(MPC_EPISODE_[A-Z_]+) = (\d+)", text)}
    assert (enum["MPC_EPISODE_HEAD"], enum["MPC_EPISODE_COUNT"], enum["MPC_EPISODE_COUNTERS"], enum["MPC_EPISODE_COUNTER_STRIDE"]) == (E.HEAD, E.COUNT, E.COUNTERS, E.COUNTER_STRIDE)
    assert (E.HEAD, E.COUNT, E.COUNTERS, E.COUNTER_STRIDE) == (ref.HEAD, ref.COUNT, ref.COUNTERS, ref.COUNTER_STRIDE)
    assert (enum["MPC_EPISODE_S_WINDOW_COUNT"], enum["MPC_EPISODE_S_MEAN_RETURN"], enum["MPC_EPISODE_S_MEAN_LENGTH"], enum["MPC_EPISODE_S_WINDOW_TIMEOUTS"],
            enum["MPC_EPISODE_SUMMARY_TOTALS"], enum["MPC_EPISODE_SUMMARY_STRIDE"]) == (E.S_WINDOW_COUNT, E.S_MEAN_RETURN, E.S_MEAN_LENGTH, E.S_WINDOW_TIMEOUTS,
                                                                                       E.S_TOTALS, E.S_STRIDE)
    assert (enum["MPC_EPISODE_T_EPISODES"], enum["MPC_EPISODE_T_TIMEOUTS"], enum["MPC_EPISODE_T_SUM_RETURN"], enum["MPC_EPISODE_T_SUM_LENGTH"]) == (
        E.T_EPISODES, E.T_TIMEOUTS, E.T_SUM_RETURN, E.T_SUM_LENGTH)
    assert enum["MPC_EPISODE_MAX_GROUPS"] == E.MAX_GROUPS


def test_bad_arguments_are_refused_without_a_gpu():
    L = E.lib()
    E_ARG = -1
    h = C.c_void_p()
    assert L.mpc_episode_create(None, 8, 100, 1) == E_ARG
    assert L.mpc_episode_create(C.byref(h), 0, 100, 1) == E_ARG and b"n must" in L.mpc_episode_last_error()
    assert L.mpc_episode_create(C.byref(h), -3, 100, 1) == E_ARG
    assert L.mpc_episode_create(C.byref(h), 8, 0, 1) == E_ARG and b"window" in L.mpc_episode_last_error()
    assert L.mpc_episode_create(C.byref(h), 8, 100, 0) == E_ARG and b"groups" in L.mpc_episode_last_error()
    assert L.mpc_episode_create(C.byref(h), 8, 100, E.MAX_GROUPS + 1) == E_ARG
    assert not h.value
    assert L.mpc_episode_create(C.byref(h), 8, 100, E.MAX_GROUPS) == 0 and h.value          # a handle needs no device
    p = 0x1000
    good = [p] * 8 + [None]
    assert L.mpc_episode_bind(None, C.addressof(E._Buffers(*good))) == E_ARG and L.mpc_episode_bind(h, None) == E_ARG
    for k in range(8):                                                                       # every buffer but the groups is needed
        bad = list(good); bad[k] = None
        b = E._Buffers(*bad)
        assert L.mpc_episode_bind(h, C.addressof(b)) == E_ARG and b"non-null" in L.mpc_episode_last_error(), k
    # nothing bound: every launch refuses, before any device call
    assert L.mpc_episode_add(h, p, p, p, None) == E_ARG and b"bound" in L.mpc_episode_last_error()
    assert L.mpc_episode_summary(h, None) == E_ARG and L.mpc_episode_restart(h, None) == E_ARG and L.mpc_episode_clear(h, None) == E_ARG
    assert L.mpc_episode_add(None, p, p, p, None) == E_ARG and L.mpc_episode_add(h, None, p, p, None) == E_ARG
    assert L.mpc_episode_add(h, p, None, p, None) == E_ARG and L.mpc_episode_add(h, p, p, None, None) == E_ARG
    assert L.mpc_episode_summary(None, None) == E_ARG and L.mpc_episode_restart(None, None) == E_ARG and L.mpc_episode_clear(None, None) == E_ARG
    L.mpc_episode_destroy(h)
    L.mpc_episode_destroy(None)
    assert L.mpc_episode_random_progress(None, 8, 100, 1, None) == E_ARG and L.mpc_episode_random_progress(p, 0, 100, 1, None) == E_ARG
    assert L.mpc_episode_random_progress(p, 8, 0, 1, None) == E_ARG and b"max_len" in L.mpc_episode_last_error()
    assert L.mpc_episode_random_progress(p, 8, 2 ** 31 + 1, 1, None) == E_ARG


def test_classes_raise_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.MpcLibraryError):
        E.EpisodeStats(8)
    with pytest.raises(_lib.MpcLibraryError):
        rl_mpc_locomotion_amd.EpisodeStats(8, window=3)
    with pytest.raises(_lib.MpcLibraryError):
        E.random_progress(torch.zeros(8, dtype=torch.long), 100, 1)


def test_slot_rule(shim):
    """Every slot has exactly one writer, whatever the head, and the writers are the last cap by rank."""
    for cap in (1, 3, 100):
        for head in sorted({0, cap // 2, cap - 1}):
            for total in (0, 1, cap - 1, cap, cap + 1, 3 * cap + 2):
                slots = [shim.shim_slot_of(head, r, total, cap) for r in range(total)]
                kept = [s for s in slots if s >= 0]
                assert len(kept) == min(total, cap) == len(set(kept)) and all(0 <= s < cap for s in kept)
                assert all(s < 0 for s in slots[:max(0, total - cap)]) and kept == [(head + r) % cap for r in range(max(0, total - cap), total)]


@pytest.mark.parametrize("cap", ref.CAPS)
@pytest.mark.parametrize("n", ref.NS)
def test_host_build_matches_the_model_tick_by_tick(shim, n, cap):
    for G in ref.GROUPS:
        groups, ticks = ref.make_case(n, cap, G, seed=1000 * n + 10 * cap + G)
        model = ref.Model(n, cap, G, groups)
        st = dict(cur_return=np.zeros(n, np.float32), cur_length=np.zeros(n, np.int32), win_return=np.zeros(cap, np.float32), win_length=np.zeros(cap, np.int32),
                  win_timed_out=np.zeros(cap, np.int32), counters=np.zeros(2 + 3 * (1 + G), np.int64), sums=np.zeros(1 + G, np.float64))
        gr = np.ascontiguousarray(groups.numpy(), dtype=np.int32)
        finished = 0
        for t, (rew, reset, time_outs) in enumerate(ticks):
            model.add(rew, reset, time_outs)
            shim.shim_tick(n, cap, G, *(st[k].ctypes.data for k in ("cur_return", "cur_length", "win_return", "win_length", "win_timed_out", "counters", "sums")),
                           gr.ctypes.data, rew.numpy().ctypes.data, reset.numpy().ctypes.data, time_outs.numpy().ctypes.data)
            ref.check_state(model, st, f"n {n} cap {cap} G {G} tick {t}")
            finished += int((reset > 0).sum())
        assert model.blocks[0]["episodes"] == finished >= 2 * n + 2 and (n == 1 or 0 < model.blocks[0]["timeouts"] < finished)


def test_no_groups_means_group_zero(shim):
    n, cap = 65, 3
    _, ticks = ref.make_case(n, cap, 1, seed=3)
    model = ref.Model(n, cap, 1, None)
    st = dict(cur_return=np.zeros(n, np.float32), cur_length=np.zeros(n, np.int32), win_return=np.zeros(cap, np.float32), win_length=np.zeros(cap, np.int32),
              win_timed_out=np.zeros(cap, np.int32), counters=np.zeros(5 + 3, np.int64), sums=np.zeros(2, np.float64))
    for rew, reset, time_outs in ticks:
        model.add(rew, reset, time_outs)
        shim.shim_tick(n, cap, 1, *(st[k].ctypes.data for k in ("cur_return", "cur_length", "win_return", "win_length", "win_timed_out", "counters", "sums")),
                       None, rew.numpy().ctypes.data, reset.numpy().ctypes.data, time_outs.numpy().ctypes.data)
    ref.check_state(model, st, "no groups")
    assert list(st["counters"][2:5]) == list(st["counters"][5:8]) and st["sums"][0] == st["sums"][1]


def test_random_progress_on_the_host_build(shim):
    max_len = 2000
    a, b = host_progress(shim, 7, 65, max_len), host_progress(shim, 7, 1100, max_len)
    assert np.array_equal(a, b[:65]) and np.array_equal(host_progress(shim, 7, 5, max_len, env0=60), b[60:65])   # a draw does not depend on n
    assert not np.array_equal(host_progress(shim, 8, 1100, max_len), b)
    M = 2000 * 500                                                               # 500 expected per bucket
    x = host_progress(shim, 1, M, max_len)
    assert x.min() >= 0 and x.max() < max_len
    counts = np.bincount(x, minlength=max_len)
    p = 1.0 / max_len
    sd = np.sqrt(M * p * (1 - p))
    print(f"random_progress: {M} draws over {max_len} buckets, counts {counts.min()} .. {counts.max()}, largest deviation {np.abs(counts - M * p).max() / sd:.2f} sd")
    assert np.abs(counts - M * p).max() < 5 * sd
    assert abs(x.mean() - (max_len - 1) / 2) < 5 * np.sqrt((max_len ** 2 - 1) / 12 / M)
    for edge in (1, 2, 2 ** 31):
        y = host_progress(shim, 3, 4096, edge)
        assert y.min() >= 0 and y.max() < edge
    assert host_progress(shim, 3, 4096, 2 ** 31).max() > 2 ** 30


def test_trainer_refuses_random_lengths_for_an_environment_without_them(monkeypatch):
    """learn(init_at_random_ep_len=True) needs progress_buf and cfg.max_episode_length: checked before anything runs."""
    class Env:
        num_envs, num_obs, num_actions = 4, 48, 12
    t = P.PPOTrainer.__new__(P.PPOTrainer)
    t.env, t.obs, t.seed = Env(), None, 1
    with pytest.raises(ValueError):
        t.learn(1, init_at_random_ep_len=True)
    Env.progress_buf = torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError):
        t.learn(1, init_at_random_ep_len=True)


def test_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = tmp_path / "mpc_episode.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "mpc_episode.hip"), "-o", str(out)], check=True, capture_output=True, text=True)
    found = {}
    for name, scratch in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S):
        found[name] = int(scratch)
    for kernel in ("accumulate_kernel", "scan_kernel", "place_kernel", "summary_kernel", "random_progress_kernel"):
        hit = [s for k, s in found.items() if kernel in k]
        assert hit == [0], (kernel, found)
