"""The recurrent actor-critic's whole update on the device (``RecurrentConfig(update_through_time="hip", update_heads="hip")``; include/mpc_ppo_update.h's
mpc_ppo_update_set_sequence_rows, mpc_ppo_update_grads_sequence, mpc_ppo_update_bind_extra) on the CPU: the option and its refusals, the refusals that
stay as they were, the new entry points' argument checks through ctypes, and the launch sequence restated against csrc/ppo_gemm_plan.h under g++.

A handle of include/mpc_ppo_update.h exists only on a device (mpc_ppo_update_create needs a bound mpc_ac), so what is checked here is every refusal that
looks at the arguments alone -- each entry point makes those before it looks at the handle -- and the two that need a handle's state
(mpc_ppo_update_grads_sequence before mpc_ppo_update_set_sequence_rows, mpc_ppo_update_apply with extras that have no moments) are in
tests/test_recurrent_update_gpu.py, where they come back before any launch."""
import ctypes as C
import subprocess

import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, ppo as P, recurrent as RC
from tests.test_ppo_update import CSRC

I, H = 48, 16
NETS = ((32, 16), (64,))
FORWARD, BACKWARD_DATA, BACKWARD_WEIGHT, BACKWARD_DATA_LINEAR = 0, 1, 2, 3
NARROW, WIDE = "narrow", "wide"

# ---- what tests/test_recurrent_update_gpu.py runs (it imports these): (I, H, nets, T, N, mini-batches, critic width or None) ------------------------------
SMALL = [(I, H, NETS, T, N, mb, None) for T in (1, 5) for N, mb in ((16, 1), (34, 2), (104, 2))]      # B = 16; 17: across a 16-row workgroup edge; 52
PRIVILEGED = (I, H, NETS, 5, 34, 2, 64)
WIDE_STATE = (I, 256, NETS, 3, 17, 1, None)
# one case on the plan of the training workload: 16 385 rows (17 chunks of 1024, the last of one row), the reference nets behind 256-wide memories
PRODUCTION = (I, 256, ((512, 256, 128), (512, 256, 128)), 5, 3277, 1, None)
CASES = SMALL + [PRIVILEGED, WIDE_STATE, PRODUCTION]


def case_rows(case):
    _, _, _, T, N, mb, _ = case
    return T * (N // mb)


# ---- the option ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_option_constructs_and_is_refused_on_the_host():
    cfg = RC.RecurrentConfig(update_heads="hip", update_through_time="hip")
    assert cfg.update_heads == "hip" and RC.RecurrentConfig().update_heads == "torch" and RC.RecurrentConfig(update_through_time="hip").update_heads == "torch"
    ac = RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H, update_through_time="hip", update_heads="hip")
    assert ac.update_heads == "hip" and RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H).update_heads == "torch"
    for make in (lambda: RC.RecurrentConfig(update_heads="hip"), lambda: RC.RecurrentConfig(update_heads="hip", update_through_time="torch"),
                 lambda: RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H, update_heads="hip")):
        with pytest.raises(ValueError, match='update_heads="hip" requires update_through_time="hip"'):
            make()
    for bad in ("cuda", None, "HIP"):
        for make in (lambda: RC.RecurrentConfig(update_through_time="hip", update_heads=bad),
                     lambda: RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H, update_through_time="hip", update_heads=bad)):
            with pytest.raises(ValueError, match="update_heads=.*'torch' or 'hip'"):
                make()


def test_ppo_takes_the_device_path_from_the_actor_critic(monkeypatch):
    plain = RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H, update_through_time="hip")
    alg = P.PPO(plain)
    assert alg.backend == "torch" and not alg.device_update and alg.lr_device is None
    assert not P.PPO(P.ActorCritic(I, 12, *NETS)).device_update
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ac = RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H, update_through_time="hip", update_heads="hip")
    with pytest.raises(_lib.MpcLibraryError, match="needs a GPU"):
        P.PPO(ac)

    class Env:
        num_envs, num_obs, num_actions = 4, 48, 12
    with pytest.raises(_lib.MpcLibraryError, match="needs a GPU"):
        P.PPOTrainer(Env(), recurrent=RC.RecurrentConfig(hidden_size=H, update_through_time="hip", update_heads="hip"))


def test_the_pinned_refusals_are_unchanged():
    for kw in ({}, {"update_through_time": "hip"}, {"update_through_time": "hip", "update_heads": "hip"}):
        ac = RC.ActorCriticRecurrent(I, 12, *NETS, rnn_hidden_size=H, **kw)
        with pytest.raises(ValueError, match="not built.*update_through_time"):
            P.PPO(ac, backend="hip")
        with pytest.raises(ValueError, match="not built.*update_through_time"):
            P.PPOTrainer(None, update="hip", recurrent=RC.RecurrentConfig(hidden_size=H, **kw))
    with pytest.raises(ValueError, match="backend is 'torch' or 'hip'"):
        P.PPO(P.ActorCritic(I, 12, *NETS), backend="device")


# ---- the entry points' argument checks -------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_refuse_before_the_device():
    L = P.update_lib()
    for name in ("mpc_ppo_update_set_sequence_rows", "mpc_ppo_update_grads_sequence", "mpc_ppo_update_bind_extra"):
        assert name in P.UPDATE_SYMBOLS and getattr(L, name).argtypes is not None
    E_ARG = -1
    err = L.mpc_ppo_last_error
    ptrs = lambda *v: _lib.ptr_array(list(v))
    ints = lambda *v: _lib.int_array(list(v))
    rows = L.mpc_ppo_update_set_sequence_rows
    a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000
    for k in range(4):                                                           # all four, or none
        some = [a, b, c, d]; some[k] = None
        assert rows(None, *some) == E_ARG and b"all four buffers, or four NULLs" in err()
    for k in range(4):
        bad = [a, b, c, d]; bad[k] += 4
        assert rows(None, *bad) == E_ARG and b"16-byte aligned" in err()
    for bad in ((a, b, c, c), (a, b, a, d), (a, b, b, d), (a, b, c, a), (a, b, c, b)):      # the outputs on each other, on a row buffer
        assert rows(None, *bad) == E_ARG and b"must not overlap" in err()
    assert rows(None, a, b, c, d) == E_ARG and b"mpc_ppo_update_set_sequence_rows: bad argument" in err()      # every check of the arguments passed
    assert rows(None, None, None, None, None) == E_ARG and b"bad argument" in err()
    seq = L.mpc_ppo_update_grads_sequence
    assert seq(None, 8, a, 0.2, 1.0, 0.01, 1, 1, 0.01, a, a, None) == E_ARG and b"mpc_ppo_update_grads_sequence: bad argument" in err()
    assert L.mpc_ppo_update_grads(None, 8, a, 0.2, 1.0, 0.01, 1, 1, 0.01, a, a, None) == E_ARG and b"mpc_ppo_update_grads: bad argument" in err()
    extra = L.mpc_ppo_update_bind_extra
    eight = [0x100000 * (k + 1) for k in range(9)]
    for count in (-1, 9, 100):
        assert extra(None, count, ptrs(*eight), ptrs(*eight), ptrs(*eight), ptrs(*eight), ints(*[16] * 9)) == E_ARG and b"count must lie in 0 .. 8" in err()
    good, n2 = ptrs(a, b), ints(64, 16)
    assert extra(None, 2, None, good, good, good, n2) == E_ARG and b"bad argument" in err()
    assert extra(None, 2, good, None, good, good, n2) == E_ARG and b"bad argument" in err()
    assert extra(None, 2, good, good, good, good, None) == E_ARG and b"bad argument" in err()
    assert extra(None, 2, good, good, good, None, n2) == E_ARG and b"both moments or neither" in err()
    assert extra(None, 2, good, good, None, good, n2) == E_ARG and b"both moments or neither" in err()
    assert extra(None, 2, good, good, good, good, ints(64, 0)) == E_ARG and b"at least one element" in err()
    for k in range(4):
        for bad in (ptrs(a, b + 8), ptrs(a, 0)):                                 # misaligned, null
            args = [good] * 4; args[k] = bad
            assert extra(None, 2, *args, n2) == E_ARG and b"non-null and 16-byte aligned" in err(), k
    assert extra(None, 2, good, good, None, None, n2) == E_ARG and b"mpc_ppo_update_bind_extra: bad argument" in err()      # (no moments is allowed: apply refuses)
    assert extra(None, 0, None, None, None, None, None) == E_ARG and b"mpc_ppo_update_bind_extra: bad argument" in err()


# ---- the launch sequence ------------------------------------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "ppo_gemm_plan.h"
extern "C" {
void shim_plan(int kind, const int *mnk, int *out) {
  const pgemm::Shape shape[2] = {{mnk[0], mnk[1], mnk[2]}, {mnk[3], mnk[4], mnk[5]}};
  const pgemm::Plan p = pgemm::plan_gemm(kind, shape);
  out[0] = p.chunk_rows; out[1] = p.wide ? 1 : 0; out[2] = (int)p.grid_x;
  for (int k = 0; k < 2; ++k) { out[3 + 3 * k] = p.p[k].tiles_m; out[4 + 3 * k] = p.p[k].tiles_n; out[5 + 3 * k] = p.p[k].chunks; }
}
int shim_kinds() { return pgemm::kForward == 0 && pgemm::kBackwardData == 1 && pgemm::kBackwardWeight == 2 && pgemm::kBackwardDataLinear == 3; }
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("recurrent_update_plan_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.shim_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p]; L.shim_plan.restype = None
    assert L.shim_kinds() == 1

    def run(kind, a, b=None):
        mnk = (C.c_int * 6)(*(a or (0, 0, 0)), *(b or (0, 0, 0)))
        out = (C.c_int * 9)()
        L.shim_plan(kind, mnk, out)
        return dict(chunk_rows=out[0], tile=WIDE if out[1] else NARROW, grid_x=out[2], problems=[tuple(out[3:6]), tuple(out[6:9])])
    return run


def launches(nets, rows, hidden):
    """mpc_ppo_update_grads_sequence's GEMM launches, copied by hand from csrc/mpc_ppo_update.hip: mpc_ppo_update_grads' sequence (as
    tests/test_ppo_gemm_plan.py restates it) on first layers ``hidden`` wide, then ONE backward-data launch with no activation factor through layer 0
    of both nets: (rows, hidden, first layer's width)."""
    dims = [[hidden, *nets[0], 12], [hidden, *nets[1], 1]]
    nl = [len(d) - 1 for d in dims]
    out = []
    for l in range(max(nl)):
        out.append((FORWARD, *[(rows, d[l + 1], d[l]) if l < n else None for d, n in zip(dims, nl)]))
    for s in range(max(nl)):
        w, x = [], []
        for d, n in zip(dims, nl):
            l = n - 1 - s
            w.append((d[l + 1], d[l], rows) if l >= 0 else None)
            x.append((rows, d[l], d[l + 1]) if l > 0 else None)
        out.append((BACKWARD_WEIGHT, *w))
        if any(x):
            out.append((BACKWARD_DATA, *x))
    out.append((BACKWARD_DATA_LINEAR, *[(rows, d[0], d[1]) for d in dims]))
    return out


def planned(plan, nets, rows, hidden):
    out = []
    for kind, a, b in launches(nets, rows, hidden):
        p = plan(kind, a, b)
        out.append((kind, p["tile"], p["chunk_rows"], (p["problems"][0][2], p["problems"][1][2])))
    return out


def combos(plan, nets, rows, hidden):
    return {(kind, tile, chunk_rows) for kind, tile, chunk_rows, _ in planned(plan, nets, rows, hidden)}


def test_the_sequence_is_the_feed_forward_one_and_one_launch_more(plan):
    from tests import test_ppo_gemm_plan as G
    for nets, rows, hidden in ((NETS, 85, 16), (NETS, 260, 16), (PRODUCTION[2], 24576, 256)):
        mine = launches(nets, rows, hidden)
        assert mine[:-1] == G.launches(nets, rows, num_obs=hidden) and mine[-1][0] == BACKWARD_DATA_LINEAR and len(mine) == len(G.launches(nets, rows, hidden)) + 1
    # the new kind is planned as backward data is: the same tile and grid for the same shapes
    for a, b in (((51, 256, 32), (51, 256, 64)), ((24576, 256, 512), (24576, 256, 512)), ((16385, 256, 512), (16385, 256, 512)), ((260, 16, 32), None)):
        assert plan(BACKWARD_DATA_LINEAR, a, b) == plan(BACKWARD_DATA, a, b)


def test_the_recurrent_workload_plan_launch_by_launch(plan):
    nets = PRODUCTION[2]
    assert nets == (P.PPOConfig().actor_hidden_dims, P.PPOConfig().critic_hidden_dims)
    assert planned(plan, nets, 24576, 256) == [
        (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, NARROW, 0, (1, 1)),
        (BACKWARD_WEIGHT, NARROW, 256, (96, 96)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 256, (96, 96)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 1024, (24, 24)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 1024, (24, 24)),
        (BACKWARD_DATA_LINEAR, WIDE, 0, (1, 1))]
    # the GPU test's own case on that plan: 17 chunks of 1024 rows, the last of one row
    assert case_rows(PRODUCTION) == 16385 and PRODUCTION[1] == 256
    big = planned(plan, nets, 16385, 256)
    assert [(k, t, c) for k, t, c, _ in big] == [(k, t, c) for k, t, c, _ in planned(plan, nets, 24576, 256)]
    assert big[-2] == (BACKWARD_WEIGHT, WIDE, 1024, (17, 17)) and big[-1] == (BACKWARD_DATA_LINEAR, WIDE, 0, (1, 1))


def test_the_workload_runs_only_kernels_the_gpu_test_runs(plan):
    """The (kind, tile, chunk length) combinations of the measured workload's mini-batch (4096 environments x 24 steps in 4 blocks: 24 576 rows behind
    256-wide memories), and of a fifth of it, are among those that the shapes of tests/test_recurrent_update_gpu.py plan."""
    tested = set()
    for case in CASES:
        tested |= combos(plan, case[2], case_rows(case), case[1])
    small = set()
    for case in SMALL + [PRIVILEGED, WIDE_STATE]:
        small |= combos(plan, case[2], case_rows(case), case[1])
    assert all(tile == NARROW and chunk_rows in (0, 256) for _, tile, chunk_rows in small)      # the edges run on the narrow tile
    assert {case_rows(c) for c in SMALL} == {16, 17, 52, 80, 85, 260}                            # 260: two 256-row weight chunks, the last of 4 rows
    assert [c for k, _, _, c in planned(plan, NETS, 260, 16) if k == BACKWARD_WEIGHT] == [(2, 2), (2, 2), (2, 1)]      # (the critic has a layer fewer)
    nets = PRODUCTION[2]
    for rows in (24576, 4896):
        production = combos(plan, nets, rows, 256)
        assert {kind for kind, _, _ in production} == {FORWARD, BACKWARD_DATA, BACKWARD_WEIGHT, BACKWARD_DATA_LINEAR}
        assert production <= tested, (rows, production - tested)
    assert (BACKWARD_DATA_LINEAR, WIDE, 0) in tested and (BACKWARD_DATA_LINEAR, NARROW, 0) in tested


def test_the_workspace_holds_every_planned_launch(plan):
    for case in CASES:
        rows = case_rows(case)
        for kind, _, chunk_rows, chunks in planned(plan, case[2], rows, case[1]):
            assert max(chunks) <= -(-rows // 256)
            assert (chunk_rows in (256, 512, 1024)) == (kind == BACKWARD_WEIGHT)


# ---- the float64 reference of the GPU tests ---------------------------------------------------------------------------------------------------------------------
def test_the_joined_restatement_is_float64_autograd():
    """tests/recurrent_update_ref.py's ``grads_restated`` (the roll and its backward pass written out, the heads by autograd) against float64 autograd all
    the way through ``PPO.losses``: every one of the 19 gradients and the four terms, on a block with every done pattern and privileged critic rows."""
    from tests import recurrent_update_ref as uref
    cpu, _ = uref.recurrent_pair(I, H, NETS, seed=3, critic_width=64)
    st = uref.filled_storage(cpu, 5, 34, seed=4)
    cfg = P.PPOConfig(actor_hidden_dims=NETS[0], critic_hidden_dims=NETS[1], num_mini_batches=2)
    assert len(uref.names(cpu)) == 19
    for i in range(2):
        got, terms, dys, _ = uref.grads_restated(cpu, cfg, st, i)
        want, terms64 = uref.grads_autograd(cpu, cfg, st, i, torch.float64)
        assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(terms, terms64))
        for k in want:
            assert float((got[k] - want[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max())), k
        assert all(float(d.abs().max()) > 0 for d in dys)
