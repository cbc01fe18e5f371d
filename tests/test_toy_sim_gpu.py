"""The batched toy plant on the MI355X (include/mpc_sim.h, rl_mpc_locomotion_amd.toy_sim.BatchedToySim): its initial state and reset against
the numpy model (tests/toy_sim.py), one-step consistency inside a 1024-robot closed loop, the whole closed loop on the device against the
reference's golden, batch independence, and the Isaac-Gym-style bridge loop without copies.  Tolerances and the tie rule: tests/test_toy_sim.py."""
import copy

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd.quadruped import ROBOT_TABLE64
from tests import toy_sim as T
from tests.test_closed_loop import _cases, _check, _groups
from tests.test_toy_sim import GOLD_SLOPE, TIE, compare, decision_margin, to_record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT, BOUND, WALK = 0, 1, 6


def from_record(t, f, k):
    """Load an include/mpc_sim.h record into a numpy ToyRobot."""
    t.pos, t.quat, t.v, t.w = f[0:3].copy(), f[3:7].copy(), f[7:10].copy(), f[10:13].copy()
    t.q, t.qd, t.anchor = f[13:25].reshape(4, 3).copy(), f[25:37].reshape(4, 3).copy(), f[37:49].reshape(4, 3).copy()
    t.contact, t.lift, t.fell = k[0:4].astype(bool), k[4:8].astype(int), bool(k[8])
    return t


def _sim(rt, slope=None, yaw=None):
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    return BatchedToySim(rt, slope=slope, yaw0=yaw, device=DEV)


def _ctl(rt, gait, flat=False):
    from rl_mpc_locomotion_amd.locomotion import BatchedLocomotion
    return BatchedLocomotion(rt, gait, horizon=10, flat_ground=flat, device=DEV)


def _cmd(n, vx=0.3):
    import torch
    c = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
    c[:, 0] = vx
    return c


def test_initial_state_and_reset():
    import torch
    combos = [(rt, sl, yaw) for rt in (0, 1, 2) for sl in ((0.0, 0.0), GOLD_SLOPE) for yaw in (0.0, 0.3, -2.0)]
    rt = [c[0] for c in combos]
    slope = np.array([c[1] for c in combos])
    yaw = np.array([c[2] for c in combos])
    sim = _sim(rt, slope, yaw)
    st = sim.get_state()
    for i, (r, sl, y) in enumerate(combos):
        rf, rk = to_record(T.ToyRobot(ROBOT_TABLE64[r], yaw0=y, slope=sl))
        assert (st["i32"][i] == rk).all()
        np.testing.assert_allclose(st["f64"][i], rf, rtol=0, atol=1e-12, err_msg=f"robot type {r} slope {sl} yaw {y}")
    contact, fell = sim.flags()
    assert contact.all().item() and not fell.any().item()

    # reset mid-run: the reset robots equal a fresh create bit for bit, the others a run without the reset
    n = 64
    rts = [i % 3 for i in range(n)]
    slopes = np.array([GOLD_SLOPE if i % 2 else (0.0, 0.0) for i in range(n)])
    yaws = np.linspace(-1.0, 1.0, n)
    ids = [3, 10, 11, 40, 63]
    runs = []
    for with_reset in (False, True):
        sim, ctl = _sim(rts, slopes, yaws), _ctl(rts, [TROT] * n)
        cmd = _cmd(n)
        for k in range(60):
            sim.step(ctl.run(sim.dof_state.view(n, 12, 2), sim.root_states, cmd))
            if with_reset and k == 29:
                sim.reset_idx(torch.tensor(ids, dtype=torch.int32, device=DEV))
                ctl.reset(ids)
                fresh = _sim(rts, slopes, yaws).get_state()
                now = sim.get_state()
                assert np.array_equal(now["f64"][ids], fresh["f64"][ids]) and np.array_equal(now["i32"][ids], fresh["i32"][ids])
                obs = sim.root_states[ids].cpu().numpy()
                assert np.array_equal(obs, fresh["f64"][ids][:, :13].astype(np.float32))
        runs.append(sim.get_state())
    others = [i for i in range(n) if i not in ids]
    assert np.array_equal(runs[0]["f64"][others], runs[1]["f64"][others]) and np.array_equal(runs[0]["i32"][others], runs[1]["i32"][others])


def test_one_step_consistency_at_scale():
    n = 1024
    rng = np.random.default_rng(5)
    rt = [i % 3 for i in range(n)]
    gait = [(TROT, WALK, BOUND)[(i // 3) % 3] for i in range(n)]
    slope = np.array([GOLD_SLOPE if (i // 9) % 2 else (0.0, 0.0) for i in range(n)])
    yaw = rng.uniform(-np.pi, np.pi, n)
    sim, ctl = _sim(rt, slope, yaw), _ctl(rt, gait)
    cmd = _cmd(n)
    probe = {20, 60, 110, 150, 199}
    compared = ties = 0
    for k in range(200):
        tau = ctl.run(sim.dof_state.view(n, 12, 2), sim.root_states, cmd)
        if k in probe:
            pre, tau_h = sim.get_state(), tau.cpu().numpy().copy()
        sim.step(tau)
        if k not in probe:
            continue
        post = sim.get_state()
        alive = np.flatnonzero(pre["i32"][:, 8] == 0)          # (a fallen robot stays frozen)
        assert len(alive) >= 32
        for i in rng.choice(alive, 32, replace=False):
            t = from_record(T.ToyRobot(ROBOT_TABLE64[rt[i]], yaw0=yaw[i], slope=slope[i]), pre["f64"][i], pre["i32"][i])
            t0 = copy.deepcopy(t)
            t.step(tau_h[i])
            same, dpos, dvel = compare(post["f64"][i], post["i32"][i], t)
            compared += 1
            if not same:
                m = decision_margin(t0, tau_h[i])
                assert m < TIE, f"tick {k} robot {i}: contact / lift / fell differ with a numpy decision margin of {m:.3e}"
                ties += 1
                continue
            assert dpos <= 1e-9 and dvel <= 1e-7, f"tick {k} robot {i}: |dpos| {dpos:.3e}, |dvel| {dvel:.3e}"
    assert compared == 5 * 32
    print(f"{compared} robot steps compared, {ties} decision ties")


def test_device_closed_loop_tracks_the_reference():
    import torch
    g, names = _cases()
    for grp in _groups(names, g):
        meta = [g[n + "/meta"] for n in grp]
        rt = [int(m[0]) for m in meta]
        m = len(grp)
        ticks = [int(x[6]) for x in meta]
        sim = _sim(rt, np.array([[x[3], x[4]] for x in meta]), np.array([x[5] for x in meta]))
        ctl = _ctl(rt, [int(x[1]) for x in meta], bool(meta[0][2]))
        cmd = torch.from_numpy(np.stack([g[n + "/cmd"] for n in grp]).astype(np.float32)).to(DEV)
        K = max(ticks)
        body = torch.zeros((K, m, 13), dtype=torch.float32, device=DEV)
        cont = torch.zeros((K, m, 4), dtype=torch.bool, device=DEV)
        fell = torch.zeros((K, m), dtype=torch.bool, device=DEV)
        for k in range(K):
            c, f = sim.flags()
            body[k].copy_(sim.root_states); cont[k].copy_(c); fell[k].copy_(f)
            sim.step(ctl.run(sim.dof_state.view(m, 12, 2), torch.nan_to_num(sim.root_states, nan=0.0, posinf=0.0, neginf=0.0), cmd))
        body, cont, fell = body.cpu().numpy(), cont.cpu().numpy(), fell.cpu().numpy()
        for i, n in enumerate(grp):
            T_ = ticks[i]
            bad = (cont[:T_, i] != g[n + "/contact"][:T_].astype(bool)).any(1) | fell[:T_, i]
            first = int(np.argmax(bad)) if bad.any() else T_
            dpos = np.abs(body[:T_, i, :3] - g[n + "/body"][:T_, :3]).max(1).astype(np.float64)
            dpos[fell[:T_, i]] = np.nan
            _check(g, n, dpos, first)


def test_batch_independence():
    import torch
    n, pick = 4096, 2741
    rng = np.random.default_rng(11)
    rt = rng.integers(0, 3, n).tolist()
    gait = rng.choice([TROT, WALK, BOUND], n).tolist()
    slope = np.where(rng.random((n, 1)) < 0.5, 0.0, 1.0) * np.array(GOLD_SLOPE)
    yaw = rng.uniform(-np.pi, np.pi, n)
    cmd = _cmd(n)
    traj = []
    for sel in (slice(None), slice(pick, pick + 1)):
        idx = list(range(n))[sel]
        k_ = len(idx)
        sim, ctl = _sim([rt[i] for i in idx], slope[sel], yaw[sel]), _ctl([rt[i] for i in idx], [gait[i] for i in idx])
        j = idx.index(pick)
        rec = torch.zeros((100, 13), dtype=torch.float32, device=DEV)
        trq = torch.zeros((100, 12), dtype=torch.float32, device=DEV)
        for k in range(100):
            tau = ctl.run(sim.dof_state.view(k_, 12, 2), sim.root_states, cmd[:k_])
            sim.step(tau)
            rec[k].copy_(sim.root_states[j]); trq[k].copy_(tau[j])
        st = sim.get_state()
        traj.append((rec.cpu().numpy(), trq.cpu().numpy(), st["f64"][j], st["i32"][j]))
    (r0, t0, f0, k0), (r1, t1, f1, k1) = traj
    assert np.array_equal(t0, t1) and np.array_equal(r0, r1) and np.array_equal(f0, f1) and np.array_equal(k0, k1)


def test_bridge_loop_without_copies_and_golden_trot_stands():
    import torch
    from rl_mpc_locomotion_amd.env_bridge import MpcEnvBridge
    from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
    n = 4096
    rng = np.random.default_rng(3)
    rt = (np.arange(n) % 3).tolist()
    sim = _sim(rt, None, rng.uniform(-np.pi, np.pi, n))
    bridge = MpcEnvBridge(rt, [TROT] * n, device=DEV)
    layers = [(rng.standard_normal((32, 48)).astype(np.float32) * 0.05, np.zeros(32, np.float32)),
              (rng.standard_normal((12, 32)).astype(np.float32) * 0.05, np.zeros(12, np.float32))]
    policy = WeightPolicy(layers, device=DEV)
    cmd = _cmd(n)
    dof_ptr, root_ptr = sim.dof_state.data_ptr(), sim.root_states.data_ptr()
    actions = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
    for _ in range(100):
        torques = bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, cmd)
        dof, root = sim.step(torques)
        assert dof.data_ptr() == dof_ptr and root.data_ptr() == root_ptr
        obs = policy.observations_from(bridge.ctl, sim.dof_state.view(n, 12, 2), cmd, actions)
        _, raw = policy.step(obs, return_actions=True)
        actions = raw.clamp(-1.0, 1.0)
    assert sim.dof_state.data_ptr() == dof_ptr and sim.root_states.data_ptr() == root_ptr
    assert sim.dof_state.view(n, 12, 2).data_ptr() == dof_ptr
    _, fell = sim.flags()
    alive = ~fell
    assert torch.isfinite(sim.root_states[alive]).all().item()

    # 4096 copies of the golden's three trot-flat cases (their yaw, command and weights) stand for 1000 ticks
    g, names = _cases()
    trot = [nm for nm in names if nm.endswith("_trot_flat")]
    assert len(trot) == 3
    meta = [g[nm + "/meta"] for nm in trot]
    which = np.arange(n) % 3
    rt = [int(meta[w][0]) for w in which]
    sim = _sim(rt, None, np.array([meta[w][5] for w in which]))
    ctl = _ctl(rt, [int(meta[w][1]) for w in which], True)
    cmd = torch.from_numpy(np.stack([g[trot[w] + "/cmd"] for w in which]).astype(np.float32)).to(DEV)
    for _ in range(1000):
        sim.step(ctl.run(sim.dof_state.view(n, 12, 2), sim.root_states, cmd))
    _, fell = sim.flags()
    assert not fell.any().item(), f"{int(fell.sum())} of {n} robots fell"
