"""The h = 10 solve kernels after the factorisation set-up's changes (mpc_wrench.h: D and E of a foot lane in registers from the job's prologue on,
Solver::Dat / Eat; the structured c Theta_ij, Solver::th_nz) on small batches that walk every path of a job.

The persistent job kernel runs with SIX wave slots (MPC_SOLVE_JOBS=6: not a multiple of a CU's four), so a slot takes about ten ADMM jobs and
ten polish jobs of a 64-robot batch one after the other -- the registers and the LDS stage of one job are the next job's -- and is compared
bit for bit (forces, state records, info) with the one-workgroup-per-robot single-pass kernel (MPC_SOLVE_JOBS=0), over a cold and two
warm-started calls.  Both are held to the goldens' decisions and to the parity tolerance of tests/test_gpu_parity.py.  The fixtures are tiled to 64
rows.  What the inputs exercise is asserted, not assumed: re-factorisations (info[3] > 0), polishes taken and rejected (info[2] == 1 / -1)
in every golden case, robots that do not end SOLVED in the infeasible batch (checked against the oracle on the CPU)."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from tests.helpers import grf_relerr, grf_rtol, inertia9_from_diag, load_golden, GRF_RTOL

pytestmark = pytest.mark.gpu
H = 10
SLOTS = 6


def _pair(monkeypatch, mass, inertia_diag, dt, alpha):
    """(job kernel on SLOTS wave slots, single-pass launch): mpc_batch_create reads MPC_SOLVE_JOBS when the handle is created."""
    from rl_mpc_locomotion_amd.batched import BatchedConvexMpc
    monkeypatch.setenv("MPC_SOLVE_JOBS", str(SLOTS))
    jobs = BatchedConvexMpc(mass, inertia9_from_diag(inertia_diag), H, dt, alpha, device="cuda:0")
    monkeypatch.setenv("MPC_SOLVE_JOBS", "0")
    one = BatchedConvexMpc(mass, inertia9_from_diag(inertia_diag), H, dt, alpha, device="cuda:0")
    monkeypatch.delenv("MPC_SOLVE_JOBS")
    return jobs, one


def _solve(gpu, rec):
    import torch
    gpu.forces.fill_(777.0)      # (a robot that does not end SOLVED leaves its row untouched)
    f, info = gpu.solve(torch.from_numpy(np.ascontiguousarray(rec, dtype=np.float32)).to("cuda:0"))
    torch.cuda.synchronize()
    return f.cpu().numpy().copy(), info.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_call(jobs, one, rec, what):
    fj, ij = _solve(jobs, rec)
    fo, io = _solve(one, rec)
    assert np.array_equal(ij, io), f"{what}: info differs in rows {np.nonzero((ij != io).any(1))[0][:8]}"
    assert np.array_equal(_bits(fj), _bits(fo)), f"{what}: forces differ in rows {np.nonzero((_bits(fj) != _bits(fo)).any(1))[0][:8]}"
    sj, so = jobs.get_state(), one.get_state()
    assert np.array_equal(_bits(sj), _bits(so)), f"{what}: state records differ in rows {np.nonzero((_bits(sj) != _bits(so)).any(1))[0][:8]}"
    return fj, ij


def _golden_calls(name, n, monkeypatch):
    """Three calls (cold, warm, warm) on the fixture's rows tiled to n; the calls the fixture recorded are compared with it.  Returns the infos."""
    g = load_golden(name)
    assert int(g["h"]) == H
    rows = np.arange(n) % len(g["mass"])
    jobs, one = _pair(monkeypatch, g["mass"][rows], g["inertia_diag"][rows], float(g["dt_mpc"]), float(g["alpha"]))
    steps, infos = int(g["steps"]), []
    for call in range(3):
        s = min(call, steps - 1)      # (a fixture of two calls: its last inputs once more, warm)
        f, info = _same_call(jobs, one, g[f"inputs_{s}"][rows], f"{name}, n = {n}, call {call}")
        assert (info[:, 5] == (call == 0)).all()
        if call < steps:
            assert np.array_equal(info[:, :4], g[f"info_{s}"][rows]), (name, call)
            ok = info[:, 1] == 1
            err = grf_relerr(f[ok], g[f"forces_{s}"][rows][ok], first_step_only=False).max()
            print(f"{name} n={n} call {call}: max rel. force error against the golden {err:.3e} (bound {grf_rtol(name):.0e})")
            assert err < grf_rtol(name), (name, call, err)
        infos.append(info)
    return infos


@pytest.mark.parametrize("name", ["solver_h10_cfg2", "solver_h10_cfg3", "solver_h10_edge", "solver_h10_stress"])
def test_64_robots_on_six_slots_equal_the_single_pass_kernel_and_the_golden(monkeypatch, name):
    infos = np.concatenate(_golden_calls(name, 64, monkeypatch))
    if name == "solver_h10_cfg3":
        assert sorted(set(load_golden(name)["robot_type"].tolist())) == [0, 1, 2]
    assert (infos[:, 3] > 0).any(), "no robot re-factorised"
    assert (infos[:, 2] == 1).any() and (infos[:, 2] == -1).any(), "the polish was not both taken and rejected"
    assert (infos[:, 4] >= 2).all()      # (an ADMM factorisation and, every robot being SOLVED here, a polish factorisation)


@pytest.mark.parametrize("n", [1, 5])
def test_fewer_robots_than_slots(monkeypatch, n):
    """One workgroup, and five (a CU's four slots and one more): the three robot types of config 3."""
    _golden_calls("solver_h10_cfg3", n, monkeypatch)


def test_robots_that_do_not_end_solved(monkeypatch):
    """A third of the batch is primal infeasible (tests/helpers.infeasible_workload): status -3 at the check where OSQP finds its certificate, no
    polish job, force rows untouched; the rest solve as usual beside them.  Decisions against the oracle's OSQP on the CPU."""
    from oracle.refmpc import RefBatch
    from rl_mpc_locomotion_amd.synthetic import perturb_workload
    from tests.helpers import infeasible_workload
    wl, inp = infeasible_workload(n=64)
    n = len(wl.mass)
    jobs, one = _pair(monkeypatch, wl.mass, wl.inertia_diag, wl.dt_mpc, wl.alpha)
    ref = RefBatch(wl.mass, wl.inertia_diag, H, wl.dt_mpc, wl.alpha)
    for call in range(3):
        f, info = _same_call(jobs, one, inp, f"infeasible third, call {call}")
        fr = ref.solve(inp, nthreads=8)
        assert (ref.info[:n // 3, 1] != 1).all() and (ref.info[n // 3:, 1] == 1).any()      # (what this case is for, by the oracle)
        assert np.array_equal(info[:, :4], ref.info[:, :4].astype(np.int32)), call
        assert (info[:n // 3, 1] == -3).all() and (info[:n // 3, 2] == 0).all() and (f[:n // 3] == 777.0).all()
        ok = ref.info[:, 1] == 1
        assert grf_relerr(f[ok], fr[ok]).max() < GRF_RTOL
        inp = inp.copy()
        inp[n // 3:] = perturb_workload(wl, 60 + call).inputs[n // 3:]
