"""The persistent job kernel at h = 10 (mpc_solve_jobs_kernel<10>: the ADMM part and the polish of a solve as two jobs, each loading its
records in one batch, Solver::load_batched) against the one-workgroup-per-robot single-pass kernel (MPC_SOLVE_JOBS=0), bit for bit.

Both run the same arithmetic on the same records; what differs is how a job gets them -- through the LDS stage, from whichever wave took
the job, a polish job possibly on another XCD than its ADMM job -- and what the polish job writes back.  Sizes: 1 and 5 launch fewer
workgroups than the chip has wave slots; 1030 is more than the 1024 slots, so some waves run two ADMM jobs (the stage is reused) and the
polish jobs land on other waves than their ADMM jobs."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload
from tests.helpers import inertia9_from_diag, load_golden

pytestmark = pytest.mark.gpu
H = 10


def _pair(monkeypatch, mass, inertia_diag, dt, alpha):
    """(default launch, single-pass launch): mpc_batch_create reads MPC_SOLVE_JOBS when the handle is created."""
    from rl_mpc_locomotion_amd.batched import BatchedConvexMpc
    monkeypatch.delenv("MPC_SOLVE_JOBS", raising=False)
    jobs = BatchedConvexMpc(mass, inertia9_from_diag(inertia_diag), H, dt, alpha, device="cuda:0")
    monkeypatch.setenv("MPC_SOLVE_JOBS", "0")
    one = BatchedConvexMpc(mass, inertia9_from_diag(inertia_diag), H, dt, alpha, device="cuda:0")
    monkeypatch.delenv("MPC_SOLVE_JOBS")
    return jobs, one


def _solve(gpu, rec):
    import torch
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
    return ij


@pytest.mark.parametrize("n", [1, 5, 1030])
def test_job_kernel_equals_the_single_pass_kernel(monkeypatch, n):
    wl = make_solver_workload(n, h=H, seed=40 + n, config=2)
    jobs, one = _pair(monkeypatch, wl.mass, wl.inertia_diag, wl.dt_mpc, wl.alpha)
    for call in range(3):      # cold, warm, warm
        info = _same_call(jobs, one, wl.inputs, f"n = {n}, call {call}")
        assert (info[:, 5] == (call == 0)).all()
        # the profile record of the job kernel: slot 15 (the ADMM job's duration, the next launch's dispatch key) of every robot, slot 0
        # (the polish job's duration, one plain store) exactly where a polish job ran
        prof = jobs.get_profile()
        assert (prof[:, 15] != 0).all(), np.nonzero(prof[:, 15] == 0)[0][:8]
        assert np.array_equal(prof[:, 0] > 0, info[:, 2] != 0), np.nonzero((prof[:, 0] > 0) != (info[:, 2] != 0))[0][:8]
        assert (prof[:, 0] >= 0).all()
        wl = perturb_workload(wl, 900 + call)


def test_job_kernel_equals_the_single_pass_kernel_on_the_edge_rows(monkeypatch):
    """The rows of the edge fixture (a failed solve clears the record and leaves its force row untouched; every other row is written)."""
    g = load_golden("solver_h10_edge")
    assert int(g["h"]) == H
    jobs, one = _pair(monkeypatch, g["mass"], g["inertia_diag"], float(g["dt_mpc"]), float(g["alpha"]))
    for s in range(int(g["steps"])):
        info = _same_call(jobs, one, g[f"inputs_{s}"], f"edge rows, step {s}")
        assert np.array_equal(info[:, :4], g[f"info_{s}"])
        prof = jobs.get_profile()
        assert (prof[:, 15] != 0).all()
        assert np.array_equal(prof[:, 0] > 0, info[:, 2] != 0)
