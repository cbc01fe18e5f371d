"""The pair sweep's reordered fetch (mpc_wrench.h Solver::sweep_pair: piv, the pivot rows at the lane's tile column, then those at its tile row; the
arithmetic and its order unchanged) on the GPU, on few wave slots as tests/test_kform_gpu.py arranges it: the persistent job kernel on SIX slots
(MPC_SOLVE_JOBS=6), so that a slot runs several ADMM and polish jobs one after the other, against the single-pass kernel (MPC_SOLVE_JOBS=0) bit for
bit, and both against the live oracle with the tolerance and the decision check of tests/test_gpu_parity.py.

h = 2 is the smallest horizon with an off-diagonal tile and a hand-over from one tile row to the next, h = 3 the smallest with a tile in neither the
pivot row nor the pivot column (8 robots each); h = 10 is the shipped shape (the 64 rows of the golden batch solver_h10_cfg2, tiled).  A robot with
a non-finite input walks the sweep's breakdown flag: it fails alone."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload
from tests.helpers import GRF_RTOL, grf_relerr, inertia9_from_diag, load_golden

pytestmark = pytest.mark.gpu
SLOTS = 6


def _pair(monkeypatch, mass, inertia_diag, h, dt, alpha):
    from rl_mpc_locomotion_amd.batched import BatchedConvexMpc
    monkeypatch.setenv("MPC_SOLVE_JOBS", str(SLOTS))
    jobs = BatchedConvexMpc(mass, inertia9_from_diag(inertia_diag), h, dt, alpha, device="cuda:0")
    monkeypatch.setenv("MPC_SOLVE_JOBS", "0")
    one = BatchedConvexMpc(mass, inertia9_from_diag(inertia_diag), h, dt, alpha, device="cuda:0")
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
    return fj, ij, sj


def _against_oracle(monkeypatch, mass, inertia_diag, h, dt, alpha, calls):
    """Cold and warm-started calls: job kernel = single-pass kernel bit for bit; decisions equal to the oracle's, forces within GRF_RTOL."""
    from oracle.refmpc import RefBatch
    jobs, one = _pair(monkeypatch, mass, inertia_diag, h, dt, alpha)
    ref = RefBatch(mass, inertia_diag, h, dt, alpha)
    for call, rec in enumerate(calls):
        f, info, _ = _same_call(jobs, one, rec, f"h = {h}, call {call}")
        fr = ref.solve(rec, nthreads=8)
        assert np.array_equal(info[:, :4], ref.info[:, :4].astype(np.int32)), (h, call)
        ok = ref.info[:, 1] == 1
        assert ok.any()
        err = grf_relerr(f[ok], fr[ok], first_step_only=False).max()
        print(f"h = {h}, call {call}: max rel. force error against the oracle {err:.3e} (bound {GRF_RTOL:.0e})")
        assert err < GRF_RTOL, (h, call, err)


@pytest.mark.parametrize("h", [2, 3])
def test_short_horizons_on_six_slots(monkeypatch, h):
    wl = make_solver_workload(8, h=h, seed=90 + h, config=2)
    calls = [wl.inputs, perturb_workload(wl, 900).inputs, perturb_workload(wl, 901).inputs]
    _against_oracle(monkeypatch, wl.mass, wl.inertia_diag, h, wl.dt_mpc, wl.alpha, calls)


def test_64_golden_robots_on_six_slots(monkeypatch):
    g = load_golden("solver_h10_cfg2")
    assert int(g["h"]) == 10
    rows = np.arange(64) % len(g["mass"])
    steps = int(g["steps"])
    calls = [g[f"inputs_{min(c, steps - 1)}"][rows] for c in range(3)]
    _against_oracle(monkeypatch, g["mass"][rows], g["inertia_diag"][rows], 10, float(g["dt_mpc"]), float(g["alpha"]), calls)


@pytest.mark.parametrize("h", [2, 10])
def test_a_robot_with_a_non_finite_input_fails_alone(monkeypatch, h):
    n, bad = 8, 3
    wl = make_solver_workload(n, h=h, seed=90 + h, config=2)
    inp = wl.inputs.copy()
    inp[bad, 0] = np.nan
    keep = np.arange(n) != bad
    jobs, one = _pair(monkeypatch, wl.mass, wl.inertia_diag, h, wl.dt_mpc, wl.alpha)
    fg, ig, sg = _same_call(jobs, one, wl.inputs, f"h = {h}, all robots good")
    assert (ig[:, 1] == 1).all()
    jobs, one = _pair(monkeypatch, wl.mass, wl.inertia_diag, h, wl.dt_mpc, wl.alpha)
    f, info, st = _same_call(jobs, one, inp, f"h = {h}, robot {bad} non-finite")
    assert info[bad, 1] == -7 and (f[bad] == 777.0).all()      # NON_CVX, its force row untouched
    assert np.array_equal(info[keep], ig[keep]) and np.array_equal(_bits(f[keep]), _bits(fg[keep])) and np.array_equal(_bits(st[keep]), _bits(sg[keep]))
