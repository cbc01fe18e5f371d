"""The pair sweep's reordered fetch (mpc_wrench.h Solver::sweep_pair: piv, the pivot rows at the lane's tile column, then those at its tile row; the
arithmetic and its order unchanged) on the host emulation.

Horizons: h = 2 is the smallest with an off-diagonal tile and a hand-over from one tile row to the next, h = 3 the smallest with a tile in neither
the pivot row nor the pivot column, h = 10 the shipped shape.  Per horizon one cold and two warm-started solves, run once and shared by the tests:
forward and reversed thread order, poisoned registers and LDS, the live oracle with the tolerances of tests/test_emulated_kernel.py."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload
from tests.emu.emu import EmuBatch, lib
from tests.helpers import GRF_RTOL, grf_relerr

HORIZONS = (2, 3, 10)
N, STEPS = 6, 3


def _workloads(h):
    wl = make_solver_workload(N, h=h, seed=70 + h, config=2)
    out = []
    for s in range(STEPS):
        out.append(wl)
        wl = perturb_workload(wl, 800 + s)
    return out


def _run(wls, h, reverse=False, poison=False):
    wl = wls[0]
    try:
        lib().emu_set_poison(int(poison))
        emu = EmuBatch(wl.mass, wl.inertia_diag, h, wl.dt_mpc, wl.alpha)
        res = []
        for w in wls:
            f = emu.solve(w.inputs, reverse=reverse).copy()
            res.append((f, emu.info.copy(), emu.state.copy()))
    finally:
        lib().emu_set_poison(0)
    return res


@pytest.fixture(scope="module", params=HORIZONS)
def runs(request):
    h = request.param
    wls = _workloads(h)
    return h, wls, _run(wls, h)


def test_thread_order_does_not_matter(runs):
    h, wls, fwd = runs
    for (fa, ia, sa), (fb, ib, sb) in zip(fwd, _run(wls, h, reverse=True)):
        assert np.array_equal(fa, fb, equal_nan=True) and np.array_equal(ia, ib) and np.array_equal(sa, sb), h


def test_nothing_unwritten_is_read(runs):
    h, wls, clean = runs
    for (fa, ia, sa), (fb, ib, sb) in zip(clean, _run(wls, h, poison=True)):
        assert np.array_equal(fa, fb, equal_nan=True) and np.array_equal(ia, ib) and np.array_equal(sa, sb), h


def test_results_match_the_oracle(runs):
    from oracle.refmpc import RefBatch
    h, wls, res = runs
    wl = wls[0]
    ref = RefBatch(wl.mass, wl.inertia_diag, h, wl.dt_mpc, wl.alpha)
    for s, (w, (f, info, _)) in enumerate(zip(wls, res)):
        fr = ref.solve(w.inputs, nthreads=4)
        assert np.array_equal(info[:, :4], ref.info[:, :4]), (h, s)
        assert (ref.info[:, 1] == 1).all()
        err = grf_relerr(f, fr, first_step_only=False).max()
        print(f"h = {h}, call {s}: max rel. force error against the oracle {err:.3e} (bound {GRF_RTOL:.0e})")
        assert err < GRF_RTOL, (h, s, err)


@pytest.mark.parametrize("h", [2, 10])
def test_a_robot_with_a_non_finite_input_fails_alone(h):
    """The sweep's breakdown flag (a pivot block that is not positive definite): a robot whose record holds a NaN reports NON_CVX and writes no
    forces, whichever thread order, and the robots beside it solve as if it were not there."""
    wl = make_solver_workload(N, h=h, seed=70 + h, config=2)
    bad = 2
    inp = wl.inputs.copy()
    inp[bad, 0] = np.nan
    good = _run([wl], h)[0]
    for reverse in (False, True):
        emu = EmuBatch(wl.mass, wl.inertia_diag, h, wl.dt_mpc, wl.alpha)
        f = emu.solve(inp, reverse=reverse)
        assert emu.info[bad, 1] == -7 and np.isnan(f[bad]).all()      # (rows the wrapper pre-fills with NaN: no forces written)
        keep = np.arange(N) != bad
        assert np.array_equal(f[keep], good[0][keep]) and np.array_equal(emu.info[keep], good[1][keep]) and np.array_equal(emu.state[keep], good[2][keep])
