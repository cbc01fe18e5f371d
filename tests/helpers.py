import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HAVE_REFERENCE = os.path.isdir("/root/reference/MPC_Controller")

# Parity tolerance of the fp64 solve against the vendored OSQP, relative to max(|f_ref|_inf, 1 N)
# over the first-step 12 forces.  BASELINE.json's bar is 1e-3; the fp64 kernel
# reproduces OSQP's iterates, so the tests hold it to 1e-5 (observed <= 3e-7).
GRF_RTOL = 1e-5
# The stress fixture scales the weights by up to 1e9: the QP's conditioning amplifies the rounding difference between the
# reference's sparse LDL^T and the explicit inverse used here.  Decisions (iterations, status, polish, rho updates) must still
# be identical; forces are held to 2e-4 (BASELINE's bar is 1e-3).
GRF_RTOL_STRESS = 2e-4


# The derived bound of the float32 kernel tests (tests/test_ppo_gemm_gpu.py, tests/test_policy_layer_gpu.py): a float32 sum of n terms, in any order and
# fused or not, lies within gamma(n) * sum |terms| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp32(x):
    """The float32 spacing of the binade that holds |x| (float64 in), at least the smallest subnormal."""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.maximum(np.ldexp(1.0, e - 24), 2.0 ** -149)


def draw(rng, shape, scale, lo=0.5, hi=2.0):
    """float32 values of either sign whose magnitudes are log-uniform in [lo, hi] * scale: no term of a product sum is small beside the others."""
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), shape))
    return (rng.choice([-1.0, 1.0], shape) * mag * scale).astype(np.float32)


def grf_rtol(name):
    return GRF_RTOL_STRESS if name.endswith("stress") else GRF_RTOL


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def grf_relerr(f, fref, first_step_only=True):
    k = 12 if first_step_only else f.shape[1]
    return np.abs(f[:, :k] - fref[:, :k]).max(1) / np.maximum(np.abs(fref[:, :k]).max(1), 1.0)


def inertia9_from_diag(d):
    out = np.zeros((len(d), 9))
    out[:, 0], out[:, 4], out[:, 8] = d[:, 0], d[:, 1], d[:, 2]
    return out


def infeasible_workload(n=24, h=10, seed=5):
    """A config-2 batch whose first third has NEGATIVE friction coefficients (mu = -0.4): the pyramid rows then demand f_z <= 0 while
    the f_z row demands f_z >= f_min > 0 on every stance foot -- a primal infeasible QP with valid bounds (l <= u everywhere), which
    OSQP detects at its first or second termination check (auxil.c:364-424).  Returns (workload, inputs)."""
    import rl_mpc_locomotion_amd  # noqa: F401
    from rl_mpc_locomotion_amd import layout as L
    from rl_mpc_locomotion_amd.synthetic import make_solver_workload
    wl = make_solver_workload(n, h=h, seed=seed, config=2)
    inp = wl.inputs.copy()
    fr = L.in_friction(h)
    inp[:n // 3, fr:fr + 4] = -0.4
    return wl, inp


def kkt_certificate(P, q, cone, l, u, x, active_tol=1e-7):
    """Optimality of x for  min 1/2 x'Px + q'x  s.t.  l <= A x <= u  (A = blockdiag of the 5 x 3 cone block), checked from the KKT conditions
    alone -- no second solver involved: returns (primal violation relative to max(1, |bound|), stationarity residual relative to |q|_inf)
    where the multipliers are the best sign-correct ones (non-negative least squares per foot over the rows that sit on a bound).
    For a strictly convex QP both ~ 0 certify x as THE optimum (what the reference's qpOASES branch returns, mpc_osqp.cc:797-947)."""
    from scipy.optimize import nnls
    nf = len(q) // 3
    g = P @ x + q
    pv, sr = 0.0, 0.0
    for f in range(nf):
        xf, lf, uf = x[3 * f:3 * f + 3], l[5 * f:5 * f + 5], u[5 * f:5 * f + 5]
        s = cone @ xf
        sc = np.maximum(1.0, np.maximum(np.abs(lf), np.where(np.abs(uf) < 1e20, np.abs(uf), 0.0)))
        pv = max(pv, float(np.max(np.maximum(lf - s, s - uf) / sc)))
        cols = []
        for r in range(5):
            at_l, at_u = abs(s[r] - lf[r]) <= active_tol * sc[r], abs(uf[r] - s[r]) <= active_tol * sc[r]
            if at_l:
                cols.append(-cone[r])        # y_r <= 0: A'y contributes -w a_r, w >= 0
            if at_u:
                cols.append(cone[r])
        gf = g[3 * f:3 * f + 3]
        if cols:
            _, rn = nnls(np.array(cols).T, -gf)
        else:
            rn = float(np.linalg.norm(gf))
        sr = max(sr, rn)
    return pv, sr / max(float(np.abs(q).max()), 1e-30)
