"""The prep kernel's records on the GPU after its phases were regrouped (mpc_core.h Assembler::run, Scaler::scale).

(a) The bits did not move: QP record, scale record, state record, forces and info of six horizons, seven robots, one cold and two warm
    calls and every input type the API accepts equal what the parent commit's library computed (tests/golden/prep_records_gpu_parent.npz,
    tools/mint_prep_fixtures.py: forces and info in full, the records as 64-bit digests of their bytes).
(b) No race: between two workgroup barriers the first wavefront's chain runs unordered against the other wavefronts, which the host
    emulation cannot see.  768 distinct robots in one launch put three workgroups at different phases on every CU; the same robots in launches of
    three run with a CU to themselves.  Every record of every robot must be the same bits either way, cold and warm."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mint_prep_fixtures as mint  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "prep_records_gpu_parent.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("h", mint.HORIZONS)
def test_records_equal_the_parent(h, golden):
    res = mint.run_gpu(h)
    keys = [k for k in golden if k.startswith(f"h{h}_")]
    assert len(keys) == 5 * mint.CALLS * len(mint.GPU_DTYPES) and set(keys) == set(res)
    bad = [k for k in keys if res[k].shape != golden[k].shape or res[k].dtype != golden[k].dtype or res[k].tobytes() != golden[k].tobytes()]
    assert not bad, bad


def test_crowded_and_lonely_workgroups_agree():
    import torch
    from rl_mpc_locomotion_amd.batched import BatchedConvexMpc
    from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload
    h, n = 10, 768
    wl = make_solver_workload(n, h=h, seed=4242, config=3)      # (robot type = index mod 3: every group of three has the same three models)
    calls = [wl.inputs, perturb_workload(wl, 4243).inputs]
    assert len(np.unique(calls[0], axis=0)) == n

    def inertia9(k):
        out = np.zeros((k, 9))
        out[:, 0], out[:, 4], out[:, 8] = wl.inertia_diag[:k, 0], wl.inertia_diag[:k, 1], wl.inertia_diag[:k, 2]
        return out

    def records(gpu, rec):
        f, info = gpu.solve(torch.from_numpy(np.ascontiguousarray(rec)).to("cuda:0"))
        torch.cuda.synchronize()
        return [mint.mask_qp_padding(gpu.get_qp(), h), gpu.get_scale(), gpu.get_state(), f.cpu().numpy(), info.cpu().numpy()]

    big = BatchedConvexMpc(wl.mass, inertia9(n), h, wl.dt_mpc, wl.alpha, device="cuda:0")
    crowded = [records(big, rec) for rec in calls]
    small = BatchedConvexMpc(wl.mass[:3], inertia9(3), h, wl.dt_mpc, wl.alpha, device="cuda:0")
    names = ("qp", "scale", "state", "forces", "info")
    bad = []
    for g in range(n // 3):
        small.reset()
        small.forces.zero_()      # (a robot that is not SOLVED keeps its previous forces: the group's, not its predecessor's)
        for c, rec in enumerate(calls):
            lonely = records(small, rec[3 * g:3 * g + 3])
            for name, a, b in zip(names, lonely, crowded[c]):
                if a.tobytes() != np.ascontiguousarray(b[3 * g:3 * g + 3]).tobytes():
                    bad.append((g, "cold" if c == 0 else "warm", name))
    assert not bad, bad[:20]
    assert (crowded[0][4][:, 5] == 1).all() and (crowded[1][4][:, 5] == 0).all()      # (one cold call, one warm)
