"""Cases and fixtures of the prep kernel's phase tests (tests/test_prep_phases_emu.py, tests/test_prep_records_gpu.py).

The fixtures pin what the prep kernel (assembly + Ruiz scaling) and the solve behind it computed BEFORE its phases were regrouped; they
are minted from a checkout of that parent commit and then only ever compared against:

  python tools/mint_prep_fixtures.py emu --tree PARENT_CHECKOUT      -> tests/golden/prep_phases_emu_parent.npz   (host emulation, no GPU)
  MPC_LIB_PATH=PARENT_LIBRARY python tools/mint_prep_fixtures.py gpu -> tests/golden/prep_records_gpu_parent.npz  (on the GPU)

What is stored: forces and info in full; of every record (state; on the GPU also the QP and the scale record) a 64-bit BLAKE2 digest of
its bytes per robot and call -- the comparison is for bit equality, which a digest decides as well as the bytes do, and the records
of six horizons, three calls and three input types would be 9 MB."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HORIZONS = (2, 3, 10, 12, 16, 20)      # 2, 3: the set-up scratch overlaps the arrays it feeds and the H - 1 loops are shortest
CALLS = 3                               # one cold, two warm


def digest(rows):
    """uint64 [n]: BLAKE2b-64 of the bytes of every row."""
    rows = np.ascontiguousarray(rows)
    return np.array([int.from_bytes(hashlib.blake2b(r.tobytes(), digest_size=8).digest(), "little") for r in rows], dtype=np.uint64)


def mask_qp_padding(rows, h):
    """The QP record with its three padding doubles (behind the cone block's 15 entries and th2's 6) zeroed: no kernel writes them, they hold
    whatever the allocation held."""
    rows = np.array(rows)
    cone = 12 * h + 2 * 20 * h
    rows[:, [cone + 15, cone + 16 + 72 + 36 + 6, cone + 16 + 72 + 36 + 7]] = 0.0
    return rows


def cases(h, n, seed=0):
    """[CALLS] workloads of n robots: the three robot types and the three gaits mixed (configuration 3), robot 1's second planning step with
    all four feet in swing in every call, and the last robot with a NaN velocity in the second call -- the solve reports NON_CVX and the
    third call restarts cold."""
    sys.path.insert(0, ROOT)
    import rl_mpc_locomotion_amd  # noqa: F401
    from rl_mpc_locomotion_amd import layout as L
    from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload
    wl = make_solver_workload(n, h=h, seed=100 + h + seed, config=3)
    out = []
    for call in range(CALLS):
        rec = wl.inputs.copy()
        rec[1, L.IN_CONTACT + 4 * (1 % h):L.IN_CONTACT + 4 * (1 % h) + 4] = 0.0
        if call == 1:
            rec[n - 1, L.IN_COM_VEL] = np.nan
        out.append((wl, rec))
        wl = perturb_workload(wl, 7 * h + call + seed)
    return out


def run_emu(tree, h, n=5, reverse=False, poison=False):
    """{name: array} of the three calls on the host emulation built from `tree`."""
    sys.path.insert(0, tree)
    from tests.emu import emu
    emu.lib().emu_set_poison(int(poison))
    cs = cases(h, n)
    wl0 = cs[0][0]
    eb = emu.EmuBatch(wl0.mass, wl0.inertia_diag, h, wl0.dt_mpc, wl0.alpha)
    out = {}
    for call, (_, rec) in enumerate(cs):
        f = eb.solve(rec, reverse=reverse)
        out[f"h{h}_c{call}_forces"] = f.copy()
        out[f"h{h}_c{call}_info"] = eb.info.copy()
        out[f"h{h}_c{call}_state"] = digest(eb.state)
    emu.lib().emu_set_poison(0)
    return out


GPU_DTYPES = ("float32", "float64", "float16")


def run_gpu(h, n=7):
    """{name: array} of the three calls through BatchedConvexMpc, once per input type the API accepts."""
    import torch
    sys.path.insert(0, ROOT)
    from rl_mpc_locomotion_amd.batched import BatchedConvexMpc
    cs = cases(h, n)
    wl0 = cs[0][0]
    inertia9 = np.zeros((n, 9))
    inertia9[:, 0], inertia9[:, 4], inertia9[:, 8] = wl0.inertia_diag[:, 0], wl0.inertia_diag[:, 1], wl0.inertia_diag[:, 2]
    out = {}
    for dt in GPU_DTYPES:
        gpu = BatchedConvexMpc(wl0.mass, inertia9, h, wl0.dt_mpc, wl0.alpha, device="cuda:0")
        for call, (_, rec) in enumerate(cs):
            f, info = gpu.solve(torch.from_numpy(rec).to("cuda:0").to(getattr(torch, dt)).contiguous())
            torch.cuda.synchronize()
            key = f"h{h}_{dt}_c{call}_"
            out[key + "forces"] = f.cpu().numpy().copy()
            out[key + "info"] = info.cpu().numpy().copy()
            for name, rows in (("qp", gpu.get_qp()), ("scale", gpu.get_scale()), ("state", gpu.get_state())):
                rows = np.array(rows.cpu().numpy() if hasattr(rows, "cpu") else rows)
                out[key + name] = digest(mask_qp_padding(rows, h) if name == "qp" else rows)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("emu", "gpu"))
    ap.add_argument("--tree", default=ROOT, help="emu: the checkout whose tests/emu is built and run (the parent commit's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    data = {}
    for h in HORIZONS:
        data.update(run_emu(os.path.abspath(a.tree), h) if a.what == "emu" else run_gpu(h))
    out = a.out or os.path.join(GOLDEN, "prep_phases_emu_parent.npz" if a.what == "emu" else "prep_records_gpu_parent.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
