"""Prep and solve kernel times of the exact mode without and with its seed from the float32 working-set search (tuning hook
MPC_EXACT_F32_SEED=1, mpc_exact32.h) on seeded sequences of 4096 robots, h = 10 / 16 / 20 (BASELINE configs 2 / 4 / 5): the fp64 method's
passes, robots left to the ADMM route, and the largest force difference between the two runs.
    python tools/exact_f32_rate.py [--out profiles/r07_exact_f32.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rl_mpc_locomotion_amd  # noqa: E402,F401
from rl_mpc_locomotion_amd.batched import BatchedConvexMpc  # noqa: E402
from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload  # noqa: E402


def run(h, cfg, n=4096, warm=3, steps=8):
    wl = make_solver_workload(n, h=h, seed=1000, config=cfg)
    inertia9 = np.zeros((n, 9)); inertia9[:, 0], inertia9[:, 4], inertia9[:, 8] = wl.inertia_diag.T
    out, forces = {}, {}
    for mode in ("exact", "exact_f32_seed"):
        os.environ["MPC_EXACT_F32_SEED"] = "1" if mode == "exact_f32_seed" else "0"     # (read when the batch is created)
        s = BatchedConvexMpc(wl.mass, inertia9, h, wl.dt_mpc, wl.alpha, solver="exact")
        s.enable_timing()
        w, fs, passes = wl, [], []
        for k in range(warm + steps):
            f, info = s.solve(torch.from_numpy(w.inputs).cuda())
            torch.cuda.synchronize()
            fs.append(f.cpu().numpy().copy())
            ii = info.cpu().numpy()
            passes.append(float(ii[:, 0].mean()))
            w = perturb_workload(w, 7000 + 131 * k)
        a, c = s.kernel_times(steps)
        out[mode] = {"prep_ms": float(np.mean(a)), "solve_ms": float(np.mean(c)), "solve_ms_min": float(np.min(c)),
                     "passes_mean_cold": passes[0], "passes_mean_seeded": float(np.mean(passes[warm:])),
                     "unsolved_last": int((ii[:, 1] != 1).sum())}
        forces[mode] = np.stack(fs)
    fe, f3 = forces["exact"], forces["exact_f32_seed"]
    out["max_rel_diff_between_modes"] = float((np.abs(fe - f3).max(-1) / np.maximum(np.abs(fe).max(-1), 1.0)).max())
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {}
    for h, cfg in ((10, 2), (16, 4), (20, 5)):
        res[f"h{h}_cfg{cfg}"] = run(h, cfg)
        print(f"h={h} cfg={cfg}", json.dumps(res[f"h{h}_cfg{cfg}"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
