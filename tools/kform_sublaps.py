"""Sub-laps of the factorisation set-up (the section profile's K-form slot) of the h = 10 solve jobs: mean shader cycles per robot of profile slots
1 .. 6 on the third and fourth warm step of tools/section_profile.py's sequence -- all robots, and the robots with exactly one ADMM factorisation
and a polish (nfact == 2), whose slots hold ONE factorisation each.

  tools/build_variant.sh p10 -DMPC_SECTION_PROFILE -DMPC_PROFILE_SUB=10      # the ADMM job's factorisations (mpc_wrench.h factor / factor_core / factor_tail)
  MPC_LIB_PATH=.../variants/libmpc_batch_p10.so python tools/kform_sublaps.py Sinv,zf+allsum,step_factor,Gf,dl,tile
  tools/build_variant.sh p11 -DMPC_SECTION_PROFILE -DMPC_PROFILE_SUB=11      # the polish job's (polish_factor / factor_tail)
  MPC_LIB_PATH=.../variants/libmpc_batch_p11.so python tools/kform_sublaps.py polish-setup,Ff+lengths,orth_col,Gf+L,dl,tile
(profiles/kform_sublaps_*.txt)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import rl_mpc_locomotion_amd  # noqa
from rl_mpc_locomotion_amd.batched import BatchedConvexMpc
from rl_mpc_locomotion_amd.synthetic import make_solver_workload, perturb_workload
names = sys.argv[1].split(",")
n, h = 4096, 10
wl = make_solver_workload(n, h=h, seed=1000, config=2)
inertia9 = np.zeros((n, 9)); inertia9[:, 0], inertia9[:, 4], inertia9[:, 8] = wl.inertia_diag.T
sv = BatchedConvexMpc(wl.mass, inertia9, h, wl.dt_mpc, wl.alpha)
w = wl
for step in range(4):
    f, info = sv.solve(torch.from_numpy(w.inputs).cuda()); torch.cuda.synchronize()
    p = np.abs(sv.get_profile()).astype(np.float64); i = info.cpu().numpy()
    w = perturb_workload(w, 7000 + step)
    if step < 2: continue
    one = (i[:, 4] == 2) & (i[:, 2] != 0)
    print(f"step {step}: nfact {i[:,4].mean():.3f}, robots with nfact == 2 and a polish: {one.sum()}")
    print("   all robots      : " + " ".join(f"{nm}={p[:,k+1].mean():.0f}" for k, nm in enumerate(names)) + f" | sum {p[:,1:7].sum(1).mean():.0f}")
    print("   nfact == 2 only : " + " ".join(f"{nm}={p[one,k+1].mean():.0f}" for k, nm in enumerate(names)) + f" | sum {p[one,1:7].sum(1).mean():.0f}")
