"""Golden fixture for the domain randomisation's noise (rl_mpc_locomotion_amd.domain_rand, csrc/domain_rand.h): the reference's OWN
`VecTask.apply_randomizations` (RL_Environment/tasks/base/vec_task.py:491-599), taken from the source file by AST and executed unmodified on a
stand-in object.  Isaac Gym is not installed, so `gym.get_frame_count` is a stub that returns the frame count the case is at, the property maps
and `check_buckets` are empty stubs, `actor_params` is an empty dictionary, and `torch.randn_like` / `torch.rand_like` hand out draws that are
recorded beside the lambda's output.

    python tests/golden/make_golden_domain_rand.py        (build container only: needs /root/reference)

Only arrays are stored.  domain_rand.npz holds, for every case (2 distributions x 2 operations x {no schedule, linear, constant} x frequency 1, 7):
  case_*        the case's settings (distribution, operation, schedule, frequency as parallel arrays), `range`, `range_correlated`, SCHEDULE_STEPS
  frames        the frame counts apply_randomizations was called at, in order
  params        [cases, frames, 4] float64: the lambda's parameters after each call, in the reference's order (mu, var, mu_corr, var_corr or
                lo, hi, lo_corr, hi_corr)
  x             the one 16 x 48 float32 tensor (with signed zeros, NaN, the infinities and values beyond the clip in it)
  at            the two positions in `frames` after which the lambda was called on x
  zc, d, out    [cases, 2, 16, 48] float32: the correlated draw the lambda kept, the per-call draw it was handed, and what it returned
  clamped       torch.clamp(out, -CLIP, CLIP), the line that follows the lambda in VecTask.step (:337)"""
import ast
import operator
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = "/root/reference/RL_Environment/tasks/base/vec_task.py"

SCHEDULE_STEPS = 100
FRAMES = (0, 1, 6, 7, 50, SCHEDULE_STEPS - 1, SCHEDULE_STEPS, SCHEDULE_STEPS + 1)
AT = (4, 7)                                    # the lambda runs after the calls at frame 50 and at frame SCHEDULE_STEPS + 1
RANGE = {"gaussian": ([0.02, 0.3], [0.01, 0.1]), "uniform": ([-0.3, 0.5], [-0.05, 0.15])}
CLIP = 5.0
ROWS, COLS = 16, 48


def reference_method():
    ns = dict(torch=torch, operator=operator, np=np, get_property_setter_map=lambda gym: {}, get_default_setter_args=lambda gym: {},
              get_property_getter_map=lambda gym: {}, check_buckets=lambda gym, envs, dr_params: None)
    tree = ast.parse(open(VEC).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VecTask"][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "apply_randomizations"]
    assert len(fn) == 1
    exec(compile(ast.Module(body=fn, type_ignores=[]), VEC, "exec"), ns)
    return ns["apply_randomizations"]


class Draws:
    """torch.randn_like / rand_like replaced: every draw comes from this generator and is kept."""
    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)
        self.last = {}

    def randn_like(self, t):
        self.last["randn"] = torch.randn(t.shape, generator=self.gen, dtype=t.dtype)
        return self.last["randn"]

    def rand_like(self, t):
        self.last["rand"] = torch.rand(t.shape, generator=self.gen, dtype=t.dtype)
        return self.last["rand"]


def stand_in(frame):
    t = types.SimpleNamespace()
    t.gym = types.SimpleNamespace(get_frame_count=lambda sim: frame["count"])
    t.sim, t.envs, t.num_envs = None, [], ROWS
    t.first_randomization, t.last_step, t.last_rand_step = True, -1, -1          # vec_task.py:218-224
    t.dr_randomizations, t.original_props, t.actor_params_generator, t.extern_actor_params = {}, {}, None, {}
    t.randomize_buf = torch.zeros(ROWS, dtype=torch.long)
    t.reset_buf = torch.ones(ROWS, dtype=torch.long)
    return t


def main():
    apply_randomizations = reference_method()
    rng = np.random.default_rng(41)
    x = (rng.standard_normal((ROWS, COLS)) * rng.choice([0.01, 1.0, 4.0, 30.0], (ROWS, COLS))).astype(np.float32)
    x[0, :9] = [0.0, -0.0, np.nan, np.inf, -np.inf, CLIP, -CLIP, 5.5, -7.25]
    x[9, 40:] = [np.nan, -0.0, 0.0, 1e-30, 3e38, -3e38, np.inf, 4.9999995]
    xt = torch.from_numpy(x)
    names = {"gaussian": ("mu", "var", "mu_corr", "var_corr"), "uniform": ("lo", "hi", "lo_corr", "hi_corr")}
    cases, params, zcs, ds, outs, clamped = [], [], [], [], [], []
    real = torch.randn_like, torch.rand_like
    try:
        for dist in ("gaussian", "uniform"):
            for op in ("additive", "scaling"):
                for sched in ("none", "linear", "constant"):
                    for freq in (1, 7):
                        draws = Draws(1000 + len(cases))
                        torch.randn_like, torch.rand_like = draws.randn_like, draws.rand_like
                        entry = {"distribution": dist, "operation": op, "range": list(RANGE[dist][0]), "range_correlated": list(RANGE[dist][1])}
                        if sched != "none":
                            entry.update(schedule=sched, schedule_steps=SCHEDULE_STEPS)
                        dr_params = {"frequency": freq, "observations": entry, "actor_params": {}}
                        frame = {"count": 0}
                        t = stand_in(frame)
                        p_case, z_case, d_case, o_case, c_case = [], [], [], [], []
                        for k, count in enumerate(FRAMES):
                            frame["count"] = count
                            apply_randomizations(t, dr_params)
                            cur = t.dr_randomizations["observations"]
                            p_case.append([float(cur[nm]) for nm in names[dist]])
                            if k in AT:
                                out = cur["noise_lambda"](xt)
                                assert out.dtype == torch.float32
                                z_case.append(cur["corr"].numpy().copy())
                                d_case.append(draws.last["randn" if dist == "gaussian" else "rand"].numpy().copy())
                                o_case.append(out.numpy().copy())
                                c_case.append(torch.clamp(out, -CLIP, CLIP).numpy().copy())
                        assert entry["range"] == list(RANGE[dist][0])          # the reference scales local copies
                        cases.append((dist, op, sched, freq))
                        params.append(p_case); zcs.append(z_case); ds.append(d_case); outs.append(o_case); clamped.append(c_case)
    finally:
        torch.randn_like, torch.rand_like = real
    out = dict(case_distribution=np.array([c[0] for c in cases]), case_operation=np.array([c[1] for c in cases]),
               case_schedule=np.array([c[2] for c in cases]), case_frequency=np.array([c[3] for c in cases], np.int64),
               range_gaussian=np.array(RANGE["gaussian"]), range_uniform=np.array(RANGE["uniform"]), schedule_steps=np.int64(SCHEDULE_STEPS),
               frames=np.array(FRAMES, np.int64), at=np.array(AT, np.int64), clip=np.float64(CLIP), params=np.array(params, np.float64), x=x,
               zc=np.array(zcs, np.float32), d=np.array(ds, np.float32), out=np.array(outs, np.float32), clamped=np.array(clamped, np.float32))
    assert out["params"].shape == (24, len(FRAMES), 4) and out["out"].shape == (24, 2, ROWS, COLS)
    path = os.path.join(HERE, "domain_rand.npz")
    np.savez_compressed(path, **out)
    print(f"domain_rand: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
