"""Closed-loop rate on the device: BatchedLocomotion.run + BatchedToySim.step for 4096 robots, h = 10 (Aliengo trotting, and the three
robot types mixed), no host round trip per tick.  Reports robot-ticks / s of the whole loop over K ticks, the toy plant's step time from
HIP events (mpc_sim_step alone, 4096 robots), and the fraction of robots fallen after 1000 ticks, with the shader clock as bench.py --full
records it (device_state).  Command: trot at 0.5 m/s with the MPC weights of the closed-loop golden's trot cases (and, for the fallen
fraction only, the robot table's default weights).
    python tools/closed_loop_rate.py [--ticks 1000] [--out profiles/r07_toy_sim.json]
With --terrain reference|mild|zero (one or more) the robots stand on a height field (rl_mpc_locomotion_amd.terrain: the reference's 5 cm random
uniform terrain, the same generator with 1 cm steps, or an all-zero field: the plane's trajectories through the terrain kernel), spread over it on a grid, the controller estimates the ground normal
(flat_ground=False), and the report gains, per terrain and beside the same legs on the plane, the loop rate, the fallen fraction and the
plant's step on the plane and on the terrain measured alternately, repeat by repeat, in one process (HIP events: median, p10, p90).
    python tools/closed_loop_rate.py --terrain reference mild --out profiles/r11_toy_terrain.json
With --friction MU [MU ...] (inf is a value) the plant gets a Coulomb friction record (rl_mpc_locomotion_amd.friction): the friction step at mu = inf
and at each MU is measured against the plain step kernel in the same run, the closed loops alternating block by block (tools/_rate.py's spread of
the HIP-event spans around mpc_sim_step), and per MU the fallen share and the mean slip per foot and tick after --ticks ticks are reported.
    python tools/closed_loop_rate.py --friction inf 0.4 --out profiles/friction_rate.json
With --variants the six step kernels (plane and an all-zero field, each plain, with the neutral plant record and with mu = inf: one trajectory) are
the alternating sides of one process, and nothing else is run: what a change to the kernels' shared shell (csrc/sim_step.h) is measured with.
    python tools/closed_loop_rate.py --variants --out results/variants.json
The kernel-trace stats of the same loop: rocprofv3 --kernel-trace --stats ... -- python tools/closed_loop_rate.py --ticks 50 --quick"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_mpc_locomotion_amd  # noqa: E402,F401
from rl_mpc_locomotion_amd import _lib  # noqa: E402
from rl_mpc_locomotion_amd.locomotion import BatchedLocomotion  # noqa: E402
from rl_mpc_locomotion_amd.terrain import Terrain, spread_origins  # noqa: E402
from rl_mpc_locomotion_amd.toy_sim import BatchedToySim  # noqa: E402
from bench import device_state  # noqa: E402
import _rate  # noqa: E402  (tools/ is the script's directory)

TROT = 0
# the command record of the closed-loop golden's trot cases (tests/golden/closed_loop_h10.npz: vx, vy, wz, then 12 MPC weights and 0).  The
# robot table's default Aliengo weights leave roll and pitch unweighted: in this toy such a robot tips over (the `default_weights` leg).
GOLDEN_TROT_CMD = [0.5, 0.0, 0.0, 5, 5, 5, 50, 50, 50, 1, 1, 1, 1, 1, 1, 0]


def make_terrain(kind, n, seed=0):
    """(Terrain, origins [n,2]) of --terrain `kind`, or (None, None)."""
    if kind == "none":
        return None, None
    if kind == "zero":                 # the plane's trajectories through the terrain kernel: its own cost, without the rough ground's divergence
        t = Terrain(np.zeros((500, 500), np.int16), 0.1, 0.005, -50.0 / 3, -50.0 / 3)
    else:
        t = Terrain.reference(seed) if kind == "reference" else Terrain.mild(seed)
    return t, spread_origins(n, t, margin=3.0)


def side(robot_type, dev, flat_ground=True, mu=None, plant=False, **ground):
    """One closed loop: (sim, controller, dof view, Friction or None).  `ground`: BatchedToySim's terrain and origin; `plant` attaches the neutral
    plant record, `mu` a friction record with that coefficient."""
    n = len(robot_type)
    sim = BatchedToySim(robot_type, yaw0=np.random.default_rng(0).uniform(-np.pi, np.pi, n), device=dev, **ground)
    fr = None
    if plant:
        from rl_mpc_locomotion_amd.plant_rand import PlantRand
        sim._plant_rand = PlantRand(n, device=dev)
        sim._plant_rand.bind(sim)
    if mu is not None:
        from rl_mpc_locomotion_amd.friction import Friction
        fr = Friction(n, mu=mu, device=dev)
        fr.bind(sim)
    return sim, BatchedLocomotion(robot_type, [TROT] * n, horizon=10, flat_ground=flat_ground, device=dev), sim.dof_state.view(n, 12, 2), fr


def trot_cmd(n, dev):
    return torch.tensor(GOLDEN_TROT_CMD, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()


def alternate(sides, repeats=10, block=50):
    """The plant's step of each of `sides` {name: side(...)}, alternating in one process: ten warm-up ticks each, then `repeats` times `block` ticks
    of one closed loop, then of the next, HIP events around mpc_sim_step alone.  Robots that have fallen are frozen and cost nothing, so every side's
    fallen share at the end is reported with its times."""
    sim0 = next(iter(sides.values()))[0]
    cmd, ms = trot_cmd(sim0.n, sim0.device), {name: [] for name in sides}
    for sim, ctl, view, _ in sides.values():
        for _ in range(10):
            sim.step(ctl.run(view, sim.root_states, cmd))
    for _ in range(repeats):
        for name, (sim, ctl, view, _) in sides.items():
            ev = [(_rate.ev(), _rate.ev()) for _ in range(block)]
            for a, b in ev:
                tau = ctl.run(view, sim.root_states, cmd)
                a.record(); sim.step(tau); b.record()
            torch.cuda.synchronize()
            ms[name].append([a.elapsed_time(b) for a, b in ev])
    step = {name: {**_rate.spread(np.array(m)), "median_ms_per_repeat": [float(x) for x in np.median(m, 1)],
                   "fallen_fraction_at_end": float(sides[name][0].flags()[1].float().mean().item())} for name, m in ms.items()}
    return {"repeats": repeats, "ticks_per_repeat": block, "robots": sim0.n, "step": step}


def step_ab(robot_type, dev, terrain, origin):
    """The plant's step on the plane and on the terrain (each sim with its own controller, flat_ground=False), alternating repeat by repeat."""
    out = alternate({"plane": side(robot_type, dev, flat_ground=False), "terrain": side(robot_type, dev, flat_ground=False, terrain=terrain, origin=origin)})
    keys = {"median_ms": "step_ms_median", "p10_ms": "step_ms_p10", "p90_ms": "step_ms_p90", "median_ms_per_repeat": "step_ms_median_per_repeat",
            "fallen_fraction_at_end": "fallen_fraction_at_end"}            # (this record's keys are older than _rate.spread's)
    out.update({name: {keys[k]: v for k, v in rec.items()} for name, rec in out.pop("step").items()})
    out["terrain_over_plane_median"] = out["terrain"]["step_ms_median"] / out["plane"]["step_ms_median"]
    # the first repeat alone: before robots have had the time to fall on the rougher ground
    out["terrain_over_plane_first_repeat"] = out["terrain"]["step_ms_median_per_repeat"][0] / out["plane"]["step_ms_median_per_repeat"][0]
    return out


def variants_ab(robot_type, dev):
    """All six step kernels as sides of one process: the plane and an all-zero field, each plain, with the neutral plant record, and with the
    Coulomb contact at mu = inf -- six loops with one trajectory, so that every side steps the same robots through the same states."""
    terrain, origin = make_terrain("zero", len(robot_type))
    return alternate({f"{ground}_{model}": side(robot_type, dev, **kw, **gkw)
                      for ground, gkw in (("plane", {}), ("field", {"terrain": terrain, "origin": origin}))
                      for model, kw in (("plain", {}), ("plant", {"plant": True}), ("coulomb", {"mu": float("inf")}))})


def friction_ab(robot_type, dev, mus, ticks):
    """The plant's step without friction and with a friction record at each of `mus`, alternating block by block; the ratio of the first repeat --
    before a slippery floor has had the time to fell anybody -- stands beside the ratio of the medians.  Then, per mu, a fresh closed loop of
    `ticks` ticks: the fallen share and the mean slip per foot and tick."""
    n = len(robot_type)
    cmd = trot_cmd(n, dev)
    name_of = lambda mu: "plain" if mu is None else "mu_" + repr(float(mu))
    out = alternate({name_of(mu): side(robot_type, dev, mu=mu) for mu in [None] + list(mus)})
    plain = out["step"]["plain"]
    for name, rec in out["step"].items():
        if name != "plain":
            rec["over_plain_median"] = rec["median_ms"] / plain["median_ms"]
            rec["over_plain_first_repeat"] = rec["median_ms_per_repeat"][0] / plain["median_ms_per_repeat"][0]
    out["closed_loop"] = {"ticks": ticks}
    for mu in mus:
        sim, ctl, view, fr = side(robot_type, dev, mu=mu)
        slip = torch.zeros((), dtype=torch.float64, device=dev)
        slipping = torch.zeros((), dtype=torch.float64, device=dev)
        for _ in range(ticks):
            sim.step(ctl.run(view, sim.root_states, cmd))
            slip += fr.foot_slip.sum()
            slipping += (fr.foot_slip > 0).any(1).sum()
        fell = sim.flags()[1].cpu().numpy()
        rt = np.asarray(robot_type)
        out["closed_loop"][name_of(mu)] = {"fallen_fraction": float(fell.mean()), "fallen_fraction_per_robot_type": {int(t): float(fell[rt == t].mean()) for t in np.unique(rt)},
                                           "mean_slip_m_per_foot_tick": float(slip.item()) / (4 * n * ticks),
                                           "robot_ticks_with_a_slip_fraction": float(slipping.item()) / (n * ticks)}
    return out


def run(robot_type, ticks, dev, default_weights=False, terrain=None, origin=None, flat_ground=True):
    n = len(robot_type)
    sim, ctl, view, _ = side(robot_type, dev, flat_ground, **({} if terrain is None else {"terrain": terrain, "origin": origin}))
    cmd = torch.tensor(GOLDEN_TROT_CMD[:3] if default_weights else GOLDEN_TROT_CMD, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
    for _ in range(10):           # warm-up (first solves are cold)
        sim.step(ctl.run(view, sim.root_states, cmd))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        sim.step(ctl.run(view, sim.root_states, cmd))
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t0
    fell = sim.flags()[1].cpu().numpy()
    rt = np.asarray(robot_type)
    out = {"robots": n, "ticks": ticks, "flat_ground": flat_ground, "weights": "robot table defaults" if default_weights else "closed-loop golden trot", "loop_s": loop_s,
           "robot_ticks_per_s": n * ticks / loop_s, "ms_per_tick": loop_s / ticks * 1e3, "fallen_fraction": float(fell.mean()),
           "fallen_fraction_per_robot_type": {int(t): float(fell[rt == t].mean()) for t in np.unique(rt)}}
    if default_weights or terrain is not None or not flat_ground:       # (with --terrain the plant's step is step_ab's)
        return out
    # the plant alone, HIP events around mpc_sim_step inside the same closed loop (a fresh batch: every robot standing at the start)
    sim, ctl, view, _ = side(robot_type, dev)
    ev = [(_rate.ev(), _rate.ev()) for _ in range(ticks)]
    for a, b in ev:
        tau = ctl.run(view, sim.root_states, cmd)
        a.record(); sim.step(tau); b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    out.update({"sim_step_ms_median": float(np.median(ms)), "sim_step_ms_mean": float(ms.mean()), "sim_step_ms_min": float(ms.min()),
                "sim_step_ms_max": float(ms.max()), "sim_step_events": len(ms)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--quick", action="store_true", help="the mixed-type loop only (for a kernel trace)")
    ap.add_argument("--terrain", nargs="+", choices=["none", "reference", "mild", "zero"], default=["none"],
                    help="height fields to run on beside the plane (the controller then runs with flat_ground=False)")
    ap.add_argument("--terrain-seed", type=int, default=0)
    ap.add_argument("--friction", nargs="+", type=float, metavar="MU",
                    help="friction coefficients (inf is one): the friction step against the plain one, and the fallen share and slip per MU; nothing else is run")
    ap.add_argument("--variants", action="store_true", help="the six step kernels (plane / zero field x plain / neutral plant record / mu = inf) against each other; nothing else is run")
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = "cuda:0"
    n = args.robots
    res = {"kernel_source_sha256": _lib.kernel_source_hash()}
    mixed = [i % 3 for i in range(n)]
    if args.friction or args.variants:
        if any(not mu >= 0 for mu in args.friction or []):
            ap.error("--friction: every MU must be >= 0")
        res["device_state"] = {"before": device_state(0)}
        if args.friction:
            res["friction_mixed_types"] = friction_ab(mixed, dev, args.friction, args.ticks)
        else:
            res["variants_mixed_types"] = variants_ab(mixed, dev)
        _rate.clock(res, "after")
        _rate.emit(res, args.out)
        sys.exit(0)
    clock0 = None if args.quick else device_state(0)
    legs = {"mixed_types": (mixed, False)} if args.quick else {"aliengo": ([0] * n, False), "mixed_types": (mixed, False), "mixed_types_default_weights": (mixed, True)}
    for name, (rt, dw) in legs.items():
        res[name] = run(rt, args.ticks, dev, default_weights=dw)
        print(name, json.dumps(res[name]), flush=True)
    aliengo = [0] * n
    for kind in [k for k in args.terrain if k != "none"]:
        t, origin = make_terrain(kind, n, args.terrain_seed)
        res.setdefault("plane_flat_ground_false", {})
        for name, rt in (("aliengo", aliengo), ("mixed_types", mixed)):
            if name not in res["plane_flat_ground_false"]:
                res["plane_flat_ground_false"][name] = run(rt, args.ticks, dev, flat_ground=False)
                print("plane_flat_ground_false", name, json.dumps(res["plane_flat_ground_false"][name]), flush=True)
        res["terrain_" + kind] = {"field": {"rows": t.rows, "cols": t.cols, "hscale": t.hscale, "vscale": t.vscale, "x0": t.x0, "y0": t.y0,
                                            "seed": args.terrain_seed, "min_units": int(t.heights.min()), "max_units": int(t.heights.max()),
                                            "max_cell_slope": t.max_cell_slope()}}
        for name, rt in (("aliengo", aliengo), ("mixed_types", mixed)):
            leg = run(rt, args.ticks, dev, terrain=t, origin=origin, flat_ground=False)
            leg["step_plane_vs_terrain"] = step_ab(rt, dev, t, origin)
            res["terrain_" + kind][name] = leg
            print("terrain_" + kind, name, json.dumps(leg), flush=True)
    if clock0 is not None:
        res["device_state"] = {"before": clock0, "after": device_state(0, smi=False)}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
