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


def step_ab(robot_type, dev, terrain, origin, repeats=10, block=50):
    """The plant's step on the plane and on the terrain, alternating repeat by repeat in one process: two closed loops (each sim with its own
    controller, flat_ground=False), `block` ticks of one, then of the other, HIP events around mpc_sim_step alone.  Robots that have fallen are
    frozen and cost nothing, so each side's fallen fraction at the end is reported with its time."""
    n = len(robot_type)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    cmd = torch.tensor(GOLDEN_TROT_CMD, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
    sides = {}
    for name, kw in (("plane", {}), ("terrain", {"terrain": terrain, "origin": origin})):
        sim = BatchedToySim(robot_type, yaw0=yaw, device=dev, **kw)
        ctl = BatchedLocomotion(robot_type, [TROT] * n, horizon=10, flat_ground=False, device=dev)
        sides[name] = (sim, ctl, sim.dof_state.view(n, 12, 2), [])
        for _ in range(10):
            sim.step(ctl.run(sides[name][2], sim.root_states, cmd))
    for _ in range(repeats):
        for name, (sim, ctl, view, ms) in sides.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
            for a, b in ev:
                tau = ctl.run(view, sim.root_states, cmd)
                a.record(); sim.step(tau); b.record()
            torch.cuda.synchronize()
            ms.append([a.elapsed_time(b) for a, b in ev])
    out = {"repeats": repeats, "ticks_per_repeat": block, "robots": n}
    for name, (sim, _, _, ms) in sides.items():
        m = np.array(ms)
        out[name] = {"step_ms_median": float(np.median(m)), "step_ms_p10": float(np.percentile(m, 10)), "step_ms_p90": float(np.percentile(m, 90)),
                     "step_ms_median_per_repeat": [float(x) for x in np.median(m, 1)], "fallen_fraction_at_end": float(sim.flags()[1].float().mean().item())}
    out["terrain_over_plane_median"] = out["terrain"]["step_ms_median"] / out["plane"]["step_ms_median"]
    # the first repeat alone: before robots have had the time to fall on the rougher ground
    out["terrain_over_plane_first_repeat"] = out["terrain"]["step_ms_median_per_repeat"][0] / out["plane"]["step_ms_median_per_repeat"][0]
    return out


def friction_ab(robot_type, dev, mus, ticks, repeats=10, block=50):
    """The plant's step without friction and with a friction record at each of `mus`, alternating block by block in one process: one closed loop a
    side (each sim with its own controller), `block` ticks of one, then of the next, HIP events around mpc_sim_step alone.  Robots that have fallen
    are frozen and cost nothing, so every side reports its fallen share with its time, and the ratio of the first repeat -- before a slippery floor
    has had the time to fell anybody -- stands beside the ratio of the medians.  Then, per mu, a fresh closed loop of `ticks` ticks: the fallen
    share and the mean slip per foot and tick."""
    from rl_mpc_locomotion_amd.friction import Friction
    import _rate                       # (tools/ is the script's directory)
    n = len(robot_type)
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    cmd = torch.tensor(GOLDEN_TROT_CMD, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()

    def side(mu):
        sim = BatchedToySim(robot_type, yaw0=yaw, device=dev)
        fr = None
        if mu is not None:
            fr = Friction(n, mu=mu, device=dev)
            fr.bind(sim)
        return sim, BatchedLocomotion(robot_type, [TROT] * n, horizon=10, flat_ground=True, device=dev), sim.dof_state.view(n, 12, 2), fr
    name_of = lambda mu: "plain" if mu is None else "mu_" + repr(float(mu))
    sides = {name_of(mu): side(mu) + ([],) for mu in [None] + list(mus)}
    for sim, ctl, view, _, _ in sides.values():
        for _ in range(10):
            sim.step(ctl.run(view, sim.root_states, cmd))
    for _ in range(repeats):
        for sim, ctl, view, _, ms in sides.values():
            ev = [(_rate.ev(), _rate.ev()) for _ in range(block)]
            for a, b in ev:
                tau = ctl.run(view, sim.root_states, cmd)
                a.record(); sim.step(tau); b.record()
            torch.cuda.synchronize()
            ms.append([a.elapsed_time(b) for a, b in ev])
    out = {"repeats": repeats, "ticks_per_repeat": block, "robots": n, "step": {}}
    for name, (sim, _, _, _, ms) in sides.items():
        m = np.array(ms)
        out["step"][name] = {**_rate.spread(m), "median_ms_per_repeat": [float(x) for x in np.median(m, 1)],
                             "fallen_fraction_at_end": float(sim.flags()[1].float().mean().item())}
    plain = out["step"]["plain"]
    for name, rec in out["step"].items():
        if name != "plain":
            rec["over_plain_median"] = rec["median_ms"] / plain["median_ms"]
            rec["over_plain_first_repeat"] = rec["median_ms_per_repeat"][0] / plain["median_ms_per_repeat"][0]
    del sides
    out["closed_loop"] = {"ticks": ticks}
    for mu in mus:
        sim, ctl, view, fr = side(mu)
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
    yaw = np.random.default_rng(0).uniform(-np.pi, np.pi, n)
    ground = {} if terrain is None else {"terrain": terrain, "origin": origin}
    sim = BatchedToySim(robot_type, yaw0=yaw, device=dev, **ground)
    ctl = BatchedLocomotion(robot_type, [TROT] * n, horizon=10, flat_ground=flat_ground, device=dev)
    cmd = torch.tensor(GOLDEN_TROT_CMD[:3] if default_weights else GOLDEN_TROT_CMD, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
    view = sim.dof_state.view(n, 12, 2)
    for _ in range(10):            # warm-up (first solves are cold)
        sim.step(ctl.run(view, sim.root_states, cmd))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        sim.step(ctl.run(view, sim.root_states, cmd))
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t0
    _, fell = sim.flags()
    fell = fell.cpu().numpy()
    rt = np.asarray(robot_type)
    out = {"robots": n, "ticks": ticks, "flat_ground": flat_ground, "weights": "robot table defaults" if default_weights else "closed-loop golden trot", "loop_s": loop_s,
           "robot_ticks_per_s": n * ticks / loop_s, "ms_per_tick": loop_s / ticks * 1e3, "fallen_fraction": float(fell.mean()),
           "fallen_fraction_per_robot_type": {int(t): float(fell[rt == t].mean()) for t in np.unique(rt)}}
    if default_weights or terrain is not None or not flat_ground:       # (with --terrain the plant's step is step_ab's)
        return out
    # the plant alone, HIP events around mpc_sim_step inside the same closed loop (a fresh batch: every robot standing at the start)
    sim = BatchedToySim(robot_type, yaw0=yaw, device=dev)
    ctl = BatchedLocomotion(robot_type, [TROT] * n, horizon=10, flat_ground=True, device=dev)
    view = sim.dof_state.view(n, 12, 2)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ticks)]
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
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = "cuda:0"
    n = args.robots
    res = {"kernel_source_sha256": _lib.kernel_source_hash()}
    if args.friction:
        if any(not mu >= 0 for mu in args.friction):
            ap.error("--friction: every MU must be >= 0")
        res["device_state"] = {"before": device_state(0)}
        res["friction_mixed_types"] = friction_ab([i % 3 for i in range(n)], dev, args.friction, args.ticks)
        res["device_state"]["after"] = device_state(0, smi=False)
        print(json.dumps(res, indent=1))
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        sys.exit(0)
    clock0 = None if args.quick else device_state(0)
    mixed = [i % 3 for i in range(n)]
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
