"""What the *_rate.py tools share: HIP events and the percentiles of their spans, the stage timer over BatchedRLTask.step's marks, the
alternating-blocks wall-clock loop, legged_gym's terrain grid with a set of origins, the head and the tail of a JSON record, and the speed
verdict over closed_loop_rate.py --variants runs of a parent's library and a change's (also the command at the foot of this file)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12           # MI355X, HBM3E spec


def ev():
    import torch
    return torch.cuda.Event(enable_timing=True)


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()), "p10_ms": float(np.percentile(x, 10)),
            "p90_ms": float(np.percentile(x, 90)), "samples": int(x.size)}


def med(x):
    return float(np.median(x))


def spread(x):
    return {"median_ms": med(x), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def stage_times(task, actions, ticks, event=ev, synchronize=None):
    """{stage: ms per tick} of ``task.step(actions, mark=...)`` over 2 x ``ticks`` ticks: one event before each step and one at each mark, one
    synchronise at the end.  A stage's time is the span from the event before it (the previous mark's, or the one before the step) to its own;
    a stage that some ticks leave out has as many entries as the ticks on which it ran."""
    events = []                          # (stage, or None for the one before a step; its event), in the order they were recorded

    def mark(stage):
        e = event()
        e.record()
        events.append((stage, e))
    for _ in range(2 * ticks):
        mark(None)
        task.step(actions, mark=mark)
    if synchronize is None:
        import torch
        synchronize = torch.cuda.synchronize
    synchronize()
    spans = {}
    for (_, before), (stage, at) in zip(events, events[1:]):
        if stage is not None:
            spans.setdefault(stage, []).append(before.elapsed_time(at))
    return {stage: np.array(ms) for stage, ms in spans.items()}


def wall_blocks(loops, ticks, blocks, robots, warmup=20, per_block=False):
    """``loops`` {name: a function that runs one tick}: ``warmup`` ticks each (cold solves, code objects, torch's kernels), then ``blocks`` blocks
    of ``ticks`` ticks that end in a synchronise, the loops alternating block by block.  {name: the host clock's record, ms per tick}; with
    ``per_block`` a record also keeps its blocks' own values (``ms_per_tick_blocks``), for differences block by block."""
    import torch
    for tick in loops.values():
        for _ in range(warmup):
            tick()
    torch.cuda.synchronize()
    wall = {k: [] for k in loops}
    for _ in range(blocks):
        for name, tick in loops.items():
            t0 = time.perf_counter()
            for _ in range(ticks):
                tick()
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    out = {}
    for name, w in wall.items():
        per = np.array(w) / ticks * 1e3
        out[name] = {"ms_per_tick_median": med(per), "ms_per_tick_p10": float(np.percentile(per, 10)), "ms_per_tick_p90": float(np.percentile(per, 90)),
                     "ms_per_tick_min": float(per.min()), "ms_per_tick_max": float(per.max()), "robot_ticks_per_s": robots * ticks / med(w)}
        if per_block:
            out[name]["ms_per_tick_blocks"] = per.tolist()
    return out


def terrain_grid(n, max_init_level, dev, episode_length_s):
    """legged_gym's 10 x 20 grid of 8 m tiles, a function that makes a fresh curriculum on it for ``n`` environments (its ``origins0`` are the
    origins of a task without one), and the grid's entry of a record."""
    from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
    from rl_mpc_locomotion_amd.terrain import TerrainGrid
    grid = TerrainGrid(num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, seed=0)

    def curriculum(level=max_init_level, length_s=episode_length_s):
        return TerrainCurriculum(grid, n, max_init_level=level, seed=0, device=dev, episode_length_s=length_s)
    return grid, curriculum, {"levels": grid.num_levels, "types": grid.num_types, "tile_m": grid.tile_length, "nodes": [grid.terrain.rows, grid.terrain.cols]}


def header(args, robots, **more):
    """The head of a record: what was built, the sizes, what the mode adds, and the shader clock as bench.py --full records it."""
    from bench import device_state
    from rl_mpc_locomotion_amd import _lib
    return {"kernel_source_sha256": _lib.kernel_source_hash(), "robots": robots, "horizon": 10, "ticks_per_block": args.ticks, "blocks": args.blocks, **more,
            "device_state": {"before": device_state(0)}}


def clock(res, when):
    from bench import device_state
    res["device_state"][when] = device_state(0, smi=False)


def variants_verdict(parent, change):
    """``parent``, ``change``: the records of ``closed_loop_rate.py --variants`` runs with the parent's library and with the change's (one process
    per library, alternating, one session).  Per variant the runs' medians P and C, the bound max(P) + (max(P) - min(P)) -- the parent's own
    run-to-run range in that session is the margin -- and whether median(C) holds it."""
    runs = {"parent": parent, "change": change}
    step = lambda r, name: r["variants_mixed_types"]["step"][name]
    out = {"bound": "median(change) <= max(parent) + (max(parent) - min(parent)), per-run medians of the HIP-event spans around mpc_sim_step [ms]",
           "kernel_source_sha256": change[0]["kernel_source_sha256"], "device_state": {s: [r["device_state"] for r in rs] for s, rs in runs.items()}, "variants": {}}
    for name in parent[0]["variants_mixed_types"]["step"]:
        P, C = ([step(r, name)["median_ms"] for r in rs] for rs in (parent, change))
        bound = max(P) + (max(P) - min(P))
        out["variants"][name] = {"parent_median_ms_per_run": P, "change_median_ms_per_run": C, "median_change_ms": med(C), "bound_ms": bound, "holds": med(C) <= bound,
                                 "fallen_fraction_at_end": {s: [step(r, name)["fallen_fraction_at_end"] for r in rs] for s, rs in runs.items()}}
    return out


def emit(res, out=None):
    print(json.dumps(res, indent=1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":               # python tools/_rate.py OUT.json --parent P1.json P2.json ... --change C1.json C2.json ...
    import argparse
    ap = argparse.ArgumentParser(description="variants_verdict over the records of closed_loop_rate.py --variants runs of two libraries")
    ap.add_argument("out")
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--change", nargs="+", required=True)
    a = ap.parse_args()
    emit(variants_verdict(*([json.load(open(f)) for f in files] for files in (a.parent, a.change))), a.out)
