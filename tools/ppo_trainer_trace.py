"""What PPOTrainer computes, as hashes: the proof that a change of the trainer's host code changes no number.

    python tools/ppo_trainer_trace.py --out trace.json                                   # every configuration below, on the GPU
    python tools/ppo_trainer_trace.py --compare parent1.json parent2.json change.json --out verdict.json      # host only

For each configuration -- plain / torch, plain / hip, normalised + privileged / torch and / hip, every option at once with the hip update and with a
recurrent actor-critic whose update through time runs on the device, recurrent with the torch update through time, and a save -> load into a fresh
trainer -> learn(1) -- on 64 environments (robot types cycling, trot, horizon 10, episodes of 3 ticks, 4 ticks per collection, one epoch of two
mini-batches, nets (64, 32) / (32,)) and 2 iterations: ``infos``, a SHA-256 of every tensor in the checkpoint, and a SHA-256 of every RolloutStorage tensor
after the first and after the last collection.  The file uses nothing of the trainer but its public members, so it runs on an older tree as it is.

``--compare`` takes two runs of the parent and one of the change.  ``storage_first`` must be bitwise the parent's, unconditionally.  Every other field must
be bitwise the parent's wherever the parent's two runs equal each other; where they do not (an update that is not run-to-run reproducible), a float entry of
``infos`` must lie within four times the parent's own largest run-to-run difference for that entry (two samples are a thin estimate of the spread) and a
tensor's hash is listed as not comparable.  ``--brief`` keeps of the three runs only what they were runs of (the kernel sources' hash, torch's version) beside
the verdict, not their records: a file small enough to commit."""
import argparse
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, TROT = 64, 0
CONFIGS = ("plain_torch", "plain_hip", "normalised_privileged_torch", "normalised_privileged_hip", "all_options_hip", "all_options_recurrent_hip_through_time",
           "recurrent_torch_through_time", "save_load_learn")
STORAGE = ("observations", "privileged_observations", "actions", "mu", "sigma", "values", "rewards", "dones", "actions_log_prob", "returns", "advantages",
           "saved_h_a", "saved_c_a", "saved_h_c", "saved_c_c")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def tensor_hashes(x, path=""):
    """{path: sha256} of every tensor in a nest of dicts, lists and tuples."""
    import torch
    if isinstance(x, torch.Tensor):
        return {path: sha(x)}
    items = x.items() if isinstance(x, dict) else enumerate(x) if isinstance(x, (list, tuple)) else ()
    out = {}
    for k, v in items:
        out.update(tensor_hashes(v, f"{path}/{k}"))
    return out


def make_task(options, dev):
    import numpy as np
    from rl_mpc_locomotion_amd import rl_task as R
    cfg = R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), episode_length_s=0.03, seed=4)
    kw = dict(cfg=cfg, horizon=10, device=dev, yaw0=np.random.default_rng(6).uniform(-np.pi, np.pi, N))
    if options == "plain":
        kw.update(flat_ground=True)
    elif options == "privileged":
        from rl_mpc_locomotion_amd import privileged_obs as V
        kw.update(flat_ground=True, privileged_obs=V.PrivilegedObs(N, device=dev))
    else:                                                                        # every option of the task at once
        from rl_mpc_locomotion_amd import curriculum as K, domain_rand as DR, episode_terms as E, height_scan as HS, plant_rand as PR, privileged_obs as V, terrain as TR
        slope = lambda d, r, c, hs, vs, s: TR.pyramid_sloped_terrain(r, c, hs, vs, 0.1 + 0.2 * d, platform_size=1.5)
        stairs = lambda d, r, c, hs, vs, s: TR.pyramid_stairs_terrain(r, c, hs, vs, 0.31, 0.03 + 0.04 * d, platform_size=2.0)
        grid = TR.TerrainGrid(3, 2, 4.0, 4.0, hscale=0.1, vscale=0.005, border_size=1.0, generators=[slope, stairs])
        scan = HS.HeightScan(N, device=dev)
        kw.update(height_scan=scan, privileged_obs=V.PrivilegedObs(N, device=dev, plant=True),
                  curriculum=K.TerrainCurriculum(grid, N, max_init_level=1, seed=2, device=dev, env_length=0.0002, episode_length_s=cfg.episode_length_s),
                  episode_terms=E.EpisodeTerms(N, cfg, device=dev,
                                               command_curriculum=E.CommandCurriculumSpec(1.5, x_range0=(-0.5, 0.5), step=0.5, threshold=0.0, update_every=1)),
                  domain_rand=DR.DomainRand(N, observations=DR.NoiseSpec.legged_gym(cfg, height_scan=scan), actions=DR.NoiseSpec("gaussian", "additive", (0.0, 0.05)),
                                            push=DR.PushSpec(interval_s=0.02, max_vel_xy=0.5), seed=9, device=dev),
                  plant_rand=PR.PlantRand(N, PR.PlantSpec(payload=(-1.0, 3.0), strength=(0.9, 1.1), gravity=(-1.0, 1.0), resample="reset"), seed=21, device=dev))
    return R.BatchedRLTask([i % 3 for i in range(N)], [TROT] * N, **kw)


def make_trainer(name, dev, seed=3):
    from rl_mpc_locomotion_amd import ppo as P
    from rl_mpc_locomotion_amd.recurrent import RecurrentConfig
    cfg = P.PPOConfig(num_steps_per_env=4, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,))
    options = "plain" if name.startswith(("plain", "recurrent")) else "privileged" if name.startswith("normalised") else "all"
    how = dict(update="hip" if name.endswith("_hip") or name == "save_load_learn" else "torch", normalize_obs=options != "plain")
    if "recurrent" in name:
        how.update(update="torch", recurrent=RecurrentConfig(hidden_size=32, update_through_time="hip" if "hip_through_time" in name else "torch"))
    return P.PPOTrainer(make_task(options, dev), cfg, seed=seed, **how)


def trace(trainer, iterations):
    """``learn(iterations)`` with the storage hashed after every collection, then the checkpoint as ``save`` writes it."""
    import torch
    collections, collect = [], trainer.collect

    def traced(*a, **kw):
        collect(*a, **kw)
        collections.append({k: sha(getattr(trainer.storage, k)) for k in STORAGE if getattr(trainer.storage, k, None) is not None})
    trainer.collect = traced
    infos = trainer.learn(iterations)
    trainer.collect = collect
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ck.pt")
        trainer.save(path)
        ck = torch.load(path, map_location="cpu")
    return dict(infos=infos, checkpoint_keys=sorted(ck), checkpoint=tensor_hashes(ck), storage_first=collections[0], storage_last=collections[-1])


def run(name, dev):
    import torch
    trainer = make_trainer(name, dev)
    if name != "save_load_learn":
        return trace(trainer, 2)
    trainer.learn(2)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ck.pt")
        trainer.save(path)
        fresh = make_trainer(name, dev, seed=4)
        fresh.load(path)
    torch.manual_seed(5)                                                          # (the fresh trainer's own seed drew its initial weights: the update's randperm from a known state)
    return trace(fresh, 1)


# ---- the comparison (host only) -----------------------------------------------------------------------------------------------------------------
def leaves(x, path=""):
    """{path: value} of the numbers and strings in a nest."""
    if isinstance(x, dict):
        items = x.items()
    elif isinstance(x, list):
        items = enumerate(x)
    else:
        return {path: x}
    out = {}
    for k, v in items:
        out.update(leaves(v, f"{path}/{k}"))
    return out


def entry(path):
    """``/1/episode_terms/rew_torque`` -> ``episode_terms/rew_torque``: an entry of ``infos`` without its iteration."""
    return path.split("/", 2)[2]


def compare(p1, p2, ch):
    verdicts, ok = {}, True
    for name in p1["configurations"]:
        a, b, c = (r["configurations"][name] for r in (p1, p2, ch))
        v = {}
        for field in ("storage_first", "checkpoint_keys", "storage_last", "checkpoint", "infos"):
            la, lb, lc = leaves(a[field]), leaves(b[field]), leaves(c[field])
            if la.keys() != lc.keys() or la.keys() != lb.keys():
                v[field] = "DIFFERS: other entries"
            elif la == lb or field == "storage_first":
                v[field] = "bitwise equal to the parent" if la == lc and la == lb else "DIFFERS: " + ", ".join(k for k in la if la[k] != lc[k] or la[k] != lb[k])
            elif field != "infos":
                unstable = [k for k in la if la[k] != lb[k]]
                stable_differ = [k for k in la if la[k] == lb[k] and la[k] != lc[k]]
                v[field] = {"parent_runs_differ_not_comparable": unstable,
                            "rest": "bitwise equal to the parent" if not stable_differ else "DIFFERS: " + ", ".join(stable_differ)}
            else:                                                               # per entry: the parent's largest run-to-run difference over the iterations
                spread, distance, wrong = {}, {}, [k for k in la if la[k] == lb[k] and la[k] != lc[k] and not isinstance(la[k], float)]
                for k in la:
                    if isinstance(la[k], float):
                        spread[entry(k)] = max(spread.get(entry(k), 0.0), abs(la[k] - lb[k]))
                        distance[entry(k)] = max(distance.get(entry(k), 0.0), min(abs(lc[k] - la[k]), abs(lc[k] - lb[k])))
                    elif la[k] != lb[k] and lc[k] not in (la[k], lb[k]):
                        wrong.append(k)
                within = {e: {"parent_run_to_run": spread[e], "change_to_nearest_parent_run": distance[e], "bound": 4 * spread[e]} for e in spread if distance[e] > 0}
                wrong += [e for e, w in within.items() if w["change_to_nearest_parent_run"] > w["bound"]]
                v[field] = {"parent_runs_differ": within, "rest": "bitwise equal to the parent" if not wrong else "DIFFERS: " + ", ".join(wrong)}
        ok = ok and "DIFFERS" not in json.dumps(v)
        verdicts[name] = v
    return verdicts, ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=CONFIGS, choices=CONFIGS)
    ap.add_argument("--compare", nargs=3, metavar=("PARENT1", "PARENT2", "CHANGE"))
    ap.add_argument("--brief", action="store_true", help="--compare: write the verdict with the runs' source hashes, without their records")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.compare:
        runs = [json.load(open(p)) for p in args.compare]
        verdicts, ok = compare(*runs)
        if args.brief:
            runs = [{k: r.get(k) for k in ("kernel_source_sha256", "torch")} for r in runs]
        res = {"ok": ok, "verdict": verdicts, "parent": runs[:2], "change": runs[2]}
        print(json.dumps({"ok": ok, "verdict": verdicts}, indent=1))
    else:
        import torch
        import rl_mpc_locomotion_amd  # noqa: F401
        from rl_mpc_locomotion_amd import _lib
        if not torch.cuda.is_available():
            sys.exit("ppo_trainer_trace.py runs the trainer on the GPU; none is visible")
        res = {"kernel_source_sha256": _lib.kernel_source_hash(), "torch": torch.__version__, "configurations": {}}
        for name in args.configs:
            res["configurations"][name] = run(name, "cuda:0")
            print(name, "done", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0 if not args.compare or res["ok"] else 1)
