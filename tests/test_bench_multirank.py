"""bench.py's N > 1 control flow on the CPU: `python bench.py --gpus 2 --backend gloo --emulate` launches itself under
torch.distributed.run exactly as the driver's multi-GPU line does (self-launch, the world == --gpus check, robot sharding, barriers
and max-over-ranks timing, the all-gather leg, JSON from rank 0 only) with the host emulation of the kernels (tests/emu) standing in
for the HIP library -- so the first contact with an 8-GPU node cannot die in control flow.  The numbers mean nothing."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, gpus=2, full=True):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--backend", "gloo", "--emulate", "--steps", "2", "--warmup", "1",
                          "--repeats", "2", *(("--full",) if full else ()), *flags], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout          # rank 0 only
    return json.loads(lines[0])


def test_two_ranks_weak_scaling_line():
    b = _run("--robots", "5")
    assert b["n_gpus"] == 2 and b["steps"] == 2 and b["warmup"] == 1 and b["repeats"] == 2 and b["scaling"] == "weak"
    assert b["config"]["robots_per_gpu"] == 5 and b["config"]["robots_total"] == 10
    assert b["value"] > 0 and abs(b["value"] - 10 * 2 / (b["ms_per_step"] * 2e-3)) < 1e-6 * b["value"]
    assert b["all_gather_torques"]["shape_ok"] and b["all_gather_torques"]["robots_total"] == 10
    assert b["solved_fraction"] == 1.0 and "EMULATED" in b["data"]
    assert b["config"]["seam"] == "ctrl"                 # `value` goes through controller.run (SURVEY 8(d)'s unit incl. the torque map)
    sl = b["all_gather_torques"]["sharded_loop"]           # the product-level sharded stepper with its overlapped exchange
    assert sl["shape_ok"] and sl["robots_total"] == 10 and sl["ms_per_tick_with_exchange"] > 0
    # SURVEY 8(e)'s scaling check inside the bench: the 2-rank torques equal the single-process batch bit for bit; one report per rank
    assert sl["bit_identical_to_single_process"] is True and sl["collective"] == {"backend": "gloo", "ranks": 2}
    assert [r["rank"] for r in sl["ranks"]] == [0, 1] and [r["robots"] for r in sl["ranks"]] == [[0, 5], [5, 10]]
    assert [r["torque_block_sha256"] for r in sl["ranks"]] == sl["torque_blocks_sha256_single_process"]


@pytest.mark.parametrize("flags,total", [(("--robots", "2"), 16), (("--config", "4", "--robots-total", "19"), 19), (("--config", "5", "--robots-total", "17"), 17)])
def test_eight_ranks_dry_run(flags, total):
    """The full node: `bench.py --gpus 8` exactly as the driver launches it, on the CPU (gloo, emulated kernels) for configs 2 / 4 / 5 --
    even and uneven shards, barriers, max-over-ranks, gather leg, JSON from rank 0 only.  Unmeasured on hardware until a SCALE record exists."""
    b = _run(*flags, gpus=8)
    assert b["n_gpus"] == 8 and b["config"]["robots_total"] == total and b["value"] > 0
    assert b["all_gather_torques"]["shape_ok"] and b["all_gather_torques"]["robots_total"] == total


@pytest.mark.parametrize("config,h", [(4, 16), (5, 20)])
def test_strong_scaling_configs_shard_unevenly(config, h):
    """configs 4 / 5 shard a fixed total over the ranks; an odd total gives the ranks different shard sizes (the padded all-gather path)."""
    b = _run("--config", str(config), "--robots-total", "5")
    assert b["n_gpus"] == 2 and b["scaling"] == "strong" and b["config"]["horizon"] == h
    assert b["config"]["robots_total"] == 5 and b["config"]["robots_per_gpu"] == 3            # rank 0 holds 3 of the 5
    assert b["all_gather_torques"]["shape_ok"] and b["all_gather_torques"]["robots_total"] == 5


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline keys only, no exchange leg; --dump-outputs writes each rank's torques and solver forces of the last timed
    step, and the --full run of the same arguments computes the same arrays."""
    import numpy as np
    b = _run("--robots", "5", "--dump-outputs", str(tmp_path / "plain"), full=False)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert key in b, key
    assert b["steps"] == 2 and b["repeats"] == 2 and abs(b["value"] - 10 * 2 / (b["ms_per_step"] * 2e-3)) < 1e-6 * b["value"]
    assert "all_gather_torques" not in b and "roofline" not in b and "solved_fraction" not in b
    _run("--robots", "5", "--dump-outputs", str(tmp_path / "full"))
    for name, shape, dtype in (("torques", (5, 12), np.float32), ("forces", (5, 120), np.float64)):
        for rank in (0, 1):
            a = np.load(tmp_path / "plain" / f"{name}_rank{rank}.npy")
            assert a.shape == shape and a.dtype == dtype and np.isfinite(a).all()
            assert np.array_equal(a, np.load(tmp_path / "full" / f"{name}_rank{rank}.npy"))
    assert sorted(os.listdir(tmp_path / "plain")) == ["forces_rank0.npy", "forces_rank1.npy", "torques_rank0.npy", "torques_rank1.npy"]


def test_threaded_control_step_stream_is_the_sequential_one():
    """bench.py draws its controller inputs with ControlStepStream.steps (threads): bit for bit the arrays of step(0), step(1), ..."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from rl_mpc_locomotion_amd.synthetic import ControlStepStream
    for config in (2, 3):
        a, b = ControlStepStream(37, seed=5, config=config), ControlStepStream(37, seed=5, config=config)
        seq = [tuple(x.copy() for x in a.step(s)) for s in range(70)]
        par = list(b.steps(70, workers=3, chunk=16))
        assert len(par) == 70 and b._s == 70
        for x, y in zip(seq, par):
            assert all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(x, y))


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--backend", "gloo", "--emulate"], capture_output=True, text=True, cwd=ROOT, env=env)
    assert out.returncode != 0 and "--gpus 4 but the launcher started 2" in out.stderr


def test_gloo_needs_emulate():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backend", "gloo"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode != 0 and "needs --emulate" in out.stderr
