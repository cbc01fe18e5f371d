"""csrc/ppo_gemm_plan.h -- which ppo_gemm.h instantiation a launch of the device PPO update runs, and how backward weight is chunked -- on the CPU: the
header (no HIP in it) is compiled with g++ into a small shim and driven through ctypes.  What is pinned here:
  * the plan of every launch of the large cases of tests/test_ppo_update_gpu.py, launch by launch;
  * that the (kind, tile, chunk length) combinations of the training workload (PPOConfig()'s nets, 4096 robots x 24 steps / 4 mini-batches) are among
    those the GPU tests' own shape tables plan, so a change of the plan that moves the workload onto kernels no test runs fails here, without a GPU;
  * that the workspace of mpc_ppo_update_create (ceil(max_rows / 256) chunk partials per layer) holds every planned launch;
  * that the shape tables of tests/test_ppo_gemm_gpu.py cover the tile and vector edges they name, with every chunk length;
  * the same for the workload on the wide observation rows of a height scan (240 columns by default, and 256): the width moves one launch, the first
    layer's weight gradient, onto 1024-row chunks (and at 256 onto the 128 x 128 tile), and the GPU tests' wide tables plan and run that."""
import ctypes as C
import subprocess

import pytest

from rl_mpc_locomotion_amd import ppo as P
from tests import test_ppo_gemm_gpu as G
from tests import test_ppo_update_gpu as U
from tests.test_ppo_update import CSRC

FORWARD, BACKWARD_DATA, BACKWARD_WEIGHT = 0, 1, 2
NARROW, WIDE = "narrow", "wide"

SHIM = r"""
#include "ppo_gemm_plan.h"
extern "C" {
// out: chunk_rows, wide, grid x, then tiles_m, tiles_n, chunks of either problem
void shim_plan(int kind, const int *mnk, int *out) {
  const pgemm::Shape shape[2] = {{mnk[0], mnk[1], mnk[2]}, {mnk[3], mnk[4], mnk[5]}};
  const pgemm::Plan p = pgemm::plan_gemm(kind, shape);
  out[0] = p.chunk_rows; out[1] = p.wide ? 1 : 0; out[2] = (int)p.grid_x;
  for (int k = 0; k < 2; ++k) { out[3 + 3 * k] = p.p[k].tiles_m; out[4 + 3 * k] = p.p[k].tiles_n; out[5 + 3 * k] = p.p[k].chunks; }
}
int shim_kinds() { return pgemm::kForward == 0 && pgemm::kBackwardData == 1 && pgemm::kBackwardWeight == 2; }
int shim_chunk() { return pgemm::kChunk; }
int shim_min_chunk() { return pgemm::kMinChunk; }
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("ppo_gemm_plan_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.shim_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p]; L.shim_plan.restype = None
    assert L.shim_kinds() == 1 and L.shim_chunk() == 1024 and L.shim_min_chunk() == 256

    def run(kind, a, b=None):
        """The plan of one launch: a, b = (M, N, K) of the two problems (None: the slot is empty)."""
        mnk = (C.c_int * 6)(*(a or (0, 0, 0)), *(b or (0, 0, 0)))
        out = (C.c_int * 9)()
        L.shim_plan(kind, mnk, out)
        return dict(chunk_rows=out[0], tile=WIDE if out[1] else NARROW, grid_x=out[2], problems=[tuple(out[3:6]), tuple(out[6:9])])
    return run


def launches(nets, rows, num_obs=48):
    """mpc_ppo_update_grads' GEMM launches for a net pair (hidden layers of actor and critic) at `rows` rows of `num_obs` columns, in its order: (kind, actor's (M, N, K) or None,
    critic's): layer l of both nets side by side forward; backward from each net's last layer down, backward weight, then backward data into the
    layer below.  The sequence is copied by hand from csrc/mpc_ppo_update.hip (which says so at its forward and backward loops): a launch added or
    reshaped there has to be restated here."""
    dims = [[num_obs, *nets[0], 12], [num_obs, *nets[1], 1]]
    nl = [len(d) - 1 for d in dims]
    out = []
    for l in range(max(nl)):
        out.append((FORWARD, *[(rows, d[l + 1], d[l]) if l < n else None for d, n in zip(dims, nl)]))
    for s in range(max(nl)):
        w, x = [], []
        for d, n in zip(dims, nl):
            l = n - 1 - s
            w.append((d[l + 1], d[l], rows) if l >= 0 else None)
            x.append((rows, d[l], d[l + 1]) if l > 0 else None)
        out.append((BACKWARD_WEIGHT, *w))
        if any(x):
            out.append((BACKWARD_DATA, *x))
    return out


def planned(plan, nets, rows, num_obs=48):
    """Per launch (kind, tile, chunk_rows, chunks of the two problems)."""
    out = []
    for kind, a, b in launches(nets, rows, num_obs):
        p = plan(kind, a, b)
        out.append((kind, p["tile"], p["chunk_rows"], (p["problems"][0][2], p["problems"][1][2])))
    return out


def combos(plan, nets, rows, num_obs=48):
    return {(kind, tile, chunk_rows) for kind, tile, chunk_rows, _ in planned(plan, nets, rows, num_obs)}


def _rows(case):
    n, T, mb = case
    return n * T // mb


def test_plan_reproduces_the_rule(plan):
    """Spot values of the rule itself: the thresholds (512 workgroups of 128 x 64 for a longer chunk, 256 tiles of 128 x 128 and columns that fill them
    for the wide tile), an empty slot, the grid."""
    assert plan(FORWARD, (1, 12, 48)) == dict(chunk_rows=0, tile=NARROW, grid_x=1, problems=[(1, 1, 1), (0, 0, 1)])
    assert plan(FORWARD, (16385, 128, 256), (16385, 128, 256))["tile"] == WIDE                   # 2 x 129 tiles
    assert plan(FORWARD, (16257, 128, 256), (16256, 128, 256))["tile"] == NARROW                  # 128 + 127 tiles
    assert plan(FORWARD, (16385, 128, 256), (16385, 64, 256))["tile"] == NARROW                   # one problem's columns do not fill the tile
    assert plan(FORWARD, (32768, 128, 256)) == dict(chunk_rows=0, tile=WIDE, grid_x=256, problems=[(256, 1, 1), (0, 0, 1)])
    p = plan(BACKWARD_WEIGHT, (256, 512, 16385), (256, 512, 16385))
    assert p == dict(chunk_rows=1024, tile=WIDE, grid_x=2 * 4 * 17, problems=[(2, 4, 17), (2, 4, 17)])
    assert plan(BACKWARD_WEIGHT, (256, 512, 15 * 1024), (256, 512, 15 * 1024))["chunk_rows"] == 512      # 480 workgroups at 1024
    assert plan(BACKWARD_WEIGHT, (12, 128, 1040), (1, 128, 1040)) == dict(chunk_rows=256, tile=NARROW, grid_x=10, problems=[(1, 2, 5), (1, 2, 5)])


def test_the_large_cases_plan_the_production_kernels(plan):
    """16 385 rows, launch by launch: the wide tile in every kind, chunks of 1024 rows (17, the last of one row) and 256 on the reference nets, 512 (33,
    the last of one row) on the square ones."""
    rows = _rows(U.BIG_ROWS["production"])
    assert rows == 16385
    assert planned(plan, U.BIG_NETS["reference"], rows) == [
        (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, NARROW, 0, (1, 1)),
        (BACKWARD_WEIGHT, NARROW, 256, (65, 65)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 256, (65, 65)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 1024, (17, 17)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, NARROW, 256, (65, 65))]
    assert planned(plan, U.BIG_NETS["square"], rows) == [
        (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, NARROW, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 256, (65, 65)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 512, (33, 33)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, NARROW, 256, (65, 65))]
    # and the earlier row counts stay where they were: narrow, 256-row chunks
    for nets in U.NETS.values():
        for case in U.ROWS.values():
            assert all(tile == NARROW and chunk_rows in (0, 256) for _, tile, chunk_rows, _ in planned(plan, nets, _rows(case)))


def test_the_training_workload_runs_only_kernels_the_gpu_tests_run(plan):
    cfg = P.PPOConfig()
    rows = 4096 * cfg.num_steps_per_env // cfg.num_mini_batches
    assert rows == 24576
    production = combos(plan, (cfg.actor_hidden_dims, cfg.critic_hidden_dims), rows)
    assert {kind for kind, _, _ in production} == {FORWARD, BACKWARD_DATA, BACKWARD_WEIGHT}
    # end to end: what tests/test_ppo_update_gpu.py's own tables plan
    tested = set()
    for nets in U.NETS.values():
        for case in U.ROWS.values():
            tested |= combos(plan, nets, _rows(case))
    for nets in U.BIG_NETS.values():
        for case in U.BIG_ROWS.values():
            tested |= combos(plan, nets, _rows(case))
    assert production <= tested, production - tested
    assert (BACKWARD_WEIGHT, WIDE, 512) in tested
    # kernel by kernel: tests/test_ppo_gemm_gpu.py runs every case with both tiles
    direct = {(kind, tile, 0) for kind in (FORWARD, BACKWARD_DATA) for tile in G.TILES}
    direct |= {(BACKWARD_WEIGHT, tile, s[3]) for tile in G.TILES for case in G.BW_CASES for s in case["shapes"] if s}
    assert production <= direct and tested <= direct, (production - direct, tested - direct)


def _height_scan_row():
    """(width, live columns) of the observation row with HeightScan's default points: the task's columns and the scan, padded with zeros."""
    from rl_mpc_locomotion_amd import height_scan, rl_task
    points = len(height_scan.POINTS_X) * len(height_scan.POINTS_Y)
    return height_scan.padded_width(rl_task.NUM_OBS, points), rl_task.NUM_OBS + points


def test_the_wide_training_workload_runs_only_kernels_the_gpu_tests_run(plan):
    """The workload with the default height scan, and one of 256 columns, launch by launch: the plan is the 48-wide one except in the last launch, the
    first layer's weight gradient (the only backward-weight launch that reads X through the index), which takes 1024-row chunks (24) -- on the
    128 x 64 tile at 240 columns, on the 128 x 128 tile at 256.  Its combinations are among those that the wide tables of
    tests/test_ppo_update_gpu.py plan, and that launch itself is planned there with 17 chunks, the last of one row."""
    cfg = P.PPOConfig()
    nets = (cfg.actor_hidden_dims, cfg.critic_hidden_dims)
    rows = 4096 * cfg.num_steps_per_env // cfg.num_mini_batches
    assert rows == 24576 and nets == U.NETS["reference"]
    scan, live = _height_scan_row()
    assert scan in U.WIDTHS and scan in U.BIG_WIDTHS and U.ZERO_PAD == {scan: scan - live}      # the GPU tests' wide row is this one, zeros included
    assert U.BIG_WIDTHS == (scan, 256) and (scan, scan - live) == (240, 5)
    at48 = planned(plan, nets, rows)
    assert at48 == [
        (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, WIDE, 0, (1, 1)), (FORWARD, NARROW, 0, (1, 1)),
        (BACKWARD_WEIGHT, NARROW, 256, (96, 96)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 256, (96, 96)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, WIDE, 1024, (24, 24)), (BACKWARD_DATA, WIDE, 0, (1, 1)),
        (BACKWARD_WEIGHT, NARROW, 256, (96, 96))]
    direct = {(kind, tile, 0) for kind in (FORWARD, BACKWARD_DATA) for tile in G.TILES}
    direct |= {(BACKWARD_WEIGHT, tile, s[3]) for tile in G.TILES for case in G.BW_CASES for s in case["shapes"] if s}
    for num_obs, tile in ((scan, NARROW), (256, WIDE)):
        assert launches(nets, rows, num_obs)[-1] == (BACKWARD_WEIGHT, (512, num_obs, rows), (512, num_obs, rows))
        got = planned(plan, nets, rows, num_obs)
        assert got == at48[:-1] + [(BACKWARD_WEIGHT, tile, 1024, (24, 24))] and got != at48, (num_obs, got)
        # end to end: the wide tables alone
        tested = set()
        for name in U.WIDE_NETS:
            for case in U.WIDE_ROWS:
                for width in U.WIDTHS:
                    tested |= combos(plan, U.NETS[name], _rows(U.ROWS[case]), width)
        assert all(tile == NARROW and chunk_rows in (0, 256) for _, tile, chunk_rows in tested)      # (the small cases: the index, the widths, the edges)
        big = _rows(U.BIG_ROWS["production"])
        assert planned(plan, nets, big, num_obs)[-1] == (BACKWARD_WEIGHT, tile, 1024, (17, 17)) and big - 16 * 1024 == 1
        tested |= combos(plan, nets, big, num_obs)
        production = combos(plan, nets, rows, num_obs)
        assert (BACKWARD_WEIGHT, tile, 1024) in production
        assert production <= tested, production - tested
        assert production <= direct and tested <= direct, (production - direct, tested - direct)
    # 15 361 rows is where (512, 240, rows) first plans 1024-row chunks (2 x 4 x 4 x ceil(rows / 1024) >= 512; 512-row chunks below that)
    assert planned(plan, nets, 15360, scan)[-1][2] == 512 and planned(plan, nets, 15361, scan)[-1][2] == 1024


def test_the_workspace_holds_every_planned_launch(plan):
    """mpc_ppo_update_create allocates ceil(max_rows / kMinChunk) chunk partials per layer; a launch at rows <= max_rows never plans more."""
    all_nets = list(U.ALL_NETS.values()) + [((512, 256, 128), (64,)), ((16,), (512, 512))]
    for nets in all_nets:
        for num_obs in (48, 16, 240, 256):
            for rows in (1, 97, 255, 256, 257, 1023, 1024, 1025, 1040, 4095, 4097, 16385, 24576, 98304):
                for kind, _, chunk_rows, chunks in planned(plan, nets, rows, num_obs):
                    assert max(chunks) <= -(-rows // 256), (nets, num_obs, rows, chunks)
                    if kind == BACKWARD_WEIGHT:
                        assert chunk_rows in (256, 512, 1024) and all(c in (1, -(-rows // chunk_rows)) for c in chunks)
                    else:
                        assert chunk_rows == 0 and chunks == (1, 1)


def test_the_direct_tests_shape_tables_cover_the_edges():
    """tests/test_ppo_gemm_gpu.py: every axis value with every kind (every case runs with both tiles), two problems per launch and one empty second
    slot, padded leading dimensions, an index in forward and in backward weight, every chunk length with a one-row and with a full last chunk, and
    the 240-column rows as the update reads them."""
    assert sorted(G.TILES) == ["narrow", "wide"] and G.TILES["narrow"] == 0 and G.TILES["wide"] == 1
    fb = [s for case in G.FB_CASES for s in case["shapes"] if s]
    assert {s[0] for s in fb} >= {1, 31, 33, 127, 128, 129, 257}
    assert {s[1] for s in fb} >= {1, 12, 16, 63, 65, 127, 128, 129, 144, 240}
    assert {s[2] for s in fb} >= {1, 2, 3, 4, 5, 16, 31, 32, 33, 48, 63, 65, 100, 240}
    # the wide rows' first layer: K = 240 through the index on unpadded rows (lda = 240)
    assert any(s and s[2] == 240 and case["idx"][k] and not case["pad"] for case in G.FB_CASES for k, s in enumerate(case["shapes"]))
    bw = [s for case in G.BW_CASES for s in case["shapes"] if s]
    assert {s[0] for s in bw} >= {1, 12, 16, 127, 129}
    assert {s[1] for s in bw} >= {16, 48, 65, 128, 144, 240}
    # the wide rows' first layer: nin = 240 through the index with ldb = 240, in 1024-row chunks with a last chunk of one row; and in 256-row chunks
    assert any(s and s[1] == 240 and s[3] == 1024 and s[2] % 1024 == 1 and s[2] > 1024 and case["idx"][k] and not case["pad"]
               for case in G.BW_CASES for k, s in enumerate(case["shapes"]))
    assert any(s[1] == 240 and s[3] == 256 and s[2] > 256 for s in bw)
    assert {s[2] for s in bw} >= {1, 31, 33, 255, 256, 257, 1023, 1025, 2049}
    for chunk_rows in (256, 512, 1024):
        last = {s[2] - (-(-s[2] // chunk_rows) - 1) * chunk_rows for s in bw if s[3] == chunk_rows and s[2] > chunk_rows}
        assert 1 in last, chunk_rows
        assert any(s[3] == chunk_rows and s[2] % chunk_rows == 0 for s in bw), chunk_rows
    for table in (G.FB_CASES, G.BW_CASES):
        assert sum(case["shapes"][1] is None for case in table) == 1 and all(case["shapes"][0] for case in table)
        assert all(case["shapes"][0] != case["shapes"][1] for case in table)
        assert any(case["pad"] for case in table) and any(not case["pad"] for case in table)
        assert any(any(case["idx"]) for case in table) and any(not all(case["idx"]) for case in table)
