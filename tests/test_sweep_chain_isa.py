"""How the pair sweep's fetch is waited for in the compiled job kernel mpc_solve_jobs_kernel<10> (no GPU needed: hipcc cross-compiles gfx950, as
tests/test_isa_budget.py does).

mpc_wrench.h Solver::sweep_pair requests piv, then the two pivot rows at the lane's tile column (what x and y are made of), then the two rows at its
tile row (u, v: first used by the cross update): fourteen LDS loads, the last six of them u and v.  LDS answers in order, so x and y can start while
those six are still outstanding, and that is the point of the order: in each of the three sweep loops (factor, refactor, polish) the first wait
after every pair's fetch must leave at least six loads outstanding.  A fetch that interleaves the rows, or a schedule that waits for the whole
fetch (lgkmcnt(0)), exposes the full round trip again.  The kernel keeps no private segment."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "mpc_h10.s")
    isa_census.compile_to_asm(os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc"), out, (10,))
    return open(out).read()


def _sweep_loops(asm):
    """[instruction lines in program order] of each sweep loop of the job kernel at h = 10."""
    heads = [k for k, a in isa_census.loop_stats(asm, 10).items() if a["role"] == "sweep"]
    loops = []
    for head in heads:
        lines = []
        for block in isa_census._blocks(asm, 10):
            key = isa_census._loop_of(block)
            if key is not None and key[0] == head:
                lines += [l.strip() for l in isa_census._instructions(block)]
        loops.append(lines)
    return loops


def test_x_and_y_start_while_u_and_v_are_on_their_way(asm):
    loops = _sweep_loops(asm)
    assert len(loops) == 3      # factor, refactor, polish
    for lines in loops:
        # a pair's fetch: a run of LDS loads (nothing but loads in between)
        fetches, i = [], 0
        while i < len(lines):
            if lines[i].startswith("ds_read"):
                j = i
                while j < len(lines) and lines[j].startswith("ds_read"):
                    j += 1
                if j - i >= 12:
                    fetches.append((i, j))
                i = j
            else:
                i += 1
        assert len(fetches) == 3, fetches      # three pivot pairs per trip
        for i, j in fetches:
            assert j - i == 14, lines[i:j]      # piv (128 + 64 bits), 4 rows x three 128-bit loads
            wait = next(k for k in range(j, len(lines)) if lines[k].startswith("s_waitcnt") and "lgkmcnt" in lines[k])
            left = int(re.search(r"lgkmcnt\((\d+)\)", lines[wait]).group(1))
            print(f"fetch at {i}: first wait {lines[wait]!r} at {wait}")
            assert left >= 6, (lines[wait], "the first use waits for u and v as well")
            # the loads still outstanding are those of the rows at the tile row's slots: the last six share one address register, the six
            # before them (the tile column's) another
            regs = [re.search(r"ds_read_b128 v\[\d+:\d+\], (v\d+)", l).group(1) for l in lines[j - 12:j]]
            assert len(set(regs[:6])) == 1 and len(set(regs[6:])) == 1, regs


def test_the_job_kernel_has_no_private_segment(asm):
    m = re.search(r"\.amdhsa_kernel [^\n]*mpc_solve_jobs_kernelILi10E.*?\.end_amdhsa_kernel", asm, re.S)
    assert m, "no mpc_solve_jobs_kernel<10> in the assembly"
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(0)).group(1)) == 0
