"""Compare the gfx950 instruction streams of the library's kernels between two trees, kernel by kernel: what a refactor that claims "the same code"
has to show.  Each unit is compiled with ``--cuda-device-only -S`` and the Makefile's flags; a kernel's stream is its instructions with comments,
labels and directives dropped and symbol names and branch-target numbers made anonymous, so a kernel that moved to another unit or namespace still
compares equal.  A kernel that several units of a tree emit is taken from the first unit listed.

    python tools/kernel_isa_diff.py PARENT_TREE CHANGE_TREE [unit ...] > profiles/<name>.txt
    python tools/kernel_isa_diff.py PARENT_TREE CHANGE_TREE horizon:12 horizon:16 horizon:20      # the solver kernels of single planning horizons

Prints one line per kernel: ``identical``, or the size of the diff with both sides' instruction counts, VGPRs, AGPRs and scratch bytes."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ["recurrent", "batch", "ctrl", "policy", "ppo_update", "ppo_gemm", "ppo", "recurrent_policy", "recurrent_bptt"]


def assembly(tree, unit, tmp):
    name, _, h = unit.partition(":")      # "horizon:16": the solver kernels of one planning horizon (mpc_horizon.hip -DMPC_H=16, the Makefile's default contraction)
    src = os.path.join(tree, "rl-mpc-locomotion_amd", "csrc", f"mpc_{name}.hip")
    if not os.path.exists(src):
        return ""
    out = os.path.join(tmp, f"{name}{h}.s")
    extra = ["-DMPC_HORIZON_LIST(X)=X(10)", "-ffp-contract=off"] if unit == "batch" else [f"-DMPC_H={h}"] if h else ["-ffp-contract=off"]
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", *extra, "--cuda-device-only", "-S", src, "-o", out], check=True,
                   capture_output=True)
    return open(out).read()


def short_name(mangled):
    """cell_kernel, gemm_kernel<2,2,1>: the kernel's own identifier out of the Itanium name, whatever namespaces stand in front of it, and its
    integer and bool template arguments."""
    i = 3 if mangled.startswith("_ZN") else 2
    while i < len(mangled) and mangled[i].isdigit():
        m = re.match(r"\d+", mangled[i:])
        ident = mangled[i + m.end():i + m.end() + int(m.group())]
        i += m.end() + len(ident)
        if ident.endswith("kernel"):
            args = re.match(r"I((?:L[ib]\d+E)+)E", mangled[i:])
            return ident + ("<" + ",".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">" if args else "")
    return mangled


def kernels(text):
    """{short name: (instruction lines, vgprs, agprs, scratch)} of every kernel of one unit's assembly."""
    found = {}
    for mangled in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(mangled), text, re.M | re.S).group(1)
        tail = text[text.index(body) + len(body):]
        numbers = [int(re.search(r"; %s: (\d+)" % key, tail).group(1)) for key in ("NumVgprs", "NumAgprs", "ScratchSize")]
        lines = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            lines.append(re.sub(r"\b_Z\w+", "SYM", line))
        found[short_name(mangled)] = (lines, *numbers)
    return found


def tree_kernels(tree, units):
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            for name, k in kernels(assembly(tree, unit, tmp)).items():
                found.setdefault(name, (unit, *k))
    return found


def main():
    parent, change = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or UNITS
    a, b = tree_kernels(parent, units), tree_kernels(change, units)
    print(f"# kernel: parent unit -> change unit: result   (units: {' '.join(units)}; -O3 and the Makefile's contraction flag of each unit, gfx950)")
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in the {'parent' if name in a else 'change'}")
            continue
        (ua, la, *na), (ub, lb, *nb) = a[name], b[name]
        if la == lb and na == nb:
            print(f"{name}: {ua} -> {ub}: identical ({len(la)} instructions, {na[0]} VGPRs, {na[1]} AGPRs, {na[2]} scratch)")
        else:
            changed = sum(1 for d in difflib.unified_diff(la, lb, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            print(f"{name}: {ua} -> {ub}: {changed} diff lines; instructions {len(la)} -> {len(lb)}, VGPRs {na[0]} -> {nb[0]}, AGPRs {na[1]} -> {nb[1]}, "
                  f"scratch {na[2]} -> {nb[2]}")


if __name__ == "__main__":
    main()
