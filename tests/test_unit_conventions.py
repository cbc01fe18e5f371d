"""The two conventions of the C ABI units ("Two conventions of the C ABI units"), checked on the text of csrc/: a kernel is
defined in the one unit that launches it, and a kernel's dynamic-LDS limit is set by mpc_host.h's grow-only LdsLimit alone.  No compute."""
import glob
import os
import re

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")


def _code(path):
    """The file without its comments."""
    text = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _units():
    units = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(units) >= 20
    return units


def test_no_include_sits_inside_a_namespace():
    """A unit that wrapped a header in ``namespace { #include ... }`` compiled that header's kernels a second time under internal names."""
    for unit in _units():
        depth, opened = 0, []                                                    # brace depth, and the depths at which a namespace was opened
        for line in _code(unit).splitlines():
            if re.match(r"\s*#\s*include\b", line):
                assert not opened, f"{os.path.basename(unit)}: {line.strip()} inside a namespace"
                continue
            for token in re.findall(r"\bnamespace\b[^{;]*\{|\{|\}", line):
                if token == "}":
                    depth -= 1
                    if opened and opened[-1] == depth:
                        opened.pop()
                else:
                    if token.startswith("namespace"):
                        opened.append(depth)
                    depth += 1
        assert depth == 0 and not opened, os.path.basename(unit)


def _includes():
    """file -> the csrc headers it includes"""
    return {os.path.basename(path): set(re.findall(r'#\s*include\s+"([^"/]+)"', _code(path))) for path in glob.glob(os.path.join(CSRC, "*.h")) + _units()}


def _reach(includes, name, seen):
    for h in includes.get(name, ()):
        if h not in seen:
            seen.add(h)
            _reach(includes, h, seen)
    return seen


def test_a_header_with_kernels_belongs_to_one_unit():
    includes = _includes()
    with_kernels = [os.path.basename(h) for h in glob.glob(os.path.join(CSRC, "*.h")) if "__global__" in _code(h)]
    assert "ppo_gemm.h" in with_kernels and "recurrent_cell.h" not in with_kernels and "policy_mlp.h" not in with_kernels
    units = [u for u in includes if u.startswith("mpc_") and u.endswith(".hip")]
    for h in with_kernels:
        users = sorted(u for u in units if h in _reach(includes, u, set()))
        assert len(users) <= 1, f"{h} defines kernels and is included by {users}"


def test_every_function_of_mpc_batch_h_is_defined_in_the_unit_its_prefix_names():
    """include/mpc_batch.h declares three handles and the peer exchange; each is one unit."""
    declared = re.findall(r"^[A-Za-z_][^;(]*?\b(mpc_\w+)\s*\(", _code(os.path.join(ROOT, "include", "mpc_batch.h")), re.M)
    assert len(declared) == len(set(declared)) == 65

    def home(name):
        if name.startswith("mpc_ctrl_"):
            return "mpc_ctrl.hip"
        if name.startswith(("mpc_policy_", "mpc_pack_commands")):
            return "mpc_policy.hip"
        if name.startswith("mpc_peer_"):
            return "mpc_peer.hip"
        assert name.startswith("mpc_batch_") or name in ("mpc_last_error", "mpc_input_len", "mpc_supported_horizons", "mpc_device_clock"), name
        return "mpc_batch.hip"
    defined = {}                                                                 # function -> the units with a definition of it (a type at column 0, the name, a body)
    for unit in _units():
        for name in re.findall(r"^[A-Za-z_][\w \*]*?\b(mpc_\w+)\s*\([^;{]*\{", _code(unit), re.M):
            defined.setdefault(name, []).append(os.path.basename(unit))
    for name in declared:
        assert defined.get(name) == [home(name)], (name, defined.get(name))
    assert {home(name) for name in declared} == {"mpc_batch.hip", "mpc_ctrl.hip", "mpc_policy.hip", "mpc_peer.hip"}
    # the controller's arithmetic (controller.h with gelsd43.h and the svml_acosf table behind it) is compiled into the controller unit alone
    includes = _includes()
    assert [u for u in ("mpc_batch.hip", "mpc_ctrl.hip", "mpc_policy.hip") if "controller.h" in _reach(includes, u, set())] == ["mpc_ctrl.hip"]


def test_the_lds_limit_is_set_in_mpc_host_h_only():
    sources = [p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".h", ".hip"))]
    setters = sorted(os.path.basename(p) for p in sources if "hipFuncSetAttribute" in open(p).read())      # (comments count: one place speaks of it)
    assert setters == ["mpc_host.h"]
    users = sorted(os.path.basename(u) for u in _units() if "mpchost::LdsLimit" in _code(u))
    assert users == ["mpc_policy.hip", "mpc_ppo.hip", "mpc_recurrent.hip", "mpc_recurrent_bptt.hip", "mpc_recurrent_policy.hip"]
    for u in users:                                                              # every launch with dynamic LDS has its kernel's limit holder in the unit
        assert len(re.findall(r"mpchost::LdsLimit\s+\w+\(", _code(os.path.join(CSRC, u)))) >= 1
