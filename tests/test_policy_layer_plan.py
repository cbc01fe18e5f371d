"""What tests/test_policy_layer_gpu.py's tables reach of policy::layer (csrc/policy_mlp.h), and the host-only half of its layer test, without a GPU:
  * layer's dispatch restated in a few lines (block count, blocks per wave and trip, trips of each wave, dead blocks per group): the tables reach
    every (NB, wrapped trip, dead block) class of group that the C ABI's shape rules (hidden widths multiples of 16, at most 16 outputs, at most 8
    layers) can reach, and the branches the table's comments name;
  * every net of the chain test is one the ABI accepts, and the wide one needs more than 64 KB of LDS;
  * the float64 reference, the derived bound and the 3 x bite assertion on every case's inputs, against a numpy float32 emulation of a k-ordered sum:
    an honest float32 implementation stays inside the bound at every shape, the same emulation with one product dropped, one doubled or the bias
    dropped leaves it in every element;
  * the harness cross-compiles for gfx950 and uses no scratch."""
import re
import subprocess

import numpy as np
import pytest

from tests import test_policy_layer_gpu as T

MAX_LAYERS, MAX_OUTPUTS, MAX_LDS = 8, 16, 160 * 1024             # policy::kMaxLayers, check_stack's limits, mpc_ac_create / mpc_policy_create


def admissible_widths(limit=4096):
    """The NOUT a layer can have under the ABI: a hidden width (a multiple of 16) or a last layer's 1 .. 16 outputs."""
    return list(range(1, MAX_OUTPUTS + 1)) + list(range(16, limit + 1, 16))


def accepted(dims, outputs):
    """check_stack of csrc/mpc_ppo.hip (the limits of mpc_policy_create) and the LDS limit."""
    n_layers = len(dims) - 1
    return (1 <= n_layers <= MAX_LAYERS and all(d > 0 and d % 16 == 0 for d in dims[:-1]) and dims[-1] == outputs <= MAX_OUTPUTS
            and T.lds_bytes(dims) <= MAX_LDS)


def widths_under_test():
    """(K, NOUT) of every layer a GPU test runs: the layer table and the layers of the chain test's nets."""
    out = [(c["K"], c["NOUT"]) for c in T.CASES]
    for net in T.NETS:
        for dims in T.net_dims(net):
            out += list(zip(dims[:-1], dims[1:]))
    return out


def test_the_dispatch_restatement():
    assert T.dispatch(16) == dict(nblocks=1, NB=1, groups=1, trips=[1, 0, 0, 0, 0, 0, 0, 0], dead=[0])
    assert T.dispatch(12)["nblocks"] == 1 and T.dispatch(1)["trips"] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert T.dispatch(128)["trips"] == [1] * 8 and T.dispatch(144)["trips"] == [2, 1, 1, 1, 1, 1, 1, 1] and T.dispatch(240)["NB"] == 1
    assert T.dispatch(256) == dict(nblocks=16, NB=2, groups=8, trips=[1] * 8, dead=[0] * 8)
    assert T.dispatch(272) == dict(nblocks=17, NB=2, groups=9, trips=[2, 1, 1, 1, 1, 1, 1, 1], dead=[0] * 8 + [1])
    assert T.dispatch(496) == dict(nblocks=31, NB=2, groups=16, trips=[2] * 8, dead=[0] * 15 + [1])
    assert T.dispatch(512) == dict(nblocks=32, NB=4, groups=8, trips=[1] * 8, dead=[0] * 8)
    assert T.dispatch(528) == dict(nblocks=33, NB=4, groups=9, trips=[2, 1, 1, 1, 1, 1, 1, 1], dead=[0] * 8 + [3])
    assert T.dispatch(1040) == dict(nblocks=65, NB=4, groups=17, trips=[3, 2, 2, 2, 2, 2, 2, 2], dead=[0] * 16 + [3])


def test_the_tables_reach_every_reachable_branch():
    reachable = set().union(*(T.branches(n) for n in admissible_widths()))
    # a dead block needs NB > 1, and then a group past the first eight: 2 (g + 1) > nblocks >= 16 only for g >= 8
    assert reachable == {(1, False, False), (1, True, False), (2, False, False), (2, True, False), (2, True, True), (4, False, False), (4, True, False),
                         (4, True, True)}
    layer_table = set().union(*(T.branches(c["NOUT"]) for c in T.CASES))
    assert layer_table == reachable, reachable - layer_table
    chains = set().union(*(T.branches(nout) for net in T.NETS for dims in T.net_dims(net) for nout in dims[1:]))
    assert chains == reachable, reachable - chains
    for table in ([c["NOUT"] for c in T.CASES], [nout for net in T.NETS for dims in T.net_dims(net) for nout in dims[1:]]):
        for nb in (1, 2, 4):
            trips = [max(T.dispatch(n)["trips"]) for n in table if T.dispatch(n)["NB"] == nb]
            assert 1 in trips and max(trips) >= 2, (nb, trips)                   # one trip, and a wave that wraps
        assert any(T.dispatch(n)["NB"] == 4 and max(T.dispatch(n)["trips"]) == 3 for n in table)
        assert {max(T.dispatch(n)["dead"]) for n in table} >= {0, 1, 3}
    # what the table's comments name
    ks, nouts = {c["K"] for c in T.CASES}, {c["NOUT"] for c in T.CASES}
    assert 16 in ks and max(ks) > 512 and {528, 1040} <= ks                      # one k-trip (no prefetch), K above 512
    assert {1, 12} <= nouts                                                      # ragged last layers: dead lanes inside a live block
    assert T.dispatch(16)["trips"].count(0) == 7                                 # seven idle waves
    assert any(c["in_pad"] > 4 for c in T.CASES) and any(c["groups"] > 1 for c in T.CASES)
    assert all((c["K"] + c["in_pad"]) % 4 == 0 and c["K"] % 16 == 0 and (c["NOUT"] % 16 == 0 or c["NOUT"] <= MAX_OUTPUTS) for c in T.CASES)
    assert max(k * n for k, n in widths_under_test()) <= 1040 * 1040


def test_the_chain_nets_are_accepted_by_the_abi_and_cover_what_they_name():
    for net in T.NETS + (T.NARROW_NET,):
        actor, critic = T.net_dims(net)
        assert accepted(actor, 12) and accepted(critic, 1), net
    assert T.net_lds_bytes(T.WIDE_NET) == 4 * 16 * (48 + 4 + 1040 + 4) > 64 * 1024 and T.WIDE_NET in T.NETS
    assert T.net_lds_bytes(T.NARROW_NET) < 64 * 1024
    all_dims = [d for net in T.NETS for d in T.net_dims(net)]
    assert any(len(d) - 1 == MAX_LAYERS for d in all_dims)                       # eight layers
    assert {d[0] for d in all_dims} >= {16, 48, 64}                              # num_obs other than 48
    assert any(max(d[1::2]) >= 1040 and max(d[0::2]) <= 48 for d in all_dims)    # the widest activation in the odd buffer, the even one narrow
    assert any(max(d[0::2]) >= 528 and max(d[1::2]) <= 16 for d in all_dims)     # ... and the other way round
    assert not accepted([48, 24, 12], 12) and not accepted([48] + [16] * 8 + [12], 12) and not accepted([48, 16, 17], 17)
    assert set(T.CHAIN_ROWS) == {1, 16, 17, 33}


def emulate(X, W, b, drop=None, double=None, bias=True):
    """A k-ordered float32 sum, every product and every sum rounded (no fused multiply-add), then the bias."""
    acc = np.zeros((X.shape[0], W.shape[0]), np.float32)
    for k in range(X.shape[1]):
        if k == drop:
            continue
        term = X[:, k:k + 1] * W[None, :, k]
        acc = acc + term
        if k == double:
            acc = acc + term
    assert acc.dtype == np.float32
    return acc + b[None, :] if bias else acc


@pytest.mark.parametrize("case", range(len(T.CASES)))
def test_a_float32_sum_stays_inside_the_bound_and_a_dropped_term_does_not(case):
    o = T.layer_case(case)                                                       # asserts the 3 x bite of its own inputs
    K = o["K"]
    inside = lambda y: np.abs(y.astype(np.float64) - o["exact"]) <= o["bound"]
    honest = emulate(o["X"], o["W"], o["b"])
    ratio = (np.abs(honest.astype(np.float64) - o["exact"]) / o["bound"]).max()
    print(f"case {case} (K = {K}, NOUT = {o['NOUT']}): k-ordered float32 sum, largest error / bound {ratio:.3f}")
    assert inside(honest).all()
    for k in sorted({0, K // 2, K - 16, K - 1}):
        assert not inside(emulate(o["X"], o["W"], o["b"], drop=k)).any(), k
        assert not inside(emulate(o["X"], o["W"], o["b"], double=k)).any(), k
    assert not inside(emulate(o["X"], o["W"], o["b"], bias=False)).any()
    # a misplaced term: the last weight of each row taken from the row before
    W = o["W"].copy()
    W[:, K - 1] = np.roll(o["W"][:, K - 1], 1)
    moved = o["W"][:, K - 1] != W[:, K - 1]
    if moved.any():
        d = np.abs(o["X"][:, K - 1:K].astype(np.float64) * (W[:, K - 1].astype(np.float64) - o["W"][:, K - 1].astype(np.float64))[None, :])
        far = d > 2 * o["bound"]                                                 # (two magnitudes of one range can lie closer than that)
        assert not inside(emulate(o["X"], W, o["b"]))[far].any()


def test_the_harness_compiles_for_gfx950_without_scratch(tmp_path):
    out = tmp_path / "policy_layer_harness.o"
    flags = [f for f in T.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([T.HIPCC, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", T.CSRC, "-c", T.HARNESS, "-o", str(out)],
                       check=True, capture_output=True, text=True)
    found = {name: int(scratch) for name, scratch in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S)}
    hit = [s for k, s in found.items() if "layer_kernel" in k]
    assert hit == [0], found
