"""policy::layer of csrc/policy_mlp.h -- the layer that mlp_kernel (WeightPolicy.step) and ac_kernel (ActorCritic.act / evaluate / act_inference) share --
on the MI355X, one layer at a time against the same product in float64 on the CPU, element by element; then the production kernels against the chain
of those layers, bit for bit.

tests/device/policy_layer_harness.hip is compiled once per run with hipcc and loaded through ctypes: a workgroup of policy::kThreads per 16 rows copies
its input rows into LDS at the test's stride, calls policy::layer unchanged and copies the whole LDS output block back.

The tolerance is derived, not measured (the bound and the reasoning of tests/test_ppo_gemm_gpu.py).  A float32 sum of n terms, in any order and fused or
not, lies within gamma_n * sum |terms| of the exact sum, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1); the bias is one more term, so per element of the pre-activation
  |y - y64| <= gamma_{K+1} (sum_k |x_k w_k| + |b|).
The inputs make the bound bite: magnitudes are drawn from +-[lo, hi] times one scale per operand, the range narrowing with K (mag_range), and every case
asserts of its own inputs that each single product, and the bias, is at least 3 x the bound of its element: a dropped, doubled or misplaced term cannot
pass.  (The assertion is host-only; tests/test_policy_layer_plan.py runs it, the reference and the bound without a GPU.)

ELU is checked on the kernel's own pre-activation p (the elu = 0 launch): the identity bit for bit where p > 0; where p <= 0, within 2 float32 ulp of
expm1(float64(p)) -- the "HIP math API" page of the HIP documentation (Single precision mathematical functions) lists expm1f with a maximum error of
1 ulp, and one more ulp is the rounding of the float64 value it is compared with.

Safety nets of every case: NaN in every LDS word of the input rows beyond K (the stride is K + 4, K + 12 or K + 36); the output block pre-filled with
a NaN-payload sentinel that must survive bit for bit in columns >= NOUT and in the stride padding; W and b of exactly NOUT K and NOUT floats at the end
of a sentinel-filled allocation.

CASES holds the smallest (K, NOUT) that reach each branch of layer's dispatch with eight waves (asserted of the harness, so a change of POLICY_THREADS
fails here instead of silently un-covering; tests/test_policy_layer_plan.py checks the coverage of the table).  Largest measured error / bound per
branch: DESIGN.md section 8.3."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, draw, gamma, ulp32
from tests.test_ppo_gemm_gpu import CSRC, HIPCC, SENTINEL, _bits, _region, _sentinel, _untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HARNESS = os.path.join(ROOT, "tests", "device", "policy_layer_harness.hip")
HIPCC_FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off")
WAVES, ROWS, PAD = 8, 16, 4                                       # policy::kWaves, kRows, kPad: asserted of the harness

# (K, NOUT) per branch of policy::layer; groups: workgroups (16 rows each); in_pad / out_pad: the LDS strides are K + in_pad and NOUT + out_pad.
CASES = (
    # blocks<1>: one block and seven idle waves, one k-trip (no prefetch); 8 blocks; 9 (wave 0 wraps); 15; the ragged last layers
    dict(K=16, NOUT=16, groups=1, in_pad=4, out_pad=4),
    dict(K=48, NOUT=128, groups=2, in_pad=12, out_pad=4),
    dict(K=16, NOUT=144, groups=1, in_pad=4, out_pad=0),
    dict(K=64, NOUT=240, groups=1, in_pad=4, out_pad=4),
    dict(K=128, NOUT=12, groups=2, in_pad=36, out_pad=4),
    dict(K=16, NOUT=1, groups=1, in_pad=12, out_pad=7),
    # blocks<2>: 16 blocks; 17 (wave 0 wraps into a group with one dead block); 31 (the last group half dead)
    dict(K=48, NOUT=256, groups=1, in_pad=4, out_pad=4),
    dict(K=32, NOUT=272, groups=2, in_pad=12, out_pad=4),
    dict(K=16, NOUT=496, groups=1, in_pad=4, out_pad=8),
    # blocks<4>: 32 blocks; 33 (wave 0 wraps into a group with three dead blocks); 65 (two full trips and a third group with three dead)
    dict(K=48, NOUT=512, groups=1, in_pad=4, out_pad=4),
    dict(K=32, NOUT=528, groups=1, in_pad=36, out_pad=4),
    dict(K=16, NOUT=1040, groups=2, in_pad=4, out_pad=4),
    # long K
    dict(K=528, NOUT=16, groups=1, in_pad=4, out_pad=4),
    dict(K=1040, NOUT=16, groups=1, in_pad=4, out_pad=0),
    dict(K=1040, NOUT=12, groups=2, in_pad=12, out_pad=4),
)

# Step 3's nets: (num_obs, actor hidden, critic hidden)
NETS = (
    (16, (144, 272), (16,)),
    (64, (528, 16, 240), (496,)),
    (48, (1040,), (1040, 16)),                                    # more than 64 KB of LDS
    (48, (16, 528, 16, 528, 16, 16, 16), (512, 256, 128)),       # the actor has eight layers (kMaxLayers)
)
WIDE_NET, NARROW_NET = NETS[2], (48, (16,), (16,))
CHAIN_ROWS = (1, 16, 17, 33)

WORST = {}                                                        # (NB, wrapped, dead) -> largest error / bound seen, printed as evidence
WORST_ELU = [0.0]


# ------------------------------------------------------------------ layer's dispatch and the LDS of a net, restated (host only)

def dispatch(nout, waves=WAVES):
    """policy::layer for NOUT outputs: the block count, NB (blocks per wave and trip), the trips of each wave, the dead blocks of each group."""
    nblocks = (nout + 15) // 16
    nb = 4 if nblocks >= 4 * waves else 2 if nblocks >= 2 * waves else 1
    groups = -(-nblocks // nb)
    return dict(nblocks=nblocks, NB=nb, groups=groups, trips=[len(range(w, groups, waves)) for w in range(waves)],
                dead=[max(0, (g + 1) * nb - nblocks) for g in range(groups)])


def branches(nout, waves=WAVES):
    """The (NB, wrapped, dead) classes of the groups that layer runs for NOUT outputs: wrapped = a wave's second or later trip, dead = the group holds a
    block past the last."""
    d = dispatch(nout, waves)
    return {(d["NB"], g >= waves, d["dead"][g] > 0) for g in range(d["groups"])}


def column_branch(nout, waves=WAVES):
    """Per output column, the index into sorted(branches(nout)) of the group that computes it."""
    d = dispatch(nout, waves)
    order = sorted(branches(nout, waves))
    g = np.arange(nout) // 16 // d["NB"]
    return order, np.array([order.index((d["NB"], gi >= waves, d["dead"][gi] > 0)) for gi in g])


def net_dims(net):
    num_obs, actor, critic = net
    return [num_obs, *actor, 12], [num_obs, *critic, 1]


def lds_bytes(dims):
    """policy::lds_bytes: activations alternate between two buffers, each as wide as its widest layer plus kPad."""
    return 4 * ROWS * (max(dims[0::2]) + PAD + max(dims[1::2]) + PAD)


def net_lds_bytes(net):
    return max(lds_bytes(d) for d in net_dims(net))


# ------------------------------------------------------------------ inputs and the float64 reference (host only)

def mag_range(K):
    """Magnitudes +-[lo, hi]: a single product of at least lo^2 has to stay 3 x above gamma_{K+1} times a sum of up to K hi^2, so the range narrows with K."""
    return (0.5, 2.0) if K <= 128 else (0.7, 1.4) if K <= 528 else (0.9, 1.1)


@functools.lru_cache(maxsize=None)
def layer_case(i):
    c = CASES[i]
    K, NOUT, rows = c["K"], c["NOUT"], ROWS * c["groups"]
    lo, hi = mag_range(K)
    rng = np.random.default_rng(7000 + i)
    X, W, b = draw(rng, (rows, K), 1.3, lo, hi), draw(rng, (NOUT, K), 10.0 / np.sqrt(K) / 1.3, lo, hi), draw(rng, (NOUT,), 4.0, lo, hi)
    Xd, Wd, bd = X.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    exact = Xd @ Wd.T + bd
    bound = gamma(K + 1) * (np.abs(Xd) @ np.abs(Wd).T + np.abs(bd))
    what = f"layer case {i} (K = {K}, NOUT = {NOUT})"
    min_term = np.minimum(np.outer(np.abs(Xd).min(1), np.abs(Wd).min(1)), np.abs(bd)[None, :])      # (a lower bound of the smallest term)
    assert (min_term >= 3.0 * bound).all(), f"{what}: a term under 3 x its bound, ratio {(min_term / bound).min():.2f}"
    assert min_term.min() >= 2.0 ** -126, what
    assert (exact > bound).any() and (exact < -bound).any(), f"{what}: one ELU branch only"
    return dict(K=K, NOUT=NOUT, rows=rows, X=X, W=W, b=b, exact=exact, bound=bound)


# ------------------------------------------------------------------ the harness

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = tmp_path_factory.mktemp("policy_layer_harness")
    so = d / "policy_layer_harness.so"
    subprocess.run([HIPCC, *HIPCC_FLAGS, "-I", CSRC, HARNESS, "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.policy_layer_harness_constants.argtypes = [C.c_void_p]; L.policy_layer_harness_constants.restype = None
    L.policy_layer_harness_lds_bytes.argtypes = [C.c_int, C.c_int]; L.policy_layer_harness_lds_bytes.restype = C.c_longlong
    L.policy_layer_harness_launch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.policy_layer_harness_launch.restype = C.c_int
    k = (C.c_int * 4)()
    L.policy_layer_harness_constants(k)
    assert tuple(k) == (64 * WAVES, WAVES, ROWS, PAD), f"policy::kThreads, kWaves, kRows, kPad are {tuple(k)}: CASES was chosen for eight waves"
    return L


def _launch(harness, src, in_stride, out, out_stride, W, b, K, NOUT, elu, groups):
    rc = harness.policy_layer_harness_launch(src.data_ptr(), in_stride, out.data_ptr(), out_stride, W.data_ptr(), b.data_ptr(), K, NOUT, elu, groups, None)
    assert rc == 0, f"the harness refused or failed the launch ({harness.policy_layer_harness_lds_bytes(in_stride, out_stride)} bytes of LDS): {rc}"


def _at_the_end(a, lead=64):
    """a on the device as the last a.size floats of a sentinel-filled allocation (16-byte aligned: lead is a multiple of 4 floats).  Returns the
    allocation (to keep it alive and to check its lead) and the view."""
    buf = _sentinel(lead + a.size)
    view = buf[lead:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _poisoned_rows(a, stride):
    """a [rows][K] on the device inside [rows][stride] of NaN."""
    buf = np.full((a.shape[0], stride), np.nan, np.float32)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).to(DEV)


# ------------------------------------------------------------------ step 2: one layer against float64

@pytest.mark.parametrize("case", range(len(CASES)))
def test_layer_matches_float64(harness, case):
    c, o = CASES[case], layer_case(case)
    K, NOUT, rows = o["K"], o["NOUT"], o["rows"]
    in_stride, out_stride = K + c["in_pad"], NOUT + c["out_pad"]
    what = f"layer case {case} (K = {K}, NOUT = {NOUT}, strides {in_stride} / {out_stride})"
    src = _poisoned_rows(o["X"], in_stride)
    (wbuf, W), (bbuf, b) = _at_the_end(o["W"]), _at_the_end(o["b"])
    outs = {}
    for elu in (0, 1):
        out = _sentinel(rows, out_stride)
        _launch(harness, src, in_stride, out, out_stride, W, b, K, NOUT, elu, c["groups"])
        torch.cuda.synchronize()
        _untouched(out, _region((rows, out_stride), rows, NOUT), f"{what} elu {elu}")
        outs[elu] = out.cpu().numpy()[:, :NOUT]
    assert (_bits(wbuf)[:64] == SENTINEL).all() and (_bits(bbuf)[:64] == SENTINEL).all(), what
    p, y = outs[0], outs[1]
    assert np.isfinite(p).all(), f"{what}: a NaN or an infinity reached the result"
    ratio = np.abs(p.astype(np.float64) - o["exact"]) / o["bound"]
    order, col = column_branch(NOUT)
    for k, key in enumerate(order):
        WORST[key] = max(WORST.get(key, 0.0), float(ratio[:, col == k].max()))
    print(f"{what}: largest error / bound {ratio.max():.3f}; per (NB, wrapped, dead) so far " + ", ".join(f"{k}: {v:.3f}" for k, v in sorted(WORST.items())))
    bad = ratio > 1.0
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside their bound, first at {tuple(np.argwhere(bad)[0])}, worst ratio {ratio.max():.3f}"
    pos = p > 0
    assert pos.any() and (~pos).any(), f"{what}: one ELU branch only"
    assert (y[pos].view(np.int32) == p[pos].view(np.int32)).all(), f"{what}: ELU changed a positive pre-activation"
    want = np.expm1(p[~pos].astype(np.float64))
    off = np.abs(y[~pos].astype(np.float64) - want) / ulp32(want)
    WORST_ELU[0] = max(WORST_ELU[0], float(off.max()))
    print(f"{what}: ELU off by at most {off.max():.3f} ulp over {int((~pos).sum())} elements, {int((p < -17.5).sum())} of them below -17.5; so far {WORST_ELU[0]:.3f}")
    assert (off <= 2.0).all(), f"{what}: ELU off by {off.max():.3f} ulp"


# ------------------------------------------------------------------ step 3: the production kernels equal the chain of harness layers

@functools.lru_cache(maxsize=None)
def _models(net):
    """One random actor-critic on the device and the WeightPolicy of its actor."""
    from rl_mpc_locomotion_amd import ppo as P
    from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
    num_obs, actor, critic = net
    torch.manual_seed(4000 + num_obs + len(actor) + 10 * len(critic))
    ac = P.ActorCritic(num_obs, 12, actor, critic)
    with torch.no_grad():
        for p in ac.parameters():
            if p.dim() == 1 and p is not ac.std:
                p.copy_(torch.randn_like(p) * 0.1)
        ac.actor[-1].bias.copy_(torch.randn(12))                  # raw actions on both sides of the clamp
        ac.std.copy_(torch.rand(12) * 1.95 + 0.05)
    pol = WeightPolicy.from_state_dict(ac.state_dict(), device=DEV)
    return ac.to(DEV), pol


def _obs(n, num_obs, seed):
    return (torch.randn((n, num_obs), generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


def _stride(width):
    return (width + 3) // 4 * 4 + PAD


def _chain(harness, seq, obs):
    """obs [n, num_obs] through the Linear layers of an nn.Sequential with the harness, layer by layer: the device output of layer l, sentinel padding
    included (a NaN), is the input of layer l + 1.  Rows past n are zero, as the production kernels fill them."""
    linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
    n, d0 = obs.shape
    groups = -(-n // ROWS)
    cur = torch.full((groups * ROWS, _stride(d0)), float("nan"), dtype=torch.float32, device=DEV)
    cur[:, :d0] = 0.0
    cur[:n, :d0] = obs
    for l, m in enumerate(linears):
        K, NOUT = m.in_features, m.out_features
        assert cur.shape[1] == _stride(K)
        out = _sentinel(groups * ROWS, _stride(NOUT))
        _launch(harness, cur, _stride(K), out, _stride(NOUT), m.weight, m.bias, K, NOUT, int(l + 1 < len(linears)), groups)
        cur = out
    torch.cuda.synchronize()
    return cur[:n, :linears[-1].out_features].contiguous()


@pytest.mark.parametrize("net", range(len(NETS)))
def test_production_kernels_equal_the_chain_of_layers(harness, net):
    from rl_mpc_locomotion_amd.weight_policy import MPC_PARAM_CONST, MPC_PARAM_SCALE
    ac, pol = _models(NETS[net])
    num_obs = NETS[net][0]
    if NETS[net] == WIDE_NET:
        assert net_lds_bytes(NETS[net]) > 64 * 1024
    clamped = free = 0
    for n in CHAIN_ROWS:
        what = f"net {NETS[net]} n = {n}"
        obs = _obs(n, num_obs, seed=100 * net + n)
        mean, value = _chain(harness, ac.actor, obs), _chain(harness, ac.critic, obs)
        assert torch.isfinite(mean).all() and torch.isfinite(value).all(), what
        weights, raw = pol.step(obs, return_actions=True)
        out = ac.act(obs, seed=5, step=n)
        torch.cuda.synchronize()
        assert torch.equal(raw, mean), f"{what}: WeightPolicy.step's raw actions differ from the chain of layers"
        assert torch.equal(ac.act_inference(obs), mean), f"{what}: act_inference differs from the chain of layers"
        assert torch.equal(out["mu"], mean), f"{what}: act's mean differs from the chain of layers"
        assert torch.equal(ac.evaluate(obs), value), f"{what}: evaluate differs from the chain of layers"
        assert torch.equal(out["values"], value), f"{what}: act's values differ from the chain of layers"
        # weights = clamp(a, -1, 1) * scale + shift: a float32 product, then a float32 sum on the host; the kernel may fuse the two (one ulp)
        a = raw.cpu().numpy()
        want = np.clip(a, np.float32(-1), np.float32(1)) * np.asarray(MPC_PARAM_SCALE, np.float32) + np.asarray(MPC_PARAM_CONST, np.float32)
        assert want.dtype == np.float32
        off = np.abs(weights.cpu().numpy().astype(np.float64) - want) / ulp32(want)
        assert (off <= 1.0).all(), f"{what}: weights off by {off.max():.2f} ulp from clamp(a, -1, 1) * scale + shift"
        clamped, free = clamped + int((np.abs(a) > 1).sum()), free + int((np.abs(a) < 1).sum())
    assert clamped and free, f"net {NETS[net]}: the clamp was not exercised both ways ({clamped} / {free})"


# ------------------------------------------------------------------ step 4: two live handles of different LDS size

def _fresh_actor_critic(net, seed):
    from rl_mpc_locomotion_amd import ppo as P
    torch.manual_seed(seed)
    return P.ActorCritic(net[0], 12, net[1], net[2]).to(DEV)


def _actor_critic_wide_then_narrow(wide_net, narrow_net, seed):
    """33 rows (two full workgroups and a partial one) through the wide handle, then a narrow handle is bound and run, then the wide one again on
    the same rows: it succeeds and answers bit for bit the same."""
    wide, narrow = _fresh_actor_critic(wide_net, seed), _fresh_actor_critic(narrow_net, seed + 1)
    obs = _obs(33, 48, seed=seed + 8)
    keys = ("actions", "actions_log_prob", "values", "mu", "sigma")
    before = {k: v.clone() for k, v in wide.act(obs, seed=3, step=1).items()}
    v_before, m_before = wide.evaluate(obs).clone(), wide.act_inference(obs).clone()
    assert all(torch.isfinite(before[k]).all() for k in keys)
    small = narrow.act(obs, seed=3, step=1)                                      # creates and binds the narrow handle
    assert torch.isfinite(small["mu"]).all() and not torch.equal(small["mu"], before["mu"])
    after = wide.act(obs, seed=3, step=1)
    torch.cuda.synchronize()                                                     # (a refused launch shows here at the latest)
    for k in keys:
        assert torch.equal(after[k], before[k]), k
    assert torch.equal(wide.evaluate(obs), v_before) and torch.equal(wide.act_inference(obs), m_before)
    assert torch.equal(narrow.act(obs, seed=3, step=1)["mu"], small["mu"])


def _weight_policy_wide_then_narrow(wide_net, narrow_net, seed):
    """The same for mlp_kernel: mpc_policy_create of a narrow net after a wide one."""
    from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
    wide_sd, narrow_sd = _fresh_actor_critic(wide_net, seed).state_dict(), _fresh_actor_critic(narrow_net, seed + 1).state_dict()
    obs = _obs(33, 48, seed=seed + 7)
    wide = WeightPolicy.from_state_dict(wide_sd, device=DEV)
    w_before, a_before = (t.clone() for t in wide.step(obs, return_actions=True))
    assert torch.isfinite(w_before).all() and torch.isfinite(a_before).all()
    narrow = WeightPolicy.from_state_dict(narrow_sd, device=DEV)                 # its smaller need raises nothing: the limit stays the wide net's
    w_small = narrow.step(obs).clone()
    assert torch.isfinite(w_small).all() and not torch.equal(w_small, w_before)
    w_after, a_after = wide.step(obs, return_actions=True)
    torch.cuda.synchronize()
    assert torch.equal(w_after, w_before) and torch.equal(a_after, a_before)
    assert torch.equal(narrow.step(obs), w_small)


def test_a_wide_actor_critic_survives_the_bind_of_a_narrow_one():
    """ac_kernel's dynamic-LDS limit is one per device and kernel and only grows: the narrow handle's bind must not take the wide handle's LDS away."""
    assert net_lds_bytes(WIDE_NET) > 64 * 1024 > net_lds_bytes(NARROW_NET)
    _actor_critic_wide_then_narrow(WIDE_NET, NARROW_NET, 1)


def test_a_wide_weight_policy_survives_the_creation_of_a_narrow_one():
    _weight_policy_wide_then_narrow(WIDE_NET, NARROW_NET, 3)


# The same two properties at the LDS need this project has recorded as over a kernel's default limit: 69 632 bytes, the deployed recurrent policy's.
# 48 observations and hidden widths (544, 544) are the smallest multiples of 16 that reach it: 16 (544 + 4 + 544 + 4) floats = 70 144 bytes.
NEED = 69632
NEED_NET, SMALL_NET = (48, (544, 544), (544, 544)), (48, (32,), (32,))


def test_the_need_net_is_the_smallest_that_reaches_the_recorded_need():
    assert net_lds_bytes(NEED_NET) == 70144 >= NEED > net_lds_bytes((48, (528, 528), (528, 528))) and net_lds_bytes(SMALL_NET) < 64 * 1024


def test_a_wide_actor_critic_keeps_its_launches_after_the_bind_of_a_narrow_one():
    _actor_critic_wide_then_narrow(NEED_NET, SMALL_NET, 11)


def test_a_wide_weight_policy_keeps_its_launches_after_the_creation_of_a_narrow_one():
    _weight_policy_wide_then_narrow(NEED_NET, SMALL_NET, 13)
